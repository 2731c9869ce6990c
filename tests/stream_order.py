"""Stream order under a deep queue: the helper of tests/test_stream_order_gpu.py.

The library's `_dev` entry points do not synchronise: a caller enqueues call after call and waits once.  The parity tests
never do that -- a download, a state getter or a sync follows every call, so the host is never more than one call ahead of
the device, and the machinery that makes a deep queue safe (the staging ring's guard, the cached tables, the oversize path,
buffers reused from launch to launch, host mirrors of device state, setters that drain) never has anything to do.  Here
the stream is held by one long kernel (the plug), the calls under test are enqueued behind it with no wait, the test makes
sure the plug was still running when the last of them had been enqueued, and what comes out is compared, byte for byte, with
the same calls made one at a time.

    hold(ctx)                    one long single-wave kernel on ctx's stream
    assert_deep(ctx, what)       the queue is still held (fails otherwise: a test must not pass by having waited)
    deep_vs_stepwise(make, script)   a script of setters and calls, stepwise and deep, equal in every byte

The plug is an ADPCM encode of PLUG_N samples on one channel: a serial recurrence on one lane (kg_wire.hip).  It runs on
a second context made over the SAME stream (Context(device, stream=ctx.stream)), with its own coder object, buffers,
staging ring and channel-list cache, so it shares nothing with the module under test but the stream, and it does not move
the ring position of the context under test: a test's k-th upload is upload k of its ring.  Its channel list is staged once
when the plug is made; every hold() after that is a cache hit: no upload, no wait.

PLUG_N was chosen from a measurement on the MI355X (profiles/stream_order.txt): about 115 ns a sample, 15 ms at 2^17 and 30 ms at
2^18, against 2.2 ms for the longest burst of host work any test puts behind a plug.  Four times the burst is the bar (a slow
host core, Python jitter); 2^18 leaves thirteen.
"""
import contextlib
import time

import numpy as np
import pytest

from flydog_sdr_gps_amd import Adpcm, Context

PLUG_N = 1 << 18
FILL = 0x5A                      # what an output region holds before any call writes it

# (what, seconds of host time between the hold() and this assert_deep, the plug was still running, chained) of every assert_deep
# made in this process: what profiles/stream_order.txt reports as the bursts
BURSTS = []


class _Plug:
    def __init__(self, ctx, n):
        self.n = int(n)
        self.ctx = Context(ctx.device, stream=ctx.stream)
        self.adpcm = None
        self.d_in = self.d_out = None
        try:
            self.adpcm = Adpcm(self.ctx, nchan=1)
            self.d_in, self.d_out = self.ctx.alloc(2 * self.n), self.ctx.alloc(self.n // 2)
            t = np.arange(self.n)
            self.ctx.upload(self.d_in, (9000 * np.sin(2 * np.pi * 0.013 * t)).astype(np.int16))
            self.adpcm.encode_dev([0], self.d_in, self.n, 2, self.d_out, self.n // 2)     # the list's one upload, and the cache's growth
            self.ctx.sync()
        except Exception:
            self.close()
            raise
        self.t0 = None

    def hold(self, chained=False):
        # (the coder's state runs on from hold to hold: the plug's output is never read)
        self.adpcm.encode_dev([0], self.d_in, self.n, self.n, self.d_out, self.n // 2)
        self.t0, self.chained = time.perf_counter(), chained

    def close(self):
        if self.adpcm is not None:
            self.adpcm.close()
        for d in (self.d_in, self.d_out):
            if d:
                self.ctx.free(d)
        self.d_in = self.d_out = None
        self.ctx.close()


def plug_of(ctx, n=None):
    p = getattr(ctx, "_stream_order_plug", None)
    if p is None or (n is not None and p.n != n):
        if p is not None:
            p.close()
        p = ctx._stream_order_plug = _Plug(ctx, PLUG_N if n is None else n)
    return p


def hold(ctx, n=None, chained=False):
    """One long kernel on ctx's stream: what is enqueued behind it waits.  (The first hold() on a context makes the plug, which
    synchronises: call it before the calls that must stay in the queue.)  chained: the plug before this one is still running and
    the calls behind this one will wait for it at the ring's guard, as they should: their burst includes that wait."""
    plug_of(ctx, n).hold(chained)


def assert_deep(ctx, what):
    """The plug of the last hold() is still running: everything enqueued since is still in the queue."""
    deep = not ctx.poll()
    p = getattr(ctx, "_stream_order_plug", None)
    BURSTS.append((str(what), time.perf_counter() - p.t0 if p is not None and p.t0 is not None else float("nan"), deep,
                   bool(p is not None and getattr(p, "chained", False))))
    if not deep:
        pytest.fail("the queue was not deep at %s: lengthen the plug" % (what,))


@contextlib.contextmanager
def fresh_ctx():
    """A context of the test's own (the session's gpu_ctx has an arbitrary ring position), closed with its plug."""
    ctx = Context(0)
    try:
        yield ctx
    finally:
        p = getattr(ctx, "_stream_order_plug", None)
        if p is not None:
            p.close()
            ctx._stream_order_plug = None
        ctx.close()


def measure_plug(n, reps=3):
    """-> milliseconds the plug of n samples holds a stream (the shortest of reps), on a context of its own"""
    with fresh_ctx() as ctx:
        plug_of(ctx, n)
        best = None
        for _ in range(reps):
            ctx.timer_start()
            hold(ctx, n)
            ms = ctx.timer_stop()
            best = ms if best is None else min(best, ms)
        return best


def same_bits(a, b):
    """equal in type, shape and every bit (NaNs included); containers element by element"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def snapshot(v):
    """a copy of what a call returned on the host (the next call may reuse the array)"""
    if isinstance(v, dict):
        return {k: snapshot(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [snapshot(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.copy()
    return v


class Run:
    """what one run of a script left: out (uint8, the whole output allocation), rets (one per action), state (the getters)"""

    def __init__(self, out, rets, state):
        self.out, self.rets, self.state = out, rets, state


def run_script(make, script, deep):
    """One run on a fresh context.  make(ctx) -> an object with
        out_bytes      the size of the one output allocation (the helper fills it with FILL and sets .d_out)
        getters()      -> every state getter's answer, called once the run has drained
        close()
    having uploaded every input.  script: [(kind, fn)], fn(st) -> what the call returns on the host (or None), kind one of
        "call"   an enqueue-only entry point
        "set"    a setter, a reset, a getter, or a call that drains the stream by design (the first use or the growth of a cached
                 table): the queue must be deep right in front of it, and a new plug goes in front of the next call
        "host"   a command that changes host state only and neither enqueues nor waits (kg_fftext's and kg_iqd's commands)
        "deep"   no action: the queue must be deep here (fn is the name of the place), and the next call gets a plug of its own
                 in front, enqueued while this one still runs: the queue is never empty between the two stretches.
    A stretch of calls behind one plug may make at most KG_RING_SLOTS / 2 = 16 ring uploads once the ring has wrapped (32
    uploads on the context): the guard of upload j waits for upload j - 16, and with that one behind the plug the host waits
    for the plug, as it should.  Scripts place a "deep" mark before that happens."""
    with fresh_ctx() as ctx:
        st = make(ctx)
        d_out = None
        try:
            out = np.full(int(st.out_bytes), FILL, np.uint8)
            d_out = st.d_out = ctx.alloc(out.nbytes)
            ctx.upload(d_out, out)
            rets, calls_behind_plug, chained = [], 0, False
            for i, (kind, fn) in enumerate(script):
                if kind == "deep":
                    if deep:
                        assert calls_behind_plug, "script: no call stands behind a plug at %r" % (fn,)
                        assert_deep(ctx, fn)
                        calls_behind_plug, chained = 0, True
                    rets.append(None)
                    continue
                assert kind in ("call", "set", "host"), kind
                if kind == "host":
                    rets.append(snapshot(fn(st)))
                    continue
                if deep and kind == "set" and calls_behind_plug:
                    assert_deep(ctx, "the last call in front of action %d" % i)
                    calls_behind_plug = 0
                if kind == "set":
                    chained = False                  # it drains: the next plug has the stream to itself
                if deep and kind == "call" and not calls_behind_plug:
                    hold(ctx, chained=chained)       # a plug in front of every stretch of calls
                rets.append(snapshot(fn(st)))
                if not deep:
                    ctx.sync()
                elif kind == "call":
                    calls_behind_plug += 1
            if deep and calls_behind_plug:
                assert_deep(ctx, "the last action")
            ctx.download(d_out, out)
            return Run(out, rets, snapshot(st.getters()))
        finally:
            if d_out:
                ctx.free(d_out)
            st.close()


def deep_vs_stepwise(make, script):
    """The script one action at a time (a sync after each), and again with every action enqueued behind a plug and one download at
    the end: every byte of the output allocation, every value a call returned on the host and every state getter must be equal.
    -> the stepwise Run (for the caller's reference check: deep == stepwise, stepwise == reference)"""
    step = run_script(make, script, deep=False)
    held = len(BURSTS)
    deep = run_script(make, script, deep=True)
    assert len(BURSTS) > held, "the script has no call behind a plug: nothing ran deep"
    assert step.out.size == deep.out.size
    diff = np.nonzero(step.out != deep.out)[0]
    assert diff.size == 0, "deep and stepwise outputs differ in %d bytes, the first at %d" % (diff.size, diff[0])
    for i, (a, b) in enumerate(zip(step.rets, deep.rets)):
        assert same_bits(a, b), "action %d returned %r stepwise and %r deep" % (i, a, b)
    assert same_bits(step.state, deep.state), "the final state differs: %r stepwise, %r deep" % (step.state, deep.state)
    return step
