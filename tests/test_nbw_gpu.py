"""kg_post's Wild noise blanker (NB_WILD: rx/rx_sound.cpp:922-931 -> rx/Teensy/NB_Wild.cpp) on the GPU: every scenario of
tests/golden/nbw_ref.npz (the reference's own commands and stage, tools/make_ref_nbw_golden.py) BIT-EXACT -- every int16 output
sample, every state value -- through kg_post_nbw_init / kg_post_set_nbw and kg_post_nbw_process_dev: all scenarios side by side in
one batch (out of place), each alone in place in calls of one, three and eight blocks; the fused pass of kg_post_process_dev equal
to the same audio without the stage followed by the standalone call (SSB, AM, SAM), a stereo mode untouched, the stage ahead of
NR_WDSP and of NR_SPECTRAL equal to the stages one after the other, rows without the stage byte-identical to a run that never heard
of it; the state semantics; the refusals, which leave the state untouched.  On a mismatch the failing block is diffed against the
host driver (which tests/test_nbw_cpu.py holds to the same golden)."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post
from flydog_sdr_gps_amd._lib import KiwiGpuError

from . import nbw_common as nc

pytestmark = pytest.mark.gpu
FS = 12000.0
KG_ERR_INVALID, KG_ERR_STATE = -2, -5


@pytest.fixture(scope="module")
def golden():
    return nc.load()


@pytest.fixture(scope="module")
def streams():
    return nc.pool()


def explain(g, name, y, streams, tmp_path):
    exe = nc.build_driver(tmp_path)
    want, _, _, _, rc = nc.run_driver(exe, nc.script(g, name), nc.scenario_input(g, name, streams), tmp_path)
    assert rc == 0
    bad = np.flatnonzero(y != want)
    return "first difference at block %d sample %d: got %d, host driver %d; %d samples differ" % (
        bad[0] // nc.BLK, bad[0] % nc.BLK, y[bad[0]], want[bad[0]], bad.size) if bad.size else "equal to the host driver"


def check(g, name, y, states, what, streams, tmp_path):
    try:
        nc.check_blocks(name, y, g, what)
    except AssertionError as e:
        raise AssertionError("%s -- %s" % (e, explain(g, name, y, streams, tmp_path)))
    nc.check_states(name, states, g, what)


def test_error_codes_are_the_headers():
    import os
    import re
    text = open(os.path.join(nc.ROOT, "include", "kiwigpu.h")).read()
    codes = dict(re.findall(r"\b(KG_ERR_[A-Z]+)\s*=\s*(-\d+)", text))
    assert int(codes["KG_ERR_INVALID"]) == KG_ERR_INVALID and int(codes["KG_ERR_STATE"]) == KG_ERR_STATE


def test_all_scenarios_side_by_side_bit_exact(gpu_ctx, golden, streams, tmp_path):
    """one channel per scenario, one batch per round over the channels whose next block runs the stage: vectors from 1 / 2 to 40 / 41
    side by side, channels leaving and re-entering the list; out of place"""
    names = nc.names(golden)
    assert len(names) >= 18
    P = Post(gpu_ctx, nchan=len(names) + 1)
    try:
        reps = [nc.Replay(P, ch + 1, nc.script(golden, n), nc.scenario_input(golden, n, streams)) for ch, n in enumerate(names)]
        live = list(reps)
        while live:
            batch = []
            for r in list(live):
                nxt = r.step()
                if nxt is None:
                    live.remove(r)
                elif nxt[1]:
                    batch.append((r, nxt[0]))
                else:
                    r.done(nxt[0])                      # stereo, or the switch off: the call site leaves the block alone
            if batch:
                y = P.nbw_process([r.ch for r, _ in batch], np.stack([b for _, b in batch]), in_place=False)
                for (r, _), row in zip(batch, y):
                    r.done(row)
        for n, r in zip(names, reps):
            check(golden, n, r.output(), r.states, "side by side", streams, tmp_path)
    finally:
        P.close()


@pytest.mark.parametrize("blocks", [1, 3, 8])
def test_each_scenario_alone_in_place(gpu_ctx, golden, streams, tmp_path, blocks):
    """each scenario on a fresh kg_post, in place, in calls of up to `blocks` blocks: a call is nb_Wild_process once per 512 samples"""
    for n in nc.names(golden):
        P = Post(gpu_ctx, nchan=3)
        try:
            r = nc.Replay(P, 2, nc.script(golden, n), nc.scenario_input(golden, n, streams))
            while True:
                nxt = r.step()
                if nxt is None:
                    break
                if not nxt[1]:
                    r.done(nxt[0])
                    continue
                run = [nxt[0]]
                while len(run) < blocks and r.peek_is_block():
                    run.append(r.step()[0])
                r.done(P.nbw_process([2], np.concatenate(run)[None, :])[0])
            check(golden, n, r.output(), r.states, "alone, %d blocks a call" % blocks, streams, tmp_path)
        finally:
            P.close()


def fir_input(n, seed, amp=0.3):
    """a CFastFIR-like block: two tones, noise, and a few strong single-sample clicks"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = amp * (np.exp(2j * np.pi * 1000.0 * t) + 0.6 * np.exp(2j * np.pi * (300.0 + 50 * (seed % 7)) * t)) + 0.02 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for p in r.integers(0, n, 3):
        x[p] += 3.0 * amp * np.exp(2j * np.pi * r.random())
    return x.astype(np.complex64)


def configure(P, ch, mode):
    P.set_agc(ch, True, False, -100, 50, 6, 1000, FS)
    P.set_smeter(ch, FS)
    P.set_am_passband(ch, -2700.0, 2700.0, FS)
    P.set_mode(ch, mode)
    P.reset(ch)
    P.squelch_setup(ch, FS)
    P.squelch_set(ch, 0, 0)


SPEC = "spectral"
# channel -> (mode, Wild vector or None, NR algo, {type: params}, NR enables (denoise, auto-notch))
PLAN = {
    0: (post.MODE_SSB, [0.95, 10, 7], post.NR_OFF, {}, (0, 0)),
    1: (post.MODE_AM, [2.0, 16, 12], post.NR_OFF, {}, (0, 0)),
    2: (post.MODE_SSB, None, post.NR_OFF, {}, (0, 0)),
    3: (post.MODE_IQ, [0.95, 10, 7], post.NR_OFF, {}, (0, 0)),                             # stereo: the stage is skipped
    4: (post.MODE_SAM, [0.95, 40, 41], post.NR_OFF, {}, (0, 0)),
    5: (post.MODE_SSB, [0.95, 10, 7], post.NR_WDSP, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1)),
    6: (post.MODE_SSB, [1.5, 8, 5], SPEC, {0: [1, 0.95, 1000]}, (0, 0)),
    7: (post.MODE_SAS, [0.95, 10, 7], post.NR_OFF, {}, (0, 0)),                            # stereo: skipped
    8: (post.MODE_SSB, None, post.NR_WDSP, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1)),
    9: (post.MODE_SSB, [0.95, 1, 2], post.NR_OFF, {}, (0, 0)),
}


def set_up(P, ch, plan, wild, nr_enable):
    mode, vec, algo, params, en = plan
    configure(P, ch, mode)
    if algo == SPEC:
        P.nrs_passband(ch, 300.0, 2700.0)
        P.nrs_select(ch)
    else:
        P.set_nr_algo(ch, algo)
    for t, vals in params.items():
        for k, v in enumerate(vals):
            P.set_nr_param(ch, t, k, v)
    if nr_enable:
        for t in (0, 1):
            if en[t]:
                P.set_nr_enable(ch, t, en[t])
    if vec is not None and wild:
        P.nbw_init(ch, vec)


def test_fused_pass_equals_the_stages_one_after_the_other(gpu_ctx):
    """A: kg_post_process_dev with everything on.  B: the pass with the Wild stage and NR off, then the stages by hand on the rows:
    nb_Wild_process, then the NR switch's (auto-notch, denoiser; or the spectral one).  C: a kg_post that never heard of the Wild
    stage -- its rows for channels without the stage equal A's byte for byte."""
    n = 512
    A, B, Cc = Post(gpu_ctx, nchan=10), Post(gpu_ctx, nchan=10), Post(gpu_ctx, nchan=10)
    try:
        for ch, plan in PLAN.items():
            set_up(A, ch, plan, True, True)
            set_up(B, ch, plan, True, False)
            set_up(Cc, ch, plan, False, True)
            if plan[1] is not None:
                A.set_nbw(ch, 1)
        chans = list(PLAN)
        changed = {ch: False for ch in chans}
        for blk in range(10):
            x = np.stack([fir_input(n, 10 * blk + ch) for ch in chans])
            ya, da, ga = A.process(chans, x)
            for ch, plan in PLAN.items():
                if plan[2] == SPEC:
                    B.set_nr_algo(ch, post.NR_OFF)
            yb, db, gb = B.process(chans, x)
            yc, dc, gc = Cc.process(chans, x)
            for i, ch in enumerate(chans):
                mode, vec, algo, params, en = PLAN[ch]
                assert np.array_equal(ga[i].view(np.uint32), gb[i].view(np.uint32)), ch
                assert np.array_equal(da[i].view(np.uint32), dc[i].view(np.uint32)), ch
                if algo == SPEC:
                    B.nrs_select(ch)
                if vec is None or mode in post.STEREO_MODES:
                    assert np.array_equal(ya[i], yc[i]), (ch, blk, "a row without the stage changed")
                    continue
                want = B.nbw_process([ch], yb[i][None, :])
                changed[ch] |= not np.array_equal(want[0], yb[i])
                if algo == post.NR_WDSP:
                    want = B.nr_process([ch], post.NR_AUTONOTCH, want)
                    want = B.nr_process([ch], post.NR_DENOISE, want)
                elif algo == SPEC:
                    want = B.nrs_process([ch], want)
                assert np.array_equal(ya[i], want[0]), (ch, blk)
        for ch, plan in PLAN.items():
            sa, sb = A.nbw_state([ch]), B.nbw_state([ch])
            if plan[1] is None:
                assert not sa["hist"].any() and sa["ints"][0].tolist() == [0, 0, 0]
            elif plan[0] in post.STEREO_MODES:
                assert not sa["hist"].any(), (ch, "a stereo channel's state advanced")
            else:
                assert changed[ch], (ch, "the stage changed nothing")
                assert np.array_equal(sa["hist"].view(np.uint32), sb["hist"].view(np.uint32)) and sa["hist"].any(), ch
    finally:
        A.close(); B.close(); Cc.close()


def test_fused_batches_of_several_blocks_and_changing_lists(gpu_ctx):
    """a 1024-sample pass is two blocks; channels entering and leaving the list keep their own state"""
    M, alone = Post(gpu_ctx, nchan=3), [Post(gpu_ctx, nchan=1) for _ in range(3)]
    vecs = [[0.95, 10, 7], [1.2, 40, 41], [0.95, 3, 2]]
    try:
        for ch in range(3):
            for P, c in ((M, ch), (alone[ch], 0)):
                configure(P, c, post.MODE_SSB)
                P.nbw_init(c, vecs[ch])
                P.set_nbw(c, 1)
        for blk, (lst, n) in enumerate([([0, 1, 2], 512), ([2, 0], 1024), ([1], 512), ([0, 1, 2], 1024), ([2, 1, 0], 512)] * 2):
            x = np.stack([fir_input(n, 100 * blk + ch) for ch in lst])
            y, _, _ = M.process(lst, x)
            for i, ch in enumerate(lst):
                ya = np.concatenate([alone[ch].process([0], x[i][None, k:k + 512])[0][0] for k in range(0, n, 512)])
                assert np.array_equal(y[i], ya), (blk, ch)
        for ch in range(3):
            a, b = M.nbw_state([ch]), alone[ch].nbw_state([0])
            for k in a:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ch, k)
            assert a["hist"].any()
    finally:
        M.close()
        for P in alone:
            P.close()


def test_state_semantics(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    try:
        configure(P, 0, post.MODE_SSB)
        s = P.nbw_state([0])
        assert s["ints"][0].tolist() == [0, 0, 0] and s["thresh"][0] == 0 and not s["hist"].any()
        P.nbw_init(0, [3.0])                                            # the client's first message: an unusable vector, stored
        assert P.nbw_state([0])["ints"][0].tolist() == [0, 0, 0] and P.nbw_state([0])["thresh"][0] == 3.0
        P.nbw_init(0, [3.0, 10.9])
        P.nbw_init(0, [3.0, 10.9, 7.2])                                 # (s1_t) truncates
        assert P.nbw_state([0])["ints"][0].tolist() == [10, 7, 0]
        P.set_nbw(0, 1)
        x = fir_input(512, 3)[None, :]
        y0 = P.process([0], x)[0]
        s1 = P.nbw_state([0])
        assert s1["ints"][0].tolist() == [10, 7, 1] and s1["hist"][0, :26].any() and not s1["hist"][0, 26:].any()
        P.set_mode(0, post.MODE_AM); P.set_mode(0, post.MODE_SSB)       # a mode change leaves state and switch alone
        assert P.nbw_state([0])["ints"][0].tolist() == [10, 7, 1]
        P.set_nbw(0, 0)                                                 # off: the pass leaves the state alone
        P.process([0], x)
        s2 = P.nbw_state([0])
        assert s2["ints"][0].tolist() == [10, 7, 0] and np.array_equal(s1["hist"].view(np.uint32), s2["hist"].view(np.uint32))
        P.set_nbw(0, 1)
        P.reset(0)                                                      # a new connection: the switch cleared, the state kept
        s3 = P.nbw_state([0])
        assert s3["ints"][0].tolist() == [10, 7, 0] and np.array_equal(s1["hist"].view(np.uint32), s3["hist"].view(np.uint32))
        P.set_nbw(0, 1)                                                 # the kept vector is usable
        P.nbw_init(0, [3.0, 10, 7])                                     # every init zeroes the history, the switch stays
        s4 = P.nbw_state([0])
        assert s4["ints"][0].tolist() == [10, 7, 1] and not s4["hist"].any()
        assert P.nbw_state([1])["ints"][0].tolist() == [0, 0, 0]        # the other channel never moved
        assert y0.shape == (1, 512)
    finally:
        P.close()


def test_refusals_leave_the_state_untouched(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    ctx = P.ctx
    try:
        def bad(code, f, *a):
            with pytest.raises(KiwiGpuError) as e:
                f(*a)
            assert e.value.status == code, (e.value.status, code, f.__name__, a)
        configure(P, 0, post.MODE_SSB)
        bad(KG_ERR_STATE, P.set_nbw, 0, 1)                              # never initialised: taps 0
        bad(KG_ERR_STATE, P.nbw_process, [0], np.zeros((1, 512), np.int16))
        for vec in ([3.0, 0, 7], [3.0, 41, 7], [3.0, 10, 1], [3.0, 10, 42], [np.nan, 10, 7], [np.inf, 10, 7], [3.0, 300, 7], [3.0, -3, 7]):
            P.nbw_init(0, vec)                                          # stored while the stage is off ...
            bad(KG_ERR_STATE, P.set_nbw, 0, 1)                          # ... and never run
            bad(KG_ERR_STATE, P.nbw_process, [0], np.zeros((1, 512), np.int16))
        bad(KG_ERR_INVALID, P.nbw_init, 2, [3.0, 10, 7])
        bad(KG_ERR_INVALID, P.set_nbw, -1, 1)
        P.nbw_init(0, [0.95, 10, 7])
        P.set_nbw(0, 1)
        x = fir_input(512, 5)[None, :]
        for _ in range(3):
            P.process([0], x)
        before = P.nbw_state([0])
        assert before["hist"].any() and before["ints"][0].tolist() == [10, 7, 1]
        for vec in ([0.95, 0, 7], [0.95, 10, 0], [np.nan, 10, 7], [0.95, 41, 7]):
            bad(KG_ERR_INVALID, P.nbw_init, 0, vec)                     # unusable while the switch is on: nothing changed
        bad(KG_ERR_INVALID, P.nbw_process, [0], np.zeros((1, 256), np.int16))       # nsamps % 512
        bad(KG_ERR_INVALID, P.nbw_process, [0], np.zeros((1, 768), np.int16))
        bad(KG_ERR_INVALID, P.nbw_process, [0], np.zeros((1, 512 * 9), np.int16))   # more than KG_NBW_MAX_SAMPLES
        bad(KG_ERR_INVALID, P.nbw_process, [0, 0], np.zeros((2, 512), np.int16))    # listed twice
        bad(KG_ERR_INVALID, P.nbw_process, [5], np.zeros((1, 512), np.int16))       # a bad channel
        d = ctx.alloc(8 * 1024)
        o = ctx.alloc(2 * 1024)
        try:
            bad(KG_ERR_INVALID, P.process_dev, [0], d, 512, 512, 0, 0, d, 512)      # the fused pass needs d_s16 ...
            bad(KG_ERR_INVALID, P.process_dev, [0], d, 256, 256, o, 0, 0, 256)      # ... and whole blocks
            bad(KG_ERR_INVALID, P.process_dev, [0], d, 768, 768, o, 0, 0, 768)
        finally:
            ctx.sync()
            ctx.free(d); ctx.free(o)
        after = P.nbw_state([0])
        for k in before:
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        P.process([0], fir_input(512, 6)[None, :])                      # and the channel goes on (another block: another history)
        assert not np.array_equal(P.nbw_state([0])["hist"].view(np.uint32), before["hist"].view(np.uint32))
        P.set_nbw(0, 0)
        y, _, _ = P.process([0], fir_input(256, 9)[None, :])            # with the switch off any block length passes again
        assert y.shape == (1, 256)
    finally:
        P.close()
