"""Every device entry point held to stream order under a deep queue (tests/stream_order.py has the method and the helper).

Section 2 below places calls at known positions of the staging machinery (kg_ctx.hip): the ring's wrap and its guard, the
oversize path, the cached channel lists of kg_adpcm and kg_post with their miss / hit / grow sequence, the waterfall's
WF_TABLE_WAYS-way frame tables with the blanker's reused buffers, and the acquisition's pair table kept in a ring slot across
calls.  Section 3 runs every stateful module's `_dev` calls, with setters between them, deep against stepwise
(deep_vs_stepwise), and holds the stepwise side to the module's reference, so that equality with the stepwise run is equality
with the reference.  Every comparison is an equality; assert_deep keeps a test from passing because the host had waited.

tests/test_stream_order_coverage_cpu.py keeps the list of entry points: one added to include/kiwigpu.h without a case here
fails there."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from flydog_sdr_gps_amd import (Adpcm, Aperture, Ddc, FastFir, NoiseBlanker, Post, RxDdc, Searcher, Waterfall, WfParams, eph, fftext, handoff, iqd, nav,
                                post, prn, sats, snd, synth, trk, wf, wire)
from flydog_sdr_gps_amd._lib import check, ptr
from flydog_sdr_gps_amd.ddc import rx_phase_inc
from tests import fftext_common as fc, iqd_common as ic, nav_model as nm, nb_signals, nbw_common, nrs_common, trk_common as tc
from tests.stream_order import FILL, assert_deep, deep_vs_stepwise, fresh_ctx, hold, same_bits

pytestmark = pytest.mark.gpu

PKT = wire.WF_PKT_MAX


def state_of(**kw):
    """what make(ctx) hands deep_vs_stepwise: attributes, and close() over the objects and device buffers listed"""
    st = types.SimpleNamespace(**kw)
    st.objects, st.buffers = [], []

    def close():
        for o in st.objects:
            o.close()
        for b in st.buffers:
            st.ctx.free(b)
    st.close = close
    if not hasattr(st, "getters"):
        st.getters = lambda: None
    return st


def dev(st, host):
    """a device copy of a host array, freed with the state"""
    host = np.ascontiguousarray(host)
    d = st.ctx.alloc(max(host.nbytes, 8))
    st.buffers.append(d)
    if host.nbytes:
        st.ctx.upload(d, host)
    return d


def region(run, off, dtype, shape):
    """the bytes a call was given at `off` of the output allocation, as an array"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return run.out[off:off + n].view(dtype).reshape(shape)


class Regions:
    """hands out aligned regions of the one output allocation"""

    def __init__(self):
        self.size = 0

    def take(self, nbytes, align=256):
        off = (self.size + align - 1) // align * align
        self.size = off + int(nbytes)
        return off


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the staging machinery
# ---------------------------------------------------------------------------------------------------------------------------------

def packet_infos(k, nrows=2):
    """infos that name call k: (x_bin_server, zoom, seq, use_compression) per row"""
    return [((k * 2654435761 + r * 40503) & 0x7FFFFFFF, (k + 7 * r) % 15, k, (k + r) % 3 != 0) for r in range(nrows)]


def check_packet(oracle, pkts, nbytes, row, info, what):
    want = oracle.wf_packet(row, *info)
    assert nbytes == want.size, (what, nbytes, want.size)
    assert np.array_equal(pkts[:want.size], want), what
    assert np.all(pkts[want.size:] == FILL), (what, "bytes behind the packet were written")


def test_ring_wrap(oracle):
    """100 two-row kg_wf_packets_dev calls, one ring upload each, on a fresh context: call k is upload k.  The guard of upload j waits
    for the event of upload j - 16 (from j = 32 on), so behind a plug enqueued ahead of call p the host runs free up to call
    max(31, p + 15) and the NEXT call must wait for the plug.  Plugs ahead of calls 0, 40 and 80; the queue must still be held behind
    calls 31, 55 and 95 -- with 32, 16 and 16 tables in flight, the ring full the first time -- and every packet of every call must
    be the oracle's for ITS rows and ITS infos: a slot overwritten before its copy ran would put a later call's table under an earlier
    call's rows."""
    ncall = 100
    rng = np.random.default_rng(100)
    rows = rng.integers(0, 256, (2 * ncall, 1024), dtype=np.uint8)
    rows[::7] = np.clip(120 + 60 * np.sin(np.arange(1024) / 9.0), 0, 255).astype(np.uint8)[None, :] + (np.arange(rows[::7].shape[0]) % 50)[:, None].astype(np.uint8)
    pk = np.full((2 * ncall, PKT), FILL, np.uint8)
    nbs = []
    with fresh_ctx() as ctx:
        d_rows, d_pk = ctx.alloc(rows.nbytes), ctx.alloc(pk.nbytes)
        try:
            ctx.upload(d_rows, rows)
            ctx.upload(d_pk, pk)
            for k in range(ncall):
                if k in (0, 40, 80):
                    hold(ctx)
                nbs.append(wire.wf_packets_dev(ctx, d_rows + 2048 * k, 1024, packet_infos(k), d_pk + 2 * PKT * k))
                if k in (31, 55, 95):
                    assert_deep(ctx, "call %d of the ring wrap" % k)
            ctx.download(d_pk, pk)
        finally:
            ctx.free(d_rows)
            ctx.free(d_pk)
    for k in range(ncall):
        for r, info in enumerate(packet_infos(k)):
            check_packet(oracle, pk[2 * k + r], int(nbs[k][r]), rows[2 * k + r], info, (k, r))


INFO_DTYPE = np.dtype([("x_bin_server", "<u4"), ("zoom", "<u4"), ("seq", "<u4"), ("use_compression", "<i4")])
assert INFO_DTYPE.itemsize == C.sizeof(wire.WfPktInfo)


def big_infos(n, seq, x0, phase):
    """n infos as the C structs in one array (built ahead of the calls, so that the two calls follow each other closely): zoom 0 --
    never compressed, a cheap kernel -- for all rows but those with r % 64 == phase, which are compressed at zoom 1 + r % 14"""
    a = np.zeros(n, INFO_DTYPE)
    r = np.arange(n)
    a["x_bin_server"] = (x0 + 3 * r) & 0xFFFFFFFF
    a["seq"] = seq
    a["use_compression"] = 1
    a["zoom"] = np.where(r % 64 == phase, 1 + r % 14, 0)
    return a


def test_oversize_tables(oracle):
    """Two consecutive kg_wf_packets_dev calls whose info tables (32 769 and 40 000 rows of 16 bytes) are larger than a ring slot: they
    take the context's one scratch buffer (kg_ctx_scratch_upload: drain, blocking copy), the second while the first call's kernel may
    still be reading it; a two-row ring call follows.  Behind a plug, with the tables built ahead.  Every packet of both calls carries
    ITS call's seq, x_bin and zoom: the uncompressed ones are compared with 16 header bytes built here plus the row, the
    compressed ones with the oracle."""
    n1, n2 = 32769, 40000
    rng = np.random.default_rng(101)
    rows = rng.integers(0, 256, (n2, 1024), dtype=np.uint8)
    infos = [big_infos(n1, 0x01010101, 1000, 0), big_infos(n2, 0x02020202, 5_000_000, 32)]
    small = packet_infos(7)
    ns = (n1, n2, 2)
    pk = np.full((sum(ns), PKT), FILL, np.uint8)
    nbs = [np.zeros(n, np.int32) for n in ns[:2]]
    with fresh_ctx() as ctx:
        d_rows, d_pk = ctx.alloc(rows.nbytes), ctx.alloc(pk.nbytes)
        try:
            ctx.upload(d_rows, rows)
            ctx.upload(d_pk, pk)
            hold(ctx)
            at = 0
            for a, nb in zip(infos, nbs):
                rc = ctx.lib.kg_wf_packets_dev(ctx.h, C.c_void_p(d_rows), 1024, a.size, a.ctypes.data_as(C.c_void_p), C.c_void_p(d_pk + at * PKT),
                                               PKT, nb.ctypes.data_as(C.c_void_p))
                assert rc == 0, ctx.lib.kg_last_error()
                at += a.size
            nbs.append(wire.wf_packets_dev(ctx, d_rows + 1024 * 5, 1024, small, d_pk + at * PKT))
            ctx.download(d_pk, pk)
        finally:
            ctx.free(d_rows)
            ctx.free(d_pk)
    at = 0
    for a, nb in zip(infos, nbs):
        n = a.size
        got = pk[at:at + n]
        comp = a["zoom"] != 0
        assert np.array_equal(nb, np.where(comp, 16 + 517, 16 + 1024))
        hdr = np.zeros((n, 4), "<u4")
        hdr[:, 0], hdr[:, 1], hdr[:, 2], hdr[:, 3] = 0x20462F57, a["x_bin_server"], a["zoom"], a["seq"]
        plain = ~comp
        assert np.array_equal(got[plain, :16], hdr.view(np.uint8).reshape(n, 16)[plain]), "a header of the other call's table"
        assert np.array_equal(got[plain, 16:16 + 1024], rows[:n][plain])
        assert np.all(got[plain, 16 + 1024:] == FILL)
        for r in np.nonzero(comp)[0]:
            check_packet(oracle, got[r], int(nb[r]), rows[r], tuple(int(a[f][r]) for f in INFO_DTYPE.names), (int(a["seq"][0]), int(r)))
        at += n
    for r, info in enumerate(small):
        check_packet(oracle, pk[at + r], int(nbs[2][r]), rows[5 + r], info, ("ring call", r))


# the order of lists of 2c and 2d: A, A (hit), B (miss), A, permuted A, shorter, longer, 1 100 channels (above the cache's 4 KiB: it
# grows, and drains to do so), A, B; then the order again without the long list, twice, and A, B: 30 calls
NBIG = 1100
LIST_A, LIST_B, LIST_PERM, LIST_SHORT, LIST_LONG, LIST_BIG = [0, 1, 2, 3], [4, 5, 6, 7], [3, 2, 1, 0], [5, 4], list(range(9)), list(range(NBIG))
_ROUND = [LIST_A, LIST_A, LIST_B, LIST_A, LIST_PERM, LIST_SHORT, LIST_LONG, LIST_A, LIST_B]
LIST_ORDER = _ROUND[:7] + [LIST_BIG] + _ROUND[7:] + _ROUND + _ROUND + [LIST_A, LIST_B]
GROW_AT = 7
assert len(LIST_ORDER) == 30 and LIST_ORDER[GROW_AT] is LIST_BIG


def adpcm_audio(n, rng, kind):
    t = np.arange(n)
    x = (9000 * np.sin(2 * np.pi * 0.013 * t) + rng.normal(0, 300, n), rng.normal(0, 12000, n), np.where((t // 97) % 2 == 0, -32768, 32767),
         np.zeros(n), rng.integers(-3, 4, n))[kind % 5]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def test_cached_list_adpcm(oracle):
    """kg_adpcm's list_cache through miss, hit, miss, permuted, shorter, longer, grow, and on: 30 encode calls of 64 samples with
    the coder state carried on the device, every call's rows in its own region, the whole sequence with no wait but the growth's own.
    The queue is held behind the last call in front of the 1 100-channel list and behind the last call.  Bytes and final (index,
    previous) of every channel against the oracle carried per channel."""
    n = 64
    rng = np.random.default_rng(102)
    xs = [np.stack([adpcm_audio(n, rng, ch + k) for ch in chans]) for k, chans in enumerate(LIST_ORDER)]
    in_off = np.concatenate([[0], np.cumsum([x.size for x in xs])])
    out_off = in_off // 4 * 2                                                # n / 2 bytes per n samples
    flat = np.concatenate([x.reshape(-1) for x in xs])
    out = np.full(int(out_off[-1]), FILL, np.uint8)
    with fresh_ctx() as ctx:
        A = Adpcm(ctx, nchan=NBIG)
        d_in, d_out = ctx.alloc(flat.nbytes), ctx.alloc(out.nbytes)
        try:
            ctx.upload(d_in, flat)
            ctx.upload(d_out, out)
            for k, chans in enumerate(LIST_ORDER):
                if k == 1:
                    hold(ctx)                          # (call 0 made the cache's buffers, and drained to do so)
                if k == GROW_AT:
                    assert_deep(ctx, "the encode call in front of the list that grows the cache")
                A.encode_dev(chans, d_in + 2 * int(in_off[k]), n, n, d_out + int(out_off[k]), n // 2)
                if k == GROW_AT:
                    hold(ctx)
            assert_deep(ctx, "the last encode call")
            ctx.download(d_out, out)
            final = [A.get_state(ch) for ch in range(NBIG)]
        finally:
            ctx.free(d_in)
            ctx.free(d_out)
            A.close()
    st = [None] * NBIG
    for k, chans in enumerate(LIST_ORDER):
        got = out[int(out_off[k]):int(out_off[k + 1])].reshape(len(chans), n // 2)
        for r, ch in enumerate(chans):
            want, st[ch] = oracle.adpcm_encode_i16(xs[k][r], st[ch])
            assert np.array_equal(got[r], want), (k, ch)
    assert final == [(s.index, s.previous) for s in st]


POST_N = 256              # the block of tests/test_post_gpu.py's channel-list test, the smallest whole block the post tests batch
POST_PARAMS = [(True, False, -100, 50, 6, 1000, 12000.0), (True, True, -90, 50, 3, 500, 12000.0), (False, False, -100, 60, 6, 1000, 12000.0)]


def test_cached_list_post(oracle):
    """kg_post's list_cache through the same 30 lists (Post.process_dev, SSB; the channels beyond the first nine keep the
    constructor's AGC), with channel 2 changed to the IQ mode between calls 12 and 13: deep against stepwise, and the stepwise rows
    of the nine configured channels against the oracle's CAgc."""
    n = POST_N
    rng = np.random.default_rng(103)
    t = np.arange(40 * n)
    sig = (3000.0 * np.exp(2j * np.pi * 0.05 * t) + rng.normal(0, 20, t.size) + 1j * rng.normal(0, 20, t.size)).astype(np.complex64)
    mode_at = 13
    pos, xs = [0] * NBIG, []
    for chans in LIST_ORDER:
        xs.append(np.stack([sig[pos[ch] % (39 * n):pos[ch] % (39 * n) + n] * np.float32(1 + ch % 9) for ch in chans]))
        for ch in chans:
            pos[ch] += n
    R = Regions()
    offs = [(R.take(2 * x.shape[0] * n), R.take(4 * x.shape[0] * n), R.take(8 * x.shape[0] * n)) for x in xs]

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        P = st.P = Post(ctx, nchan=NBIG)
        st.objects.append(P)
        for ch in range(9):
            P.set_agc(ch, *POST_PARAMS[ch % 3])
            P.set_smeter(ch, 12000.0); P.set_mode(ch, post.MODE_SSB); P.reset(ch)
        st.d_x = [dev(st, x) for x in xs]
        st.getters = lambda: (P.smeter(LIST_LONG), [P.agc_delay(ch) for ch in range(9)])
        return st

    def call(k):
        o = offs[k]
        return lambda st: st.P.process_dev(LIST_ORDER[k], st.d_x[k], n, n, st.d_out + o[0], st.d_out + o[1], st.d_out + o[2], n)
    script = []
    for k in range(len(LIST_ORDER)):
        if k == mode_at:
            script.append(("set", lambda st: st.P.set_mode(2, post.MODE_IQ)))
        script.append(("set" if k in (0, GROW_AT) else "call", call(k)))      # the cache is made by call 0 and grows at GROW_AT: both drain
    step = deep_vs_stepwise(make, script)
    agcs = [oracle.Agc() for _ in range(9)]
    for ch in range(9):
        agcs[ch].set_parameters(*POST_PARAMS[ch % 3])
    for k, chans in enumerate(LIST_ORDER):
        s16 = region(step, offs[k][0], np.int16, (len(chans), n))
        agc = region(step, offs[k][2], np.complex64, (len(chans), n))
        for r, ch in enumerate(chans):
            if ch >= 9:
                continue
            if ch == 2 and k >= mode_at:
                assert same_bits(agc[r], np.asarray(agcs[ch].process_cpx(xs[k][r]), np.complex64)), (k, ch)
            else:
                assert np.array_equal(s16[r], agcs[ch].process_s16(xs[k][r])), (k, ch)


def wf_oracle_row(oracle, tables, iq, p, interp, window_func):
    windows, cic = tables
    m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped, False)
    sc = np.full(1024, p.fft_scale, np.float32)
    samps = oracle.wf_window_iq(iq, windows[window_func])
    return oracle.wf_compute_frame(samps, p.zoom, window_func, interp, True, False, p.fft_used, p.plot_width, p.plot_width_clamped, m, d, sc,
                                   (sc / np.float32(2)).astype(np.float32), p.fft_offset, cic)


WF_WAYS = 8               # WF_TABLE_WAYS of kg_wf.hip (tests/test_stream_order_coverage_cpu.py compares the two)


def test_waterfall_frame_tables(oracle):
    """kg_wf's WF_TABLE_WAYS-way cache of frame tables with its rotating victim, the frame kernels' claim counters and the blanker's
    d_nbf, two staged tables and nb_slot, all reused from launch to launch: WF_TABLE_WAYS + 2 distinct batches of 1 to 3 frames, round
    them twice (every table a miss: each is evicted before it comes round again), then one batch three times (hits), one
    kg_wf_frames_at_dev call and one kg_wf_nb_frames_dev call, channel 1 with its blanker on (its CNoiseProc state runs from frame to
    frame).  The first round fills the ways, each of which drains once to allocate itself; the 15 launches behind it run with no
    wait.  Deep against stepwise; the stepwise rows of the channels without a blanker against the oracle under
    tests/test_wf_gpu.py's rule."""
    from tests.test_wf_gpu import check_row, db_bound
    tables = (wf.window_functions(), wf.cic_comp_table())
    zooms = [0, 3, 7, 10]
    ps = [WfParams.for_zoom(z, 1.0e6 * ch) for ch, z in enumerate(zooms)]
    iqs = np.stack([synth.wf_iq_frame(seed=700 + i) for i in range(4)])
    batches = [[0], [1], [2, 3], [3, 2], [0, 1, 2], [2, 0, 3], [3, 3, 0], [2, 0], [1, 1], [0, 2, 3]]
    assert len(batches) == WF_WAYS + 2 and len(set(map(tuple, batches))) == len(batches) and all(1 <= len(b) <= 3 for b in batches)
    calls = [(b, None) for b in batches + batches + [batches[4]] * 3]
    offs_at = [2 * 8192 + 2, 0, 8192 + 4096]                    # frames read in place, not back to back
    calls.append(([2, 1, 0], offs_at))
    R = Regions()
    out_off = [R.take(1024 * len(b)) for b, _ in calls]
    nbf_off = R.take(2 * 8192 * 8)

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        w = st.w = Waterfall(ctx, nchan=4)
        st.objects.append(w)
        w.set_tables(*tables)
        for ch, p in enumerate(ps):
            w.set_channel(ch, p, interp=wf.WF_MAX, window_func=wf.WINF_HANNING, cic_comp=True)
        w.nb_setup(1, [100.0, 50.0])
        w.set_nb(1, True)
        st.d_iq = dev(st, iqs)
        st.d_warm = dev(st, np.zeros(2048, np.uint8))
        w.frames_dev([1, 1], st.d_iq, st.d_warm)               # d_nbf at the two blanked frames no later batch exceeds (growing it drains)
        ctx.sync()
        st.getters = lambda: w.nb_state([1])
        return st

    def call(k):
        b, fo = calls[k]
        if fo is None:
            return lambda st: st.w.frames_dev(b, st.d_iq, st.d_out + out_off[k])
        return lambda st: st.w.frames_dev(b, st.d_iq, st.d_out + out_off[k], frame_off=fo, iq_len=4 * 8192)
    # The first use of each of the cache's ways allocates it, and drains to do so: the first round is the warm-up of the ways ("set").
    # From then on nothing waits.  A batch with a blanked frame stages four tables, another one: a "deep" mark starts a new stretch
    # before a stretch has made 16 uploads (11, 8 and 15 here).
    script = [("set", call(k)) for k in range(len(batches))]
    for k in range(len(batches), len(calls)):
        script.append(("call", call(k)))
        if k in (len(batches) + 4, 2 * len(batches) - 1):
            script.append(("deep", "frames call %d" % k))
    script.append(("call", lambda st: st.w.nb_frames([1, 1], st.d_iq, st.d_out + nbf_off, [8192, 3 * 8192], 4 * 8192)))
    step = deep_vs_stepwise(make, script)
    want = {}
    flat = iqs.reshape(-1, 2)
    for k, (b, fo) in enumerate(calls):
        rows = region(step, out_off[k], np.uint8, (len(b), 1024))
        for f, ch in enumerate(b):
            if ch == 1:
                continue
            at = fo[f] if fo is not None else 8192 * f
            if (ch, at) not in want:
                want[(ch, at)] = wf_oracle_row(oracle, tables, flat[at:at + 8192], ps[ch], wf.WF_MAX, wf.WINF_HANNING)
            w_out, _, w_po, w_dB = want[(ch, at)]
            check_row(rows[f], w_out, w_dB, db_bound(w_po))
    assert not np.all(region(step, nbf_off, np.uint8, (2 * 8192 * 8,)) == FILL)


ACQ_L, ACQ_M = [0, 1], [1, 0]


def acq_run(ctx, s, d_bits, d_rows, d_pk, seq, deep):
    """seq: ACQ_L / ACQ_M (kg_acq_correlate_blocks_async with that list) or an int k (k two-row kg_wf_packets_dev calls: foreign uploads
    on the same ring) -> the results and cells of the last correlate"""
    if deep:
        hold(ctx)
    s.sample(d_bits)                                                        # kg_acq_sample_bits_dev
    if not deep:
        ctx.sync()
    u = 0
    for item in seq:
        if isinstance(item, int):
            for _ in range(item):
                wire.wf_packets_dev(ctx, d_rows, 1024, packet_infos(u), d_pk)
                u += 1
                if not deep:
                    ctx.sync()
        else:
            s.correlate_async(item)
            if not deep:
                ctx.sync()
    if deep:
        assert_deep(ctx, "the last correlate of %r" % (seq,))
    return s.fetch()


@pytest.mark.parametrize("seq", [[ACQ_L, k, ACQ_L] for k in (0, 14, 15, 16, 17)] + [[ACQ_L, ACQ_M, ACQ_L]],
                         ids=["k0", "k14", "k15", "k16", "k17", "LML"])
def test_acq_pair_table_reuse(oracle, seq):
    """kg_acq keeps its pair table in the ring slot it was staged in and reuses it while fewer than KG_RING_SLOTS / 2 uploads were
    made since (kg_acq_correlate_blocks_async): correlate(L), k foreign uploads on the same context, correlate(L), with k on both
    sides of 15 / 16, and L, M, L once -- one block, two C/A SVs, sampled through kg_acq_sample_bits_dev, all behind one plug.
    Results and cells equal the stepwise run bit for bit; for k = 0 also what tests/test_acq_gpu.py holds configs[0] to."""
    from tests.fixtures import oracle_row
    from tests.test_acq_gpu import SNR_RTOL, check_cells
    bits = synth.config0_bits()
    rows = np.random.default_rng(104).integers(0, 256, (2, 1024), dtype=np.uint8)
    runs = []
    for deep in (False, True):
        with fresh_ctx() as ctx:
            s = Searcher(ctx, max_sats=3)
            d_bits, d_rows, d_pk = ctx.alloc(bits.nbytes), ctx.alloc(rows.nbytes), ctx.alloc(2 * PKT)
            try:
                for sat in range(3):
                    _, t1, t2, _ = sats.SATS[sat]
                    s.set_code(sat, prn.cacode(t1, t2))
                ctx.upload(d_bits, bits)
                ctx.upload(d_rows, rows)
                runs.append(acq_run(ctx, s, d_bits, d_rows, d_pk, seq, deep))
                if seq[1] == 0 and not deep:
                    data = oracle.sample_bits(bits)
                    for i, sat in enumerate(ACQ_L):
                        want, wcells = oracle.correlate(oracle.code_fft(prn.cacode(*sats.SATS[sat][1:3])), data, code_next=oracle_row(oracle, s, sat + 1))
                        r = runs[0][0][0, i]
                        assert (int(r["dop"]), int(r["idx"]), int(r["valid"])) == (want["dop"], want["idx"], want["valid"])
                        assert abs(r["snr"] - want["snr"]) <= SNR_RTOL * want["snr"]
                        check_cells(runs[0][1][0, i], wcells, "stream order, sat %d" % sat)
                    assert (int(runs[0][0][0, 0]["dop"]), int(runs[0][0][0, 0]["idx"])) == (6, 1202)
            finally:
                for d in (d_bits, d_rows, d_pk):
                    ctx.free(d)
                s.close()
    (res_s, cells_s), (res_d, cells_d) = runs
    assert same_bits(res_s, res_d) and same_bits(cells_s, cells_d)


def test_acq_samplers(oracle):
    """kg_acq_sample_iq16_dev and kg_acq_sample_iq16_batch_dev in front of the correlator, all enqueued behind one plug: block 0 alone,
    then blocks 0 and 1 as a batch (block 0 sampled twice: the second front end must wait for nothing it should not), two
    correlations.  Equal to the stepwise run bit for bit; the time-domain samples of block 1 equal the oracle's."""
    iq = np.stack([synth.config1_iq16().reshape(-1), np.roll(synth.config1_iq16().reshape(-1), 2 * 777)])
    runs = []
    for deep in (False, True):
        with fresh_ctx() as ctx:
            s = Searcher(ctx, max_sats=3, max_blocks=2)
            d_iq = ctx.alloc(iq.nbytes)
            try:
                for sat in range(3):
                    s.set_code(sat, prn.cacode(*sats.SATS[sat][1:3]))
                ctx.upload(d_iq, iq)
                if deep:
                    hold(ctx)
                for step in (lambda: s.sample_iq16(d_iq + iq[0].nbytes, block=0), lambda: s.correlate_async(ACQ_L, 1),
                             lambda: s.sample_iq16_batch(d_iq, 2), lambda: s.correlate_async(ACQ_M, 2)):
                    step()
                    if not deep:
                        ctx.sync()
                if deep:
                    assert_deep(ctx, "the correlate behind the batch sampler")
                runs.append(s.fetch() + (s.get_data_td(1),))
            finally:
                ctx.free(d_iq)
                s.close()
    assert same_bits(runs[0], runs[1])
    _, td = oracle.sample_iq16(iq[1], want_td=True)
    assert np.array_equal(runs[0][2].view(np.uint32), td.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every stateful module, deep against stepwise
# ---------------------------------------------------------------------------------------------------------------------------------

def cpx(kind, n, seed):
    return nb_signals.audio(kind, n, seed).view(np.complex64).reshape(-1)


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_fir(oracle):
    """kg_fir: process_dev in the data pump's 170-sample pieces and in 512s, a changing channel list, SetupParameters and a reset between
    calls, then the spectrum-row, per-entry, tapped and refilter entry points and kg_snd_spec_rows_dev -- the refilter and the row call
    READ what the tapped call wrote, in stream order.  nout and FirPos() are host mirrors returned at once.  Channel 0, never set up
    again, is held to the oracle's CFastFIR under tests/test_snd_gpu.py's bound."""
    N, OS = 4096, 1024
    x = np.stack([cpx(k, N, 40 + i) for i, k in enumerate(("noise_pulses", "carrier_pulses", "quiet_then_loud", "noise_pulses"))])
    R = Regions()
    script, feeds = [], []                                   # feeds: what channel 0 was given and where its outputs went

    def pos_of(st):
        return [st.f.pos(c) for c in range(4)]

    def proc(chans, row0, pos, n):
        o = R.take(8 * OS * len(chans))
        script.append(("call", lambda st: (st.f.process_dev(chans, st.d_x + 8 * (row0 * N + pos), N, n, st.d_out + o, OS), pos_of(st))))
        if 0 in chans:
            feeds.append((x[row0 + chans.index(0), pos:pos + n], o + 8 * OS * chans.index(0)))

    proc([0, 1, 2], 0, 0, 170)
    proc([0, 1, 2], 0, 170, 170)
    proc([2, 1, 0, 3], 0, 340, 170)
    proc([0, 1, 2, 3], 0, 510, 512)
    script.append(("set", lambda st: st.f.setup(1, -2700.0, -300.0, 0.0, 12000.0)))
    proc([1, 3], 1, 1022, 170)
    o_so, o_rows, o_post = R.take(8 * OS * 3), R.take(2048 * 3), R.take(8 * 2048 * 3)
    script.append(("call", lambda st: (st.f.process_spec_dev([0, 1, 2], st.d_x + 8 * 1192, N, [170, 512, 7], st.d_out + o_so, OS, st.d_out + o_rows,
                                                             2048, [snd.SPEC_PASSBAND, snd.SPEC_CHAN_NULL, snd.SPEC_PASSBAND], st.d_out + o_post, 2048),
                                       pos_of(st))))
    feeds.append((x[0, 1192:1192 + 170], o_so))
    script.append(("call", lambda st: st.f.reset(2)))        # (in stream order: a memset on the stream and the host mirror)
    proc([0, 2], 0, 1704, 512)
    o_to, o_pre, o_tpost, o_re, o_each, o_srow = R.take(8 * OS), R.take(8 * 2048), R.take(8 * 2048), R.take(8 * OS), R.take(8 * OS * 2), R.take(1024)

    def taps(st):
        ch, nout = np.array([3], np.int32), np.zeros(1, np.int32)
        check(st.f.lib.kg_fir_process_taps_dev(st.f.h, ptr(ch), 1, ptr(st.d_x + 8 * (3 * N + 2216)), N, 512, ptr(st.d_out + o_to), OS, ptr(nout),
                                               ptr(st.d_out + o_pre), ptr(st.d_out + o_tpost), 2048), "kg_fir_process_taps_dev")
        return nout, pos_of(st)

    def refilter(st):
        ch, nblk = np.array([3], np.int32), np.array([1], np.int32)
        check(st.f.lib.kg_fir_refilter_dev(st.f.h, ptr(ch), 1, ptr(nblk), ptr(st.d_out + o_pre), 2048, ptr(st.d_out + o_re), OS), "kg_fir_refilter_dev")

    def each(st):
        ch, n_each, nout = np.array([0, 1], np.int32), np.array([170, 340], np.int32), np.zeros(2, np.int32)
        check(st.f.lib.kg_fir_process_each_dev(st.f.h, ptr(ch), 2, ptr(st.d_x + 8 * 2728), N, ptr(n_each), ptr(st.d_out + o_each), OS, ptr(nout)),
              "kg_fir_process_each_dev")
        return nout, pos_of(st)
    script += [("call", taps), ("call", refilter), ("call", each),
               ("call", lambda st: snd.spec_rows_dev(st.ctx, st.d_out + o_tpost, 1024, [snd.SPEC_PASSBAND], st.d_out + o_srow))]
    feeds.append((x[0, 2728:2728 + 170], o_each))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        f = st.f = FastFir(ctx, nchan=4, max_in=1024)
        st.objects.append(f)
        for ch in range(4):
            f.setup(ch, 100.0 + 50 * ch, 2500.0 + 50 * ch, 0.0, 12000.0)
        st.d_x = dev(st, x)
        st.getters = lambda: (pos_of(st), f.get_coef(1))
        return st
    step = deep_vs_stepwise(make, script)
    assert [int(r[0][0]) for r in step.rets[:4]] == [0, 0, 0, 512] and step.rets[3][1][0] == 170 * 3 + 512 - 512      # the pump's rhythm
    _, coef_cic, _ = oracle.fir_design(100.0, 2500.0, 0.0, 12000.0)
    ost, nchecked = oracle.fir_new_state(), 0
    for seg, o in feeds:
        want, _ = oracle.fir_process(ost, coef_cic, seg)
        if want.size:
            assert relmax(region(step, o, np.complex64, (want.size,)), want) < 1e-5
            nchecked += 1
    assert nchecked >= 2
    assert not np.all(region(step, o_re, np.uint8, (8 * 512,)) == FILL) and not np.all(region(step, o_srow, np.uint8, (1024,)) == FILL)


def test_unpack_and_payloads(oracle):
    """The context-level entry points of the audio path, each with a table of its own per call on the ring: kg_dpump_unpack_rows_dev
    (the enable mask), kg_snd_iq_payload_dev (the channel list), kg_snd_payload_dev (no table), ragged sample counts, masks and lists
    changing from call to call, each call READING what an earlier one wrote.  The unpacked samples and the IQ payload bytes of the
    stepwise run equal the oracle's."""
    rng = np.random.default_rng(105)
    nch, stride = 5, 200
    i24, q24 = rng.integers(-2 ** 23, 2 ** 23, (stride, nch)), rng.integers(-2 ** 23, 2 ** 23, (stride, nch))
    spi = snd.pack_rx_iq(i24, q24)
    raw = np.ascontiguousarray(spi.reshape(stride, nch, 6).transpose(1, 0, 2))                  # one row of records per channel
    s16 = rng.integers(-32768, 32768, (nch, stride)).astype(np.int16)
    R = Regions()
    unp = [(173, [1, 1, 0, 1, 1], 1.5, -2.0, False), (64, [1, 0, 1, 0, 1], 0.0, 0.0, True), (200, [1, 1, 1, 1, 1], -3.0, 0.5, False)]
    o_unp = [R.take(8 * stride * nch) for _ in unp]
    iqp = [(0, [0, 1, 2, 3, 4], 173, True), (1, [4, 2, 0], 64, False), (2, [3, 1], 199, True), (0, [1], 7, False)]      # (source call, list, n, LE)
    o_iqp = [R.take(4 * stride * len(lst)) for _, lst, _, _ in iqp]
    pay = [(nch, 200, True), (3, 77, False)]
    o_pay = [R.take(2 * stride * n) for n, _, _ in pay]
    script = []
    for (n, en, di, dq, inv), o in zip(unp, o_unp):
        script.append(("call", lambda st, n=n, en=en, di=di, dq=dq, inv=inv, o=o: snd.unpack_rows_dev(
            st.ctx, st.d_raw, stride, n, nch, st.d_out + o, stride, enabled=np.array(en, np.uint8), dc_i=di, dc_q=dq, spectral_inversion=inv)))
    for (src, lst, n, le), o in zip(iqp, o_iqp):
        def iq_payload(st, src=src, lst=lst, n=n, le=le, o=o):
            c = np.array(lst, np.int32)
            check(st.ctx.lib.kg_snd_iq_payload_dev(st.ctx.h, ptr(c), c.size, C.c_void_p(st.d_out + o_unp[src]), stride, n, int(le),
                                                   C.c_void_p(st.d_out + o), 4 * stride), "kg_snd_iq_payload_dev")
        script.append(("call", iq_payload))
    for (n, ns, le), o in zip(pay, o_pay):
        script.append(("call", lambda st, n=n, ns=ns, le=le, o=o: check(st.ctx.lib.kg_snd_payload_dev(
            st.ctx.h, C.c_void_p(st.d_s16), stride, n, ns, int(le), C.c_void_p(st.d_out + o), 2 * stride), "kg_snd_payload_dev")))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.d_raw, st.d_s16 = dev(st, raw), dev(st, s16)
        return st
    step = deep_vs_stepwise(make, script)
    got = []
    for (n, en, di, dq, inv), o in zip(unp, o_unp):
        out = region(step, o, np.complex64, (nch, stride))
        want = oracle.dpump_unpack(spi[:n * nch * 6], n, nch, enabled=np.array(en, np.uint8), dc_i=di, dc_q=dq, spectral_inversion=inv)
        on = np.array(en, bool)                                # (a disabled channel's row is compared between the two runs only)
        assert np.array_equal(out[on, :n].view(np.uint32), want[on].view(np.uint32))
        got.append(out)
    for (src, lst, n, le), o in zip(iqp, o_iqp):
        bytes_ = region(step, o, np.uint8, (len(lst), 4 * stride))
        for r in range(len(lst)):                              # (not a bank's context: row r of the input is entry r's)
            assert np.array_equal(bytes_[r, :4 * n], oracle.snd_iq_payload(got[src][r, :n], le)), (src, lst, r)
            assert np.all(bytes_[r, 4 * n:] == FILL)
    for (n, ns, le), o in zip(pay, o_pay):
        b = region(step, o, np.uint8, (n, 2 * stride))
        want = (s16[:n, :ns] if le else s16[:n, :ns].byteswap()).copy().view(np.uint8).reshape(n, -1)
        assert np.array_equal(b[:, :2 * ns], want)


def test_noise_blanker():
    """kg_nb: four of the golden audio scenarios (tests/golden/nb_ref.npz) side by side, block r of each in one kg_nb_process_dev call
    -- ragged counts, zero counts, the list shrinking as scenarios end -- with SetupBlanker of a fifth channel between two calls.
    Deep against stepwise; the stepwise blocks and end states against the reference's."""
    from tests.test_nb_gpu import AUDIO, audio_input, check_audio, script as nb_script, setup_args
    names = [n for n in AUDIO if sum(l[0] == "U" for l in nb_script(n)) == 1 and nb_script(n)[-1] == "S"][:4]
    assert len(names) == 4
    chans = [1, 3, 5, 7]
    xs = [audio_input(n) for n in names]
    blocks = [[int(l.split()[1]) for l in nb_script(n) if l[0] == "B"] for n in names]
    rounds = max(len(b) for b in blocks)
    stride = max(max(b) for b in blocks)
    R = Regions()
    script, where, bufs, pos = [], [[] for _ in names], [], [0] * 4
    for r in range(rounds):
        live = [i for i in range(4) if r < len(blocks[i])]
        cnt = [blocks[i][r] for i in live]
        buf = np.zeros((len(live), stride, 2), np.float32)
        for k, i in enumerate(live):
            buf[k, :cnt[k]] = xs[i][pos[i]:pos[i] + cnt[k]]
            pos[i] += cnt[k]
        o = R.take(8 * stride * len(live))
        for k, i in enumerate(live):
            where[i].append((o + 8 * stride * k, cnt[k]))
        bufs.append(buf)
        if r == 2:
            script.append(("set", lambda st: st.nb.setup(0, 12000.0, [100.0, 50.0])))
        if r and r % 8 == 0:
            script.append(("deep", "blanker round %d" % r))
        script.append(("call", lambda st, r=r, live=live, cnt=cnt, o=o: st.nb.process_dev([chans[i] for i in live], st.d_in[r], stride, cnt, st.d_out + o, stride)))
    assert rounds >= 6

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.nb = NoiseBlanker(ctx, nchan=8, max_in=stride)
        st.objects.append(st.nb)
        for i, n in enumerate(names):
            rate, prm = setup_args(nb_script(n)[0])
            st.nb.setup(chans[i], rate, prm)
        st.d_in = [dev(st, b) for b in bufs]
        st.getters = lambda: st.nb.state(chans + [0])
        return st
    step = deep_vs_stepwise(make, script)
    ints, flts = step.state
    for i, n in enumerate(names):
        outs = [region(step, o, np.float32, (c, 2)).copy() for o, c in where[i]]
        check_audio(n, outs, [(ints[i:i + 1], flts[i:i + 1])])


def test_aperture(oracle):
    """kg_aper: nine kg_aper_update_dev calls with the row list, the algorithms and the clear flags changing from call to call, the band
    report (which drains) in mid-run.  Deep against stepwise; every average of the stepwise run equals the oracle's aperture_auto()."""
    from tests.test_handoff_gpu import rows_for
    rng = np.random.default_rng(106)
    nchan, algos = 6, [handoff.MMA, handoff.EMA, handoff.IIR]
    lists = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [5, 3, 1], [0, 2, 4], [4, 5], [0, 1, 2, 3, 4, 5], [2], [1, 0, 3], [5, 4, 3, 2, 1, 0]]
    rows = [np.stack([rows_for(rng, ch + it) for ch in lst]) for it, lst in enumerate(lists)]
    cfgs = [[(algos[ch % 3], [8.0, 4.0, 2.5][ch % 3], it == 0 or (it == 5 and ch == 3), ch >= 4) for ch in lst] for it, lst in enumerate(lists)]
    script = []
    for it, lst in enumerate(lists):
        if it == 4:
            script.append(("set", lambda st: st.A.report(list(range(nchan)), [ch >= 4 for ch in range(nchan)])))
        script.append(("call", lambda st, it=it, lst=lst: st.A.update_dev(lst, st.d_rows[it], 1024, cfgs[it], -13)))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=256)
        st.A = Aperture(ctx, nchan=nchan)
        st.objects.append(st.A)
        st.d_rows = [dev(st, r) for r in rows]
        st.getters = lambda: ([st.A.get(ch) for ch in range(nchan)], st.A.report(list(range(nchan)), [ch >= 4 for ch in range(nchan)]))
        return st
    step = deep_vs_stepwise(make, script)
    want = [np.zeros(1024, np.float32) for _ in range(nchan)]
    for it, lst in enumerate(lists):
        for r, ch in enumerate(lst):
            a, p, clr, af = cfgs[it][r]
            want[ch] = oracle.aper_update(want[ch], rows[it][r], a, p, clr, 256 if af else 0, 768 if af else 1024, -13)
    for ch in range(nchan):
        assert np.array_equal(step.state[0][ch].view(np.uint32), want[ch].view(np.uint32)), ch
        assert (int(step.state[1][0][ch]), int(step.state[1][1][ch])) == oracle.aper_report(step.state[0][ch], 256 if ch >= 4 else 0, 768 if ch >= 4 else 1024)


def adc_stream(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    x = rng.normal(0, 40.0, n) + 9000.0 * np.cos(2 * np.pi * 0.0123 * t + 1.0) + 700.0 * np.cos(2 * np.pi * 0.201 * t + 2.0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def ddc_inc(f):
    return (-int(round(f * 2 ** 48))) & ((1 << 48) - 1)


def test_wf_ddc_inline(oracle):
    """kg_ddc in the in-line mode (not deferred), kg_ddc_wf_push_dev with a different per-call table every time: the object allocates
    its comb inputs at the first push of each of its two buffer sets, and it rebuilds a table when the block length changes -- both
    drain by design, as does everything around a capture -- so the deep stretches are pushes of one length (a multiple of every
    decimation), each with another channel list, behind the content-cached pack: hit, miss, permuted, shorter, first again.  The
    ragged pushes, a reset, a phase command, kg_ddc_wf_capture_dev and kg_ddc_wf_step_dev stand between the stretches.  Deep against
    stepwise; channel 0, in every call until the capture, against the oracle over the whole stream."""
    n, l2 = 16384, [3, 0, 7, 5]
    sizes = [n, n, n, n, n, n, 63, 4097, n, n, n, n]
    lists = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0], [0, 2], [0, 1, 2, 3], [0, 1, 2, 3], [0, 3], [0, 1, 2, 3], [1, 0], [0, 1, 2, 3], [2, 0, 3]]
    drains = {0, 1, 6, 7, 8}                                 # first use of a buffer set; a new block length
    adc = adc_stream(sum(sizes) + 3 * n, seed=107)
    incs = [ddc_inc(0.0123 + 2.0 ** -22), ddc_inc(0.05), ddc_inc(0.2007), ddc_inc(0.031)]
    stride = n + 16
    R = Regions()
    offs = [R.take(4 * stride * len(lst)) for lst in lists]
    o_cap, o_step = R.take(4 * stride * 2), R.take(4 * stride * 4)
    at = np.concatenate([[0], np.cumsum(sizes)])
    script = []
    for k, (sz, lst) in enumerate(zip(sizes, lists)):
        if k == 10:
            script.append(("set", lambda st: st.d.reset(2)))
        script.append(("set" if k in drains else "call",
                       lambda st, k=k, sz=sz, lst=lst: st.d.push_dev(st.d_adc + 2 * int(at[k]), sz, lst, st.d_out + offs[k], stride)))
    end = int(at[-1])
    script.append(("set", lambda st: st.d.set_phase(1, 0x123456789A)))
    script.append(("set", lambda st: st.d.capture_dev(st.d_adc + 2 * end, n, [1, 2], st.d_out + o_cap, stride, 300)))

    def step_call(st):
        chans, nouts = np.arange(4, dtype=np.int32), np.zeros(4, np.int64)
        off, mo = np.array([0, 6, 2, 14], np.int64), np.array([0, 100, 0, 0], np.int64)
        check(st.d.lib.kg_ddc_wf_step_dev(st.d.h, ptr(st.d_adc + 2 * (end + n)), n, ptr(chans), 4, ptr(st.d_out + o_step), stride, ptr(off), ptr(mo),
                                          ptr(nouts)), "kg_ddc_wf_step_dev")
        return nouts
    script.append(("set", step_call))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.d = Ddc(ctx, nchan=4, max_samples=n)
        st.objects.append(st.d)
        for ch in range(4):
            st.d.set_wf(ch, incs[ch], 1 << l2[ch])
        st.d_adc = dev(st, adc)
        st.getters = lambda: [st.d.outputs(ch, 1000) for ch in range(4)]
        return st
    step = deep_vs_stepwise(make, script)
    want, _ = oracle.ddc_wf(adc[:end], incs[0], l2[0])
    parts = []
    for k, lst in enumerate(lists):
        nout = int(step.rets[k + (1 if k >= 10 else 0)][lst.index(0)])
        parts.append(region(step, offs[k] + 4 * stride * lst.index(0), np.int16, (stride, 2))[:nout])
    got = np.concatenate(parts)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_rx_ddc(oracle):
    """kg_rxddc: ragged pushes (1, 1735, 1736, 5209 ... samples), a different channel list per call behind the content-cached pack, a
    retune and a reset between calls.  Deep against stepwise; channel 0, in every call, against the oracle with its state carried."""
    sizes = [1, 1735, 1736, 5209, 10416, 64, 20001, 77, 31248]
    lists = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [0, 2], [0, 1, 2], [1, 0], [0, 1, 2], [0], [2, 0, 1]]
    adc = adc_stream(sum(sizes), seed=108)
    inc = [(-rx_phase_inc(0.0123 * 125e6 - 600 + 900 * k)) & ((1 << 48) - 1) for k in range(4)]
    stride = 8
    R = Regions()
    offs = [R.take(6 * stride * len(lst)) for lst in lists]
    at = np.concatenate([[0], np.cumsum(sizes)])
    script = []
    for k, (sz, lst) in enumerate(zip(sizes, lists)):
        if k == 5:
            script.append(("set", lambda st: st.d.set_freq(0, inc[3])))
        if k == 7:
            script.append(("set", lambda st: st.d.reset(1)))
        script.append(("set" if k == 0 else "call",         # (the pack's cache is made by the first push, which drains to do so)
                       lambda st, k=k, sz=sz, lst=lst: (st.d.push_dev(st.d_adc + 2 * int(at[k]), sz, lst, st.d_out + offs[k], stride),
                                                        [st.d.outputs(ch, 5000) for ch in range(3)])))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.d = RxDdc(ctx, nchan=3, max_samples=max(sizes))
        st.objects.append(st.d)
        for ch in range(3):
            st.d.set_freq(ch, inc[ch])
        st.d_adc = dev(st, adc)
        st.getters = lambda: [st.d.outputs(ch, 12345) for ch in range(3)]
        return st
    step = deep_vs_stepwise(make, script)
    ost, calls = None, [r for r in step.rets if r is not None and isinstance(r, list) and len(r) == 2]
    assert len(calls) == len(sizes)
    for k, (sz, lst) in enumerate(zip(sizes, lists)):
        w, ost = oracle.ddc_rx(adc[int(at[k]):int(at[k + 1])], inc[3] if k >= 5 else inc[0], ost)
        nout = int(calls[k][0][lst.index(0)])
        got = region(step, offs[k] + 6 * stride * lst.index(0), np.uint8, (6 * stride,))[:6 * nout]
        assert np.array_equal(got, w), k


# ---- kg_post's block filters on a golden scenario each: the scenario on channel 2 (row 0), a companion on channel 0 (row 1) listed in
# every other call, so that the cached channel list changes from call to call
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POST_CH, POST_COMP = 2, 0


def post_filter_script(kind, lines, n_total):
    """The script of a golden scenario (tests/golden/nr_ref.npz, nrs_ref.npz, nbw_ref.npz; the command state of the connection is kept
    here as tests/nrs_common.py and tests/nbw_common.py keep it) as deep_vs_stepwise actions: every command a "set", every getter a
    "set", the blocks that run the stage as calls -- of one block for nr, of one to three for the two 512-sample stages.
    -> (script, ran: bool per sample, the script indices of the S lines)"""
    N, ch = n_total, POST_CH
    script, ran, s_at = [], np.zeros(N, bool), []
    algo, en, on, param, pos, ncall = 0, [0] * 4, 0, np.zeros((4, 8), np.float32), 0, 0
    pend = []                                               # running blocks waiting to be merged into one call
    since_mark = 0

    def flush():
        nonlocal ncall, since_mark
        if not pend:
            return
        p0, n = pend[0], 512 * len(pend)
        chans = [ch, POST_COMP] if ncall % 2 == 0 else [ch]
        fn = {"nrs": lambda st: st.P.nrs_process_dev(chans, st.d_x + 2 * p0, N, n, st.d_out + 2 * p0, N),
              "nbw": lambda st: st.P.nbw_process_dev(chans, st.d_x + 2 * p0, N, n, st.d_out + 2 * p0, N)}[kind]
        if since_mark == 8:
            script.append(("deep", "%s call %d" % (kind, ncall)))
            since_mark = 0
        script.append(("set" if ncall == 0 else "call", fn))     # (the list cache is made by the first call, which drains)
        ran[p0:p0 + n] = True
        ncall += 1
        since_mark += 1
        pend.clear()

    def command(fn):
        nonlocal since_mark
        flush()
        script.append(("set", fn))
        since_mark = 0
    for line in lines:
        f = line.split()
        if f[0] == "B":
            n, passthrough = int(f[1]), int(f[2])
            if kind == "nr":
                stages = [t for t in (post.NR_AUTONOTCH, post.NR_DENOISE) if en[t]] if (not passthrough and algo in (post.NR_WDSP, post.NR_ORIG)) else []
                for j, t in enumerate(stages):
                    chans = [ch, POST_COMP] if ncall % 2 == 0 else [ch]
                    script.append(("set" if ncall == 0 else "call", lambda st, t=t, j=j, p0=pos, n=n, chans=chans: st.P.nr_process_dev(
                        chans, t, (st.d_out if j else st.d_x) + 2 * p0, N, n, st.d_out + 2 * p0, N)))
                    ncall += 1
                ran[pos:pos + n] = bool(stages)
            else:
                runs = (not passthrough) and (algo == post.NR_SPECTRAL if kind == "nrs" else bool(on))
                if runs:
                    pend.append(pos)
                    if len(pend) == 1 + ncall % 3:
                        flush()
                else:
                    flush()
            pos += n
        elif f[0] == "S":
            flush()
            s_at.append(len(script))
            script.append(("set", {"nr": lambda st: [st.P.nr_state([ch], t, weights=True) for t in range(2)],
                                   "nrs": lambda st: st.P.nrs_state([ch]), "nbw": lambda st: st.P.nbw_state([ch])}[kind]))
        elif f[0] == "A":
            a = int(f[1])
            if kind == "nbw":
                algo, en, on = a, [0] * 4, 0
                command(lambda st: st.P.set_nbw(ch, 0))
            else:
                algo = a
                if kind == "nr":
                    en = [0] * 4
                command((lambda st: st.P.nrs_select(ch)) if (kind == "nrs" and a == post.NR_SPECTRAL) else (lambda st, a=a: st.P.set_nr_algo(ch, a)))
        elif f[0] == "E":
            t, e = int(f[1]), int(f[2])
            if kind == "nbw":
                if t == 0 and algo == 2:
                    on = int(bool(e))
                    command(lambda st, e=e: st.P.set_nbw(ch, e))
            else:
                command(lambda st, t=t, e=e: st.P.set_nr_enable(ch, t, e))
            en[t] = e
        elif f[0] == "P":
            t, p = int(f[1]), int(f[2])
            if kind == "nbw":
                v = param[t].copy()
                v[p] = np.float32(f[3])
                if t == 0 and algo == 2:
                    command(lambda st, v=v: st.P.nbw_init(ch, v))
                param[t] = v
            else:
                command(lambda st, t=t, p=p, v=np.float32(f[3]): st.P.set_nr_param(ch, t, p, v))
        elif f[0] == "M":
            command(lambda st, lo=float(f[1]), hi=float(f[2]): st.P.nrs_passband(ch, lo, hi))
        elif f[0] == "C":
            algo, en, on = 0, [0] * 4, 0
            param[:] = 0
            command(lambda st: st.P.reset(ch))
        else:
            raise AssertionError(line)
    flush()
    assert pos == N
    return script, ran, s_at


def post_filter_run(kind, x, lines):
    N = x.size
    xin = np.stack([x, np.roll(x, 97)])
    script, ran, s_at = post_filter_script(kind, lines, N)

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=4 * N)
        P = st.P = Post(ctx, nchan=3)
        st.objects.append(P)
        if kind == "nr":
            P.set_nr_algo(POST_COMP, post.NR_WDSP)
            for t in (0, 1):
                for k, v in enumerate([64, 16, 1e-4, 0.1]):
                    P.set_nr_param(POST_COMP, t, k, v)
                P.set_nr_enable(POST_COMP, t, 1)
        elif kind == "nrs":
            P.nrs_passband(POST_COMP, 300.0, 2700.0)
            P.nrs_select(POST_COMP)
            for k, v in enumerate([1, 0.95, 1000]):
                P.set_nr_param(POST_COMP, 0, k, v)
        else:
            P.nbw_init(POST_COMP, [3, 10, 7])
            P.set_nbw(POST_COMP, 1)
        st.d_x = dev(st, xin)
        st.getters = lambda: {"nr": lambda: P.nr_state([POST_CH, POST_COMP], 0, weights=True), "nrs": lambda: P.nrs_state([POST_CH, POST_COMP]),
                              "nbw": lambda: P.nbw_state([POST_CH, POST_COMP])}[kind]()
        return st
    step = deep_vs_stepwise(make, script)
    y = region(step, 0, np.int16, (2, N))[0]
    assert ran.sum() >= 6 * 512 and np.all(y[~ran].view(np.uint8) == FILL)
    return np.where(ran, y, x), [step.rets[i] for i in s_at]


def test_post_nr():
    """kg_post_nr_process_dev on the golden scenario that switches the algorithm in mid-stream (tests/golden/nr_ref.npz): every block and
    the end state of the stepwise run equal the reference's, and the deep run equals the stepwise one"""
    from tests.test_nr_gpu import digest
    g, name = np.load(os.path.join(GOLDEN, "nr_ref.npz")), "algo_switch_keeps_state"
    y, states = post_filter_run("nr", g[name + "_in"], [str(l) for l in g[name + "_script"]])
    assert np.array_equal(y, g[name + "_out"])
    for t, st in enumerate(states[-1]):
        si, sf = g[name + "_state_i"][t], g[name + "_state_f"][t]
        assert list(st["anr_i"][0]) == list(si[:3]) and list(st["lms_i"][0]) == list(si[3:6]), (name, t)
        assert np.array_equal(st["anr_f"][0].view(np.uint32), sf.view(np.uint32)), (name, t)
        assert digest(st["anr_w"][0]) == bytes(g[name + "_w_sha"][t]) and digest(st["lms_coef"][0]) == bytes(g[name + "_coef_sha"][t]), (name, t)


def test_post_nrs():
    """kg_post_nrs_process_dev on the golden scenario with a new connection in mid-stream (tests/golden/nrs_ref.npz), in calls of one to
    three blocks"""
    g, name = nrs_common.load(), "new_connection"
    y, states = post_filter_run("nrs", nrs_common.scenario_input(g, name), nrs_common.script(g, name))
    nrs_common.check_blocks(name, y, g, "stream order")
    nrs_common.check_states(name, states, g, "stream order")


def test_post_nbw():
    """kg_post_nbw_process_dev on the golden scenario that switches the stage off and on (tests/golden/nbw_ref.npz), in calls of one to
    three blocks"""
    g, name = nbw_common.load(), "enable_off_on"
    y, states = post_filter_run("nbw", nbw_common.scenario_input(g, name, nbw_common.pool()), nbw_common.script(g, name))
    nbw_common.check_blocks(name, y, g, "stream order")
    nbw_common.check_states(name, states, g, "stream order")


def test_post_cfir_and_squelch():
    """kg_post_cfir_process_dev (the three ProcessFilter overloads) and kg_post_squelch_perform_dev behind kg_post's cached list: ragged
    lengths, a list that changes, SetSquelch between two calls.  Deep against stepwise."""
    rng = np.random.default_rng(109)
    S = 1024
    xf = (rng.normal(0, 3000, (3, S))).astype(np.float32)
    xi = np.clip(xf, -32768, 32767).astype(np.int16)
    R = Regions()
    script = []

    def cfir(chans, kind_, n, first=False):
        o = R.take(4 * S * len(chans))
        src = "d_xi" if kind_ == post.CFIR_MONO16_MONO16 else "d_xf"

        def fn(st):
            c = np.array(chans, np.int32)
            check(st.P.lib.kg_post_cfir_process_dev(st.P.h, ptr(c), c.size, post.CFIR_AM, kind_, ptr(getattr(st, src)), S, n, ptr(st.d_out + o), S),
                  "kg_post_cfir_process_dev")
        script.append(("set" if first else "call", fn))

    def squelch(chans, n):
        o = R.take(2 * S * len(chans))

        def fn(st):
            c = np.array(chans, np.int32)
            check(st.P.lib.kg_post_squelch_perform_dev(st.P.h, ptr(c), c.size, ptr(st.d_xf), S, n, ptr(st.d_out + o), S), "kg_post_squelch_perform_dev")
        script.append(("call", fn))
    cfir([0, 1, 2], post.CFIR_REAL_REAL, 171, first=True)
    cfir([0, 1, 2], post.CFIR_REAL_MONO16, 512)
    cfir([2, 0], post.CFIR_MONO16_MONO16, 63)
    squelch([0, 1, 2], 512)
    script.append(("set", lambda st: st.P.squelch_set(1, 99, 0)))
    squelch([1, 0], 256)
    cfir([1], post.CFIR_REAL_REAL, 1000)
    squelch([2], 1024)

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        P = st.P = Post(ctx, nchan=3)
        st.objects.append(P)
        for ch in range(3):
            P.set_am_passband(ch, -2700.0, 2700.0, 12000.0)
            P.squelch_setup(ch, 12000.0)
            P.squelch_set(ch, 80 if ch else 0, 0)
        st.d_xf, st.d_xi = dev(st, xf), dev(st, xi)
        st.getters = lambda: (P.squelch_state([0, 1, 2]), P.cfir_taps(0, post.CFIR_AM))
        return st
    step = deep_vs_stepwise(make, script)
    assert not np.all(step.out == FILL)


def test_tracker(tmp_path):
    """kg_trk: the `pieces` scenario of tests/trk_common.py -- a C/A and an E1B channel, one stream in calls of 8, 99, 200, 1, 7 and then
    1, 7, 8191 and 100001 clocks in turn, GPS_CHAN dumps between the first ones.  A dump and the first call behind it drain by design (the
    host's copy of the channels is fetched and written back); the long run of calls behind the last dump is deep.  Deep against
    stepwise; the stepwise records and dumps against the literal clock-by-clock model."""
    sc = tc.scenarios()["pieces"]
    want = tc.run_tool(tc.build(tmp_path, "trk_model"), sc, tmp_path)
    R = Regions()
    script, xs, ds, clock, fresh = [], [], [], 0, True
    setup = []
    for s in sc.steps:
        op = s[0]
        if op == "X":
            n = s[1]
            cap = trk.cap_for(n)
            o_ep, o_cnt = R.take(48 * cap * sc.nchan), R.take(4 * sc.nchan)
            xs.append((o_ep, o_cnt, cap))
            script.append(("set" if fresh else "call", lambda st, n=n, cap=cap, c=clock, o_ep=o_ep, o_cnt=o_cnt: st.t.process_dev(
                st.d_bits + c // 8, n, st.d_out + o_ep, cap, cap, st.d_out + o_cnt)))
            clock += n
            fresh = False
        elif op == "D":
            ds.append(len(script))
            script.append(("set", lambda st: (st.t.get_clocks(), [st.t.get_chan(ch).tobytes().hex() for ch in range(sc.nchan)])))
            fresh = True
        else:
            assert not script, "the scenario's commands all stand in front of its first call"
            setup.append(s)

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        t = st.t = trk.Tracker(ctx, sc.nchan, sc.lo_delay, sc.cg_delay)
        st.objects.append(t)
        for s in setup:
            {"S": t.set_sat, "C": lambda ch, k: t.set_e1b_code(ch, sc.codes[k]), "G": t.set_rate_cg, "L": t.set_rate_lo, "l": t.set_gain_lo,
             "g": t.set_gain_cg, "P": t.set_polarity, "M": t.set_mask, "O": t.set_loop, "R": t.sampler_reset}[s[0]](*s[1:])
        st.d_bits = dev(st, sc.bits)
        st.getters = lambda: t.get_clocks()
        return st
    step = deep_vs_stepwise(make, script)
    recs = [[] for _ in range(sc.nchan)]
    for o_ep, o_cnt, cap in xs:
        counts = region(step, o_cnt, np.int32, (sc.nchan,))
        ep = region(step, o_ep, trk.epoch_dtype, (sc.nchan, cap))
        assert np.all(counts >= 0), counts
        for ch in range(sc.nchan):
            recs[ch] += [tc.record_tuple(e) for e in ep[ch, :counts[ch]]]
    dumps = [(step.rets[i][1], int(step.rets[i][0][0]), [int(r) for r in step.rets[i][0][1]]) for i in ds]
    tc.assert_equal({"records": recs, "dumps": dumps, "refused": []}, want, "stream order")


def test_nav_sync():
    """kg_nav: three golden streams (two C/A, one E1B) through kg_nav_push_bits_dev in unequal pushes, a mode change of channel 2 in
    mid-stream (it starts again on an E1B stream), then kg_nav_push_epochs_dev on epoch rows that carry one nav bit each.  Deep against
    stepwise; every frame record and the end states of the stepwise run against the model (tests/nav_model.py)."""
    from tests.test_nav_cpu import load_golden, same_frames, same_state
    g = load_golden()
    streams = [g["ca_random_2"]["bits"][:2400], g["e1b_bursts"]["bits"][:3000], g["ca_flip_between"]["bits"][:1500]]
    after = g["e1b_inverted"]["bits"][:1800]                # channel 2 after its mode change
    modes = [nav.L1, nav.E1B, nav.L1]
    sizes = (1, 16, 301, 17, 499, 501, 300, 2, 500, 33)
    models = [nm.Channel(m) for m in modes]
    rounds, at, r, switch_at = [], [0, 0, 0], 0, 4
    while True:
        if r == switch_at:
            streams[2], at[2], modes[2] = after, 0, nav.E1B
        pieces = []
        for ch in range(3):
            n = min(sizes[(r + 5 * ch) % len(sizes)], streams[ch].size - at[ch])
            pieces.append(streams[ch][at[ch]:at[ch] + n])
            at[ch] += n
        if not any(p.size for p in pieces):
            break
        rounds.append((pieces, list(modes)))
        r += 1
        assert r < 40
    assert len(rounds) >= 8
    R = Regions()
    script, outs, bufs = [], [], []
    for r, (pieces, md) in enumerate(rounds):
        nb = np.array([p.size for p in pieces], np.int32)
        stride, cap = max(int(nb.max()), 1), nav.cap_for(md, nb)
        host = np.zeros((3, stride), np.uint8)
        for ch, p in enumerate(pieces):
            host[ch, :p.size] = p
        bufs.append(host)
        o_fr, o_cnt = R.take(64 * max(cap, 1) * 3), R.take(12)
        outs.append((o_fr, o_cnt, max(cap, 1)))
        if r == switch_at:
            script.append(("set", lambda st: st.ns.set_mode(2, nav.E1B)))
        script.append(("call", lambda st, r=r, nb=nb, stride=stride, cap=cap, o_fr=o_fr, o_cnt=o_cnt: st.ns.push_dev(
            st.d_bits[r], stride, nb, st.d_out + o_fr, max(cap, 1), cap, st.d_out + o_cnt)))
        if r % 8 == 7 and r != switch_at - 1:
            script.append(("deep", "push %d" % r))
    rng = np.random.default_rng(110)
    ecounts, ecap = (300, 40, 37), 300
    rows = np.zeros((3, ecap), trk.epoch_dtype)
    rows.view(np.uint8)[:] = rng.integers(0, 256, rows.nbytes, dtype=np.uint8).reshape(rows.view(np.uint8).shape)
    eflags = [np.repeat(rng.integers(0, 2, 16), 20)[:300].astype(np.uint8), rng.integers(0, 2, 40).astype(np.uint8), rng.integers(0, 2, 37).astype(np.uint8)]
    for ch, f in enumerate(eflags):
        rows["flags"][ch, :f.size] = (rows["flags"][ch, :f.size] & ~np.uint32(trk.INAV)) | (f.astype(np.uint32) * trk.INAV)
    final_modes = rounds[-1][1]
    cap_e = nav.cap_for_epochs(final_modes, ecap)
    o_efr, o_ecnt = R.take(64 * max(cap_e, 1) * 3), R.take(12)
    script.append(("call", lambda st: st.ns.push_epochs_dev(st.d_ep, ecap, st.d_ecnt, ecap, st.d_out + o_efr, max(cap_e, 1), cap_e, st.d_out + o_ecnt)))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.ns = nav.NavSync(ctx, 3, [nav.L1, nav.E1B, nav.L1])
        st.objects.append(st.ns)
        st.d_bits = [dev(st, b) for b in bufs]
        st.d_ep, st.d_ecnt = dev(st, rows), dev(st, np.array(ecounts, np.int32))
        st.getters = lambda: [st.ns.state(ch) for ch in range(3)]
        return st
    step = deep_vs_stepwise(make, script)

    def frames_of(o_fr, o_cnt, fs):
        counts = region(step, o_cnt, np.int32, (3,))
        fr = region(step, o_fr, nav.frame_dtype, (3, fs))
        return [fr[ch, :counts[ch]] for ch in range(3)]
    nframes = 0
    for r, (pieces, md) in enumerate(rounds):
        if r == switch_at:
            models[2] = nm.Channel(nav.E1B)
        got = frames_of(*outs[r])
        for ch in range(3):
            same_frames(got[ch], nm.frames(models[ch].push(pieces[ch])), (r, ch))
            nframes += len(got[ch])
    got = frames_of(o_efr, o_ecnt, max(cap_e, 1))
    for ch in range(3):
        same_frames(got[ch], nm.frames(models[ch].push(models[ch].nav_bits(eflags[ch]))), ("epochs", ch))
        same_state(step.state[ch], models[ch].state(), ("end", ch))
    assert nframes >= 6


def test_ephemerides():
    """kg_eph: the golden C/A scenario (tests/golden/eph_ref.npz) through kg_eph_push_frames_dev in pushes of one to three frames, the
    binds of its channels between them, then kg_eph_sv_dev over its snapshots.  Deep against stepwise; the notes, the decoded
    ephemerides and the satellite positions of the stepwise run against the reference's records."""
    from tests.test_eph_cpu import check_sv, final_states, load_golden
    from tests.test_eph_gpu import segments
    s = load_golden()["ca"]
    nchan = 12
    R = Regions()
    script, bufs, outs, sat_of, ncall = [], [], [], {}, 0
    for binds, rows, order in segments(s["ev"]):
        for ch, sat, kind_ in binds:
            script.append(("set", lambda st, ch=ch, sat=sat, kind_=kind_: st.e.set_sat(ch, sat, kind_)))
            sat_of[ch] = sat
        ch_of = {a: ch for ch, idx in rows.items() for a in idx}
        k = 0
        while k < len(order):
            take = order[k:k + 1 + ncall % 3]
            k += len(take)
            per = {}
            for a in take:
                per.setdefault(ch_of[a], []).append(a)
            counts = np.array([len(per.get(ch, [])) for ch in range(nchan)], np.int32)
            stride = int(counts.max())
            host = np.zeros((nchan, stride), nav.frame_dtype)
            for ch, idx in per.items():
                host[ch, :len(idx)] = s["frames"][idx]
            o = R.take(32 * stride * nchan)
            bufs.append((host, counts))
            outs.append((o, stride, per))
            script.append(("call", lambda st, i=len(bufs) - 1, stride=stride, o=o: st.e.push_frames_dev(
                st.d_fr[i], stride, st.d_cnt[i], stride, st.d_out + o, stride)))
            ncall += 1
            if ncall % 8 == 0:
                script.append(("deep", "frames push %d" % ncall))
    assert ncall >= 6
    snaps = s["snaps"]
    o_sv = R.take(48 * max(snaps.size, 1))
    script.append(("call", lambda st: st.e.sv_dev(st.d_snaps, snaps.size, st.d_out + o_sv)))

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.e = eph.Ephemerides(ctx, nchan)
        st.objects.append(st.e)
        st.d_fr, st.d_cnt = [dev(st, h) for h, _ in bufs], [dev(st, c) for _, c in bufs]
        st.d_snaps = dev(st, snaps)
        st.getters = lambda: ([np.frombuffer(st.e.get(sat).tobytes(), np.uint8) for sat in sorted(set(sat_of.values()))],
                              [st.e.chan(ch) for ch in sorted(sat_of)], st.e.utc())
        return st
    step = deep_vs_stepwise(make, script)
    for o, stride, per in outs:
        notes = region(step, o, eph.note_dtype, (nchan, stride))
        for ch, idx in per.items():
            for j, a in enumerate(idx):
                assert notes[ch, j].tobytes() == s["notes"][a].tobytes(), ("note", a)
    check_sv(region(step, o_sv, eph.sv_dtype, (snaps.size,)).copy(), s, "stream order")
    final = final_states(s)
    for k, sat in enumerate(sorted(set(sat_of.values()))):
        assert step.state[0][k].tobytes() == final[sat].tobytes(), ("kg_ephem of satellite", sat)


def line_script_calls(lines, cut):
    """the B lines of a script of tests/fftext_common.py / tests/iqd_common.py grouped into calls: a call ends at a command, after `cut`
    blocks, or (iqd) where the block length changes -> [("cmd", line) | ("blocks", [(line fields, block number)])]"""
    out, pend, seen = [], [], 0
    for l in lines:
        if l[0] == "B":
            f = l.split()
            if pend and (len(pend) == cut or (len(f) == 4 and pend[0][0][2] != f[2])):
                out.append(("blocks", pend))
                pend = []
            pend.append((f, seen))
            seen += 1
        else:
            if pend:
                out.append(("blocks", pend))
                pend = []
            out.append(("cmd", l))
    if pend:
        out.append(("blocks", pend))
    return out, seen


def test_fft_extension():
    """kg_fftext: the script of tests/fftext_common.py with a clear and a new integration time in mid-stream (host-only commands: they
    neither enqueue nor wait, the zeroing rides on the channel's next block), cut into calls of two blocks.  The row map a call
    returns at once places the next call's rows.  Deep against stepwise; the stepwise side through check_against_golden."""
    name = "clear_itime_mid"
    lines, (_, spec) = fc.scripts()[name], fc.pool()
    groups, nb = line_script_calls(lines, 2)
    W = 1024
    script, calls = [], []
    for kind_, v in groups:
        if kind_ == "cmd":
            op = v[0]
            fn = {"R": lambda st, v=v: st.fx.set_rate(float(v[2:])),
                  "S": lambda st, v=v: st.fx.set_run(0, int(v[2:].split()[0]), int(v[2:].split()[1]) != 0, int(v[2:].split()[2]) == fc.QAM),
                  "I": lambda st, v=v: st.fx.set_itime(0, float(v[2:])), "C": lambda st: st.fx.clear(0)}[op]
            script.append(("host", fn))
            continue
        blocks = np.ascontiguousarray(spec[[int(f[2]) for f, _ in v]])
        inst = [int(f[1]) for f, _ in v]

        def fn(st, i=len(calls), inst=inst, n=len(v)):
            m = st.fx.process_dev([0] * n, [1] * n, inst, st.d_spec[i], W, st.d_out + W * st.at, W, n)
            st.at += m.shape[0]
            return m
        calls.append((blocks, [k for _, k in v]))
        script.append(("call", fn))
        if len(calls) % 8 == 0:
            script.append(("deep", "fftext call %d" % len(calls)))
    assert len(calls) >= 6

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=W * nb)
        st.fx = fftext.FftExt(ctx, 1)
        st.objects.append(st.fx)
        st.at = 0
        st.d_spec = [dev(st, b) for b, _ in calls]
        st.getters = lambda: st.fx.state(0, sums=True)
        return st
    step = deep_vs_stepwise(make, script)
    sent, bins = np.zeros(nb, np.int32), []
    maps = [r for (k, _), r in zip(script, step.rets) if k == "call"]
    for (_, blks), m in zip(calls, maps):
        for ch, ent, blk, b in m:
            assert ch == 0 and blk == 0
            bins.append(int(b))
            sent[blks[ent]] = 1
    info, ncma, pwr = step.state
    n = len(bins)
    assert np.all(step.out[W * n:] == FILL)
    got = {"sent": sent, "bins": np.array(bins, np.int32), "rows": step.out[:W * n].reshape(n, W), "run": int(info["run"]), "instance": int(info["instance"]),
           "nbins": int(info["bins"]), "reset": int(info["reset"]), "fft_scale": np.float32(info["fft_scale"]), "spectrum_scale": np.float32(info["spectrum_scale"]),
           "fi": float(info["fi"]), "fft_sec": float(info["fft_sec"]), "time": float(info["time"]), "ncma": ncma, "pwr": pwr}
    fc.check_against_golden(fc.load(), name, got)


def test_iq_display():
    """kg_iqd: the script of tests/iqd_common.py that changes the points in mid-lap (blocks of 512 and of 170 samples, host-only commands
    between them), one block a call.  The row map and the status map are returned at once.  Deep against stepwise; the stepwise side
    through check_against_golden."""
    name = "points_change"
    lines, samples = ic.scripts()[name], ic.pool()
    groups, nb = line_script_calls(lines, 1)
    R = Regions()
    script, calls, registered = [], [], False
    for kind_, v in groups:
        if kind_ == "cmd":
            script.append(("host", lambda st, v=v: ic.apply_command(st.q, 0, v)))
            if v[0] in "NR":
                registered = v[0] == "R" and int(v[2:].split()[0]) != 0
            continue
        if not registered:
            continue
        (f, blk), = v
        inst, ns, off = int(f[1]), int(f[2]), int(f[3])
        cap = (ns + ic.RING) * 4
        o_rows, o_st = R.take(cap), R.take(24)

        def fn(st, i=len(calls), inst=inst, ns=ns, cap=cap, o_rows=o_rows, o_st=o_st):
            m, snt = st.q.process_dev([0], [1], [inst], ns, st.d_iq[i], ns, st.d_out + o_rows, cap, st.d_out + o_st, 1, ns)
            return m, snt
        calls.append((np.ascontiguousarray(samples[off:off + ns]), blk, o_rows, o_st))
        script.append(("call", fn))
        if len(calls) % 8 == 0:
            script.append(("deep", "iqd call %d" % len(calls)))
    assert len(calls) >= 6

    def make(ctx):
        st = state_of(ctx=ctx, out_bytes=R.size)
        st.q = iqd.IqDisplay(ctx, 1)
        st.objects.append(st.q)
        st.d_iq = [dev(st, x) for x, _, _, _ in calls]
        st.getters = lambda: ic.state_of(st.q, 0)
        return st
    step = deep_vs_stepwise(make, script)
    nrows, sent, status = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.zeros(nb, iqd.status_dtype)
    cmd, ln, rows = [], [], []
    maps = [r for (k, _), r in zip(script, step.rets) if k == "call"]
    for (_, blk, o_rows, o_st), (m, snt) in zip(calls, maps):
        at = 0
        for r in m:
            assert r["ch"] == 0 and r["off"] == at
            nrows[blk] += 1
            cmd.append(int(r["cmd"])); ln.append(int(r["len"]))
            rows.append(step.out[o_rows + at:o_rows + at + int(r["len"])].copy())
            at += int(r["len"])
        sent[blk] = snt[0]
        status[blk] = region(step, o_st, iqd.status_dtype, (1,))[0]
    got = {"nrows": nrows, "cmd": np.array(cmd, np.int32), "len": np.array(ln, np.int32), "rows": rows, "sent": sent, "status": status[sent != 0]}
    got.update(step.state)
    ic.check_against_golden(ic.load(), name, got)
