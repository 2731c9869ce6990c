"""Containment of the device entry points of include/kiwigpu.h, part 2: kg_post -- the fused pass (every output NULL in turn, the
rows a mode does not produce, the stages that run over d_s16 behind it) and the standalone call sites of its stages.  The four
properties (W, R, P, E) and the layouts are those of tests/test_containment_gpu.py."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post
from flydog_sdr_gps_amd._lib import check, ptr
from tests.guarded import contain

pytestmark = pytest.mark.gpu

KG_ERR_INVALID = -2
FS = 12000.0


def fir_out(n, seed, amp=0.3):
    """what CFastFIR hands over: a carrier, a tone beside it and noise"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = amp * (np.exp(2j * np.pi * 1000.0 * t) + 0.6 * np.exp(2j * np.pi * (300.0 + 50 * (seed % 7)) * t))
    return (x + 0.08 * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64) * np.float32(8000.0)


def audio(n, seed):
    r = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = 6000 * np.sin(2 * np.pi * 700.0 * t) + 800 * r.standard_normal(n)
    x[11::97] += 20000                                                  # clicks
    return np.clip(x, -32768, 32767).astype(np.int16)


def configure(P, ch, mode):
    P.set_agc(ch, True, False, -100, 50, 6, 1000, FS)
    P.set_smeter(ch, FS)
    P.set_am_passband(ch, -2700.0, 2700.0, FS)
    P.set_mode(ch, mode)
    P.reset(ch)
    P.squelch_setup(ch, FS)
    P.squelch_set(ch, 0, 0)


MODES = {0: post.MODE_SSB, 1: post.MODE_AM, 2: post.MODE_NBFM, 3: post.MODE_IQ, 4: post.MODE_SAM, 5: post.MODE_SAS}
LIST = [4, 0, 5, 1, 3, 2]


def used_of(mode, nsamps):
    """the rows the header says a mode writes: d_s16 (not the stereo modes), d_demod (AM, NBFM), d_agc (not SSB)"""
    return (0 if mode in post.STEREO_MODES else 2 * nsamps, 4 * nsamps if mode in (post.MODE_AM, post.MODE_NBFM) else 0,
            0 if mode == post.MODE_SSB else 8 * nsamps)


def all_state(P, chans):
    return P.smeter(chans), P.squelch_state(chans), P.sam_state(chans)


@pytest.mark.parametrize("null", ["none", "s16", "demod", "agc"])
@pytest.mark.parametrize("nsamps", [1, 65, 511, 1024])
def test_post_process(gpu_ctx, nsamps, null):
    """one channel each of SSB, AM, NBFM, IQ, SAM, SAS in one list; two passes so that the AGC, the detectors and the PLL carry"""
    x = [[fir_out(nsamps, 100 * call + ch) for ch in LIST] for call in range(2)]
    used = [used_of(MODES[ch], nsamps) for ch in LIST]

    def case(lay):
        P = Post(gpu_ctx, nchan=6)
        try:
            for ch, mode in MODES.items():
                configure(P, ch, mode)
            res = []
            for call in range(2):
                g_in, s_in = lay.inp(x[call], 8)
                g_s16, s_out = lay.out(6, nsamps, 2, 2)                 # one out_stride, in elements of each output
                g_dem, _ = lay.out(6, nsamps, 4, 4, stride=s_out)
                g_agc, _ = lay.out(6, nsamps, 8, 8, stride=s_out)
                P.process_dev(LIST, g_in.ptr, s_in, nsamps, 0 if null == "s16" else g_s16.ptr, 0 if null == "demod" else g_dem.ptr,
                              0 if null == "agc" else g_agc.ptr, s_out)
                gpu_ctx.sync()
                res.append((lay.take(g_s16, [0 if null == "s16" else u[0] for u in used]),
                            lay.take(g_dem, [0 if null == "demod" else u[1] for u in used]),
                            lay.take(g_agc, [0 if null == "agc" else u[2] for u in used])))
            return res, all_state(P, list(range(6)))
        finally:
            P.close()

    contain(gpu_ctx, case)


# channel -> what runs over its d_s16 row behind the pass
def arm_stage(P, ch):
    if ch == 0:
        P.set_nr_algo(ch, post.NR_WDSP)
        for t in (0, 1):
            for k, v in enumerate([64, 16, 1e-4, 0.1]):
                P.set_nr_param(ch, t, k, v)
            P.set_nr_enable(ch, t, 1)
    elif ch == 1:
        P.set_nr_algo(ch, post.NR_ORIG)
        for t in (0, 1):
            for k, v in enumerate([0, 0, 0]):
                P.set_nr_param(ch, t, k, v)
            P.set_nr_enable(ch, t, 1)
    elif ch == 2:
        P.nrs_passband(ch, 300.0, 2700.0)
        P.nrs_select(ch)
        for k, v in enumerate([1, 0.95, 1000]):
            P.set_nr_param(ch, 0, k, v)
    else:
        P.nbw_init(ch, [3.0, 10, 7])
        P.set_nbw(ch, 1)


def stage_state(P, chans):
    return [P.nr_state(chans, t, weights=True) for t in (0, 1)], P.nrs_state(chans), P.nbw_state(chans)


def test_post_process_with_the_fused_stages(gpu_ctx):
    """NR_WDSP, NR_ORIG, NR_SPECTRAL and NB_WILD over the d_s16 rows of one pass, at their block of 512"""
    n, lst = 512, [2, 0, 3, 1]
    x = [[fir_out(n, 200 * call + ch) for ch in lst] for call in range(2)]

    def case(lay):
        P = Post(gpu_ctx, nchan=4)
        try:
            for ch in range(4):
                configure(P, ch, post.MODE_AM if ch == 1 else post.MODE_SSB)
                arm_stage(P, ch)
            res = []
            for call in range(2):
                g_in, s_in = lay.inp(x[call], 8)
                g_s16, s_out = lay.out(4, n, 2, 2)
                g_agc, _ = lay.out(4, n, 8, 8, stride=s_out)
                P.process_dev(lst, g_in.ptr, s_in, n, g_s16.ptr, 0, g_agc.ptr, s_out)
                gpu_ctx.sync()
                res.append((lay.take(g_s16, 2 * n), lay.take(g_agc, [8 * n if ch == 1 else 0 for ch in lst])))
            return res, all_state(P, list(range(4))), stage_state(P, list(range(4)))
        finally:
            P.close()

    contain(gpu_ctx, case)


def standalone(gpu_ctx, x, lst, nsamps, setup, call, state):
    """out of place, then in place (the header allows d_in == d_out): W, R, P, E for both, and the same result"""
    def make(in_place):
        def case(lay):
            P = Post(gpu_ctx, nchan=3)
            try:
                for ch in range(3):
                    configure(P, ch, post.MODE_SSB)
                    setup(P, ch)
                res = []
                for k in range(2):
                    g_in, s_in = lay.inp(x[k], 2, inplace=in_place)
                    g_out, s_out = (g_in, s_in) if in_place else lay.out(3, nsamps, 2, 2)
                    call(P, g_in.ptr, s_in, g_out.ptr, s_out)
                    gpu_ctx.sync()
                    res.append(lay.take(g_out, 2 * nsamps))
                return res, state(P)
            finally:
                P.close()
        return case

    assert contain(gpu_ctx, make(False)) == contain(gpu_ctx, make(True))


@pytest.mark.parametrize("nsamps", [1, 65, 512])
def test_post_nr_process(gpu_ctx, nsamps):
    lst = [2, 0, 1]
    x = [[audio(nsamps, 10 * k + ch) for ch in lst] for k in range(2)]

    def setup(P, ch):
        P.set_nr_algo(ch, post.NR_ORIG if ch == 1 else post.NR_WDSP)
        for k, v in enumerate([0, 0, 0] if ch == 1 else [64, 16, 1e-4, 0.1]):
            P.set_nr_param(ch, post.NR_DENOISE, k, v)

    standalone(gpu_ctx, x, lst, nsamps, setup,
               lambda P, di, si, do, so: P.nr_process_dev(lst, post.NR_DENOISE, di, si, nsamps, do, so),
               lambda P: P.nr_state([0, 1, 2], post.NR_DENOISE, weights=True))


@pytest.mark.parametrize("nsamps", [512, 1536])
def test_post_nrs_process(gpu_ctx, nsamps):
    lst = [2, 0, 1]
    x = [[audio(nsamps, 20 * k + ch) for ch in lst] for k in range(2)]

    def setup(P, ch):
        P.nrs_passband(ch, 300.0, 2700.0 + 100 * ch)
        P.nrs_select(ch)
        for k, v in enumerate([1, 0.95, 1000]):
            P.set_nr_param(ch, 0, k, v)

    standalone(gpu_ctx, x, lst, nsamps, setup, lambda P, di, si, do, so: P.nrs_process_dev(lst, di, si, nsamps, do, so),
               lambda P: P.nrs_state([0, 1, 2]))


@pytest.mark.parametrize("nsamps", [512, 1536])
def test_post_nbw_process(gpu_ctx, nsamps):
    lst = [2, 0, 1]
    x = [[audio(nsamps, 30 * k + ch) for ch in lst] for k in range(2)]

    def setup(P, ch):
        P.nbw_init(ch, [3.0, 10 + ch, 7])

    standalone(gpu_ctx, x, lst, nsamps, setup, lambda P, di, si, do, so: P.nbw_process_dev(lst, di, si, nsamps, do, so),
               lambda P: P.nbw_state([0, 1, 2]))


@pytest.mark.parametrize("kind", [post.CFIR_REAL_REAL, post.CFIR_REAL_MONO16, post.CFIR_MONO16_MONO16])
@pytest.mark.parametrize("nsamps", [1, 65, 511])
def test_post_cfir_process(gpu_ctx, nsamps, kind):
    """float rows 4-byte aligned, int16 rows 2-byte; nsamps elements of each row, in and out"""
    lst = np.array([2, 0, 1], np.int32)
    ein, eout = (2 if kind == post.CFIR_MONO16_MONO16 else 4), (4 if kind == post.CFIR_REAL_REAL else 2)
    x = [[audio(nsamps, 40 * k + ch) if ein == 2 else audio(nsamps, 40 * k + ch).astype(np.float32) * np.float32(0.37) for ch in lst]
         for k in range(2)]

    def case(lay):
        P = Post(gpu_ctx, nchan=3)
        try:
            for ch in range(3):
                configure(P, ch, post.MODE_AM)
            res = []
            for k in range(2):
                g_in, s_in = lay.inp(x[k], ein)
                g_out, s_out = lay.out(3, nsamps, eout, eout)
                check(gpu_ctx.lib.kg_post_cfir_process_dev(P.h, ptr(lst), 3, post.CFIR_AM, kind, ptr(g_in.ptr), s_in, nsamps, ptr(g_out.ptr), s_out),
                      "kg_post_cfir_process_dev")
                gpu_ctx.sync()
                res.append(lay.take(g_out, eout * nsamps))
            return res
        finally:
            P.close()

    contain(gpu_ctx, case)


@pytest.mark.parametrize("nsamps", [1, 65, 511])
def test_post_squelch_perform(gpu_ctx, nsamps):
    lst = np.array([2, 0, 1], np.int32)
    x = [[audio(nsamps, 50 * k + ch).astype(np.float32) * np.float32(0.2) for ch in lst] for k in range(2)]

    def case(lay):
        P = Post(gpu_ctx, nchan=3)
        try:
            for ch in range(3):
                configure(P, ch, post.MODE_NBFM)
                P.squelch_set(ch, 20 + 10 * ch, 0)
            res = []
            for k in range(2):
                g_in, s_in = lay.inp(x[k], 4)
                g_out, s_out = lay.out(3, nsamps, 2, 2)
                check(gpu_ctx.lib.kg_post_squelch_perform_dev(P.h, ptr(lst), 3, ptr(g_in.ptr), s_in, nsamps, ptr(g_out.ptr), s_out),
                      "kg_post_squelch_perform_dev")
                gpu_ctx.sync()
                res.append((lay.take(g_out, 2 * nsamps), P.squelch_state([0, 1, 2])))
            return res
        finally:
            P.close()

    contain(gpu_ctx, case)


def test_post_refuses_misaligned_buffers(gpu_ctx):
    """the pointers are dereferenced as their element type: complex float 8 bytes, float 4, int16 2 -- refused on the host otherwise,
    nothing launched, no state advanced"""
    P = Post(gpu_ctx, nchan=1)
    d = gpu_ctx.alloc(1 << 16)
    try:
        configure(P, 0, post.MODE_AM)
        P.set_nr_algo(0, post.NR_WDSP)
        before = P.smeter([0])
        L, lst, n = gpu_ctx.lib, np.zeros(1, np.int32), 64
        a, b, c, e = d, d + 4096, d + 8192, d + 16384
        for fir, s16, dem, agc in ((a + 4, b, c, e), (a, b + 1, c, e), (a, b, c + 2, e), (a, b, c, e + 4)):
            assert L.kg_post_process_dev(P.h, ptr(lst), 1, ptr(fir), n, n, ptr(s16), ptr(dem), ptr(agc), n) == KG_ERR_INVALID
        for i, o in ((a + 1, b), (a, b + 1)):
            assert L.kg_post_nr_process_dev(P.h, ptr(lst), 1, 0, ptr(i), n, n, ptr(o), n) == KG_ERR_INVALID
            assert L.kg_post_nrs_process_dev(P.h, ptr(lst), 1, ptr(i), 512, 512, ptr(o), 512) == KG_ERR_INVALID
            assert L.kg_post_nbw_process_dev(P.h, ptr(lst), 1, ptr(i), 512, 512, ptr(o), 512) == KG_ERR_INVALID
            assert L.kg_post_cfir_process_dev(P.h, ptr(lst), 1, post.CFIR_AM, post.CFIR_MONO16_MONO16, ptr(i), n, n, ptr(o), n) == KG_ERR_INVALID
        for i, o in ((a + 2, b), (a, b + 1)):
            assert L.kg_post_cfir_process_dev(P.h, ptr(lst), 1, post.CFIR_AM, post.CFIR_REAL_MONO16, ptr(i), n, n, ptr(o), n) == KG_ERR_INVALID
            assert L.kg_post_squelch_perform_dev(P.h, ptr(lst), 1, ptr(i), n, n, ptr(o), n) == KG_ERR_INVALID
        assert L.kg_post_cfir_process_dev(P.h, ptr(lst), 1, post.CFIR_AM, post.CFIR_REAL_REAL, ptr(a), n, n, ptr(b + 2), n) == KG_ERR_INVALID
        after = P.smeter([0])
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        gpu_ctx.free(d)
        P.close()
