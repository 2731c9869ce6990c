"""Lifecycle: every object of the C ABI created, used once and destroyed, many times over; the
device's free memory must come back (no leak in create/destroy or in the per-call scratch).

The failure paths: the library counts its live device and pinned allocations (live_allocs) and, under
KIWIGPU_TUNING=1, refuses the k-th allocation for KIWIGPU_FAIL_ALLOC=k -- on the host, no device memory is filled.  Every create is
refused at every allocation it makes and must hold nothing afterwards; every grow-on-demand site is refused at every allocation
it makes and must work afterwards as if nothing had happened."""
import gc

import numpy as np
import pytest

from flydog_sdr_gps_amd import (Adpcm, Aperture, Context, Ddc, Ephemerides, FastFir, KiwiGpuError, NavSync, NoiseBlanker, PositionSolver,
                                Post, RxDdc, Searcher, Tracker, Waterfall, WfParams, acq, ddc, handoff, live_allocs, nav, post, prn, sats,
                                synth, wf, wire)
from flydog_sdr_gps_amd.rxbank import RxBank

pytestmark = pytest.mark.gpu


def use_everything(ctx):
    s = Searcher(ctx, max_blocks=2)
    s.set_code(0, prn.cacode(*sats.SATS[0][1:3]))
    s.set_code(1, np.arange(4092, dtype=np.uint8) & 1, boc=True)      # a 16368-lag SV: the 512-thread correlator and its layout
    s.sample_iq16(synth.config1_iq16(seed=1), block=0)
    s.correlate_async([0, 1], nblocks=1)
    s.fetch()
    s.close()
    ctx.mark(7)                                                        # the profiling marker kernel
    ctx.sync()
    w = Waterfall(ctx, nchan=2)
    w.set_tables()
    p = WfParams.for_zoom(3, 1000.0)
    w.set_channel(0, p)
    row = w.frames([0], synth.wf_iq_frame(seed=2)[None])[0]
    w.close()
    d = Ddc(ctx, nchan=2, max_samples=1 << 16)
    d.set_wf(0, p.i_offset, p.decim)
    d.push(np.zeros(1 << 14, np.int16), [0])
    d.close()
    r = RxDdc(ctx, nchan=2, max_samples=1 << 16)
    r.set_freq(0, 12345)
    r.push(np.zeros(1 << 15, np.int16), [0])
    r.close()
    f = FastFir(ctx, nchan=2, max_in=1024)
    f.setup(0, 300.0, 2700.0, 0.0, 12000.0)
    y = f.process(0, np.ones(1024, np.complex64))
    f.close()
    P = Post(ctx, nchan=2)
    P.set_agc(0, True, False, -100, 50, 6, 1000, 12000.0)
    P.set_mode(0, post.MODE_SSB)
    s16, _, _ = P.process([0], y[None, :512])
    P.smeter([0])
    P.close()
    A = Adpcm(ctx, nchan=2)
    A.encode([0], s16)
    A.close()
    wire.wf_packets(ctx, row[None], [(1, 3, 5, True)])
    a = Aperture(ctx, nchan=2)
    a.update([0], row[None], [(handoff.MMA, 8.0, True, False)])
    a.report([0])
    a.close()


def test_create_use_destroy_returns_device_memory():
    ctx = Context(0)
    try:
        use_everything(ctx)                       # first round: code objects, lazily grown scratch
        free0, total = ctx.mem_info()
        for _ in range(15):
            use_everything(ctx)
        free1, _ = ctx.mem_info()
        assert total > 200 * 2 ** 30              # an MI355X: 288 GB
        assert free0 - free1 < 8 * 2 ** 20, "device memory shrank by %.1f MiB over 15 rounds" % ((free0 - free1) / 2 ** 20)
    finally:
        ctx.close()


def test_contexts_come_and_go():
    gc.collect()
    live0 = live_allocs()
    free = []
    for _ in range(6):
        c = Context(0)
        s = Searcher(c, max_blocks=1)
        s.close()
        free.append(c.mem_info()[0])
        c.close()
    assert max(free) - min(free[1:]) < 64 * 2 ** 20
    assert live_allocs() == live0



def test_mark_rejects_tags_out_of_range(gpu_ctx):
    from flydog_sdr_gps_amd import KiwiGpuError
    gpu_ctx.mark(1)
    gpu_ctx.mark(65535)
    gpu_ctx.sync()
    for bad in (0, -3, 65536):
        with pytest.raises(KiwiGpuError):
            gpu_ctx.mark(bad)


# ---- exact accounting, and every allocation refused once -------------------------------------------------------------
NOMEM = -4
P3 = WfParams.for_zoom(3, 1000.0)
IQ = synth.wf_iq_frame(seed=2)
ROW = np.random.Generator(np.random.PCG64(7)).integers(0, 256, 1024, dtype=np.uint8)
APER_CFG = [(handoff.MMA, 8.0, True, False)]


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def run_ctx(c):
    c.mark(7)
    c.sync()


def prep_searcher(s):
    s.set_code(0, prn.cacode(*sats.SATS[0][1:3]))


def run_searcher(s):
    s.sample_iq16(rng_of(3).integers(-100, 100, 2 * s.nsamples).astype(np.int16), block=0)
    s.correlate_async([0], nblocks=1)
    return s.fetch()


def prep_waterfall(w):
    w.set_tables()
    w.set_channel(0, P3)


def prep_ddc(d):
    d.set_wf(0, P3.i_offset, P3.decim)


def prep_post(p):
    p.set_agc(0, True, False, -100, 50, 6, 1000, 12000.0)
    p.set_mode(0, post.MODE_SSB)


def run_post(p):
    p.process([0], np.ones((1, 512), np.complex64))
    p.smeter([0])


def run_aperture(a):
    a.update([0], ROW[None], APER_CFG)
    return a.report([0])


def run_bank(bank):
    from .test_receivers_gpu import _small_mix
    bank.configure(_small_mix([5, 6], bank.n))
    adc = synth.adc_stream(bank.n, 0x5EED0047)
    d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(d_adc, adc)
    bank.step(d_adc)
    bank.sync()
    bank.ctx.free(d_adc)


def prep_bank(bank):
    """run_bank up to its step; the ADC block stays for the bank's steps and goes when the bank is closed"""
    from .test_receivers_gpu import _small_mix
    bank.configure(_small_mix([5, 6], bank.n))
    adc = synth.adc_stream(bank.n, 0x5EED0047)
    bank.d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(bank.d_adc, adc)
    close = bank.close

    def close_with_adc():
        if bank.h:
            bank.ctx.free(bank.d_adc)
        close()
    bank.close = close_with_adc


# The smallest number of steps after which a fresh bank's audio_map() reports one completed sound block for receiver 0: a step of
# 8192 * 16 = 131072 ADC samples at the audio DDC's decimation of 10416 (RX_STD) is 12.58 rx_iq_t records (12 or 13 a step,
# floor(12.5837 k) after k steps), a sound block takes 512: 40 steps give 503, 41 give 515.  The call's last step is the one that
# completes the block, so every extension has rows to show for it.
BANK_EXT_STEPS = 41


def bank_ext(tell, outputs):
    """-> the call of a bank extension's growth case: its first commands for receiver 0, BANK_EXT_STEPS steps, the last step's outputs"""
    def call(bank):
        tell(bank)
        for _ in range(BANK_EXT_STEPS):
            bank.step(bank.d_adc)
        bank.sync()
        return [outputs(bank), bank.audio_map()]
    return call


def tell_fftext(bank):
    from flydog_sdr_gps_amd import fftext
    bank.fftext_set_rate(bank.fs)
    bank.fftext_set_run(0, fftext.SPEC)


def tell_iqd(bank):
    bank.iqd_init(0)
    bank.iqd_set_run(0, 1, bank.fs)


def tell_lorc(bank):
    bank.lorc_init(0, bank.fs, 600)
    bank.lorc_set_gri(0, 0, 2990)
    bank.lorc_set_gri(0, 1, 4970)
    bank.lorc_start(0)


def fax_flat(bank):
    return [[rx, recs, rows] for rx, (recs, rows) in sorted(bank.fax_out().items())]


def prep_tracker(t):
    from . import trk_common as tc
    for ch, word in ((0, tc.CA1), (1, tc.CA7)):
        t.set_sat(ch, word)
        t.set_rate_cg(ch, tc.NOM)
    t.sampler_reset()


def run_tracker(t):
    bits = rng_of(13).integers(0, 256, 4096, dtype=np.uint8)
    return t.process(bits, 8 * bits.size)


def run_nav(v):
    r = rng_of(17)
    return v.push([r.integers(0, 2, 6000, dtype=np.uint8), r.integers(0, 2, 5000, dtype=np.uint8)])      # past the workspace made at create


def eph_golden():
    from .test_eph_cpu import load_golden
    from .test_eph_gpu import segments
    g = load_golden()
    binds, rows, _ = segments(g["gal"]["ev"])[0]
    frames = [np.resize(g["gal"]["frames"][rows[ch]], 70) for ch in range(2)]           # 70 a channel: past the workspace made at create
    return binds[:2], frames, g["ca"]["snaps"][:16]


def prep_eph(e):
    for ch, sat, kind in eph_golden()[0]:
        e.set_sat(ch, sat, kind)


def run_eph(e):
    return e.push_frames(eph_golden()[1])


def run_eph_sv(e):
    return e.sv(eph_golden()[2])


def run_pos(p):
    from .test_pos_cpu import load_golden
    s = load_golden()["main"]
    return p.solve(np.ascontiguousarray(s["snaps"][5:8]), np.ascontiguousarray(s["sv"][5:8]), s["ticks"][5:8].copy(), np.array([0, 1, 0x802], np.uint32))


# name -> (create(ctx), configure, use once); the shapes are use_everything's
CREATES = {
    "Context": (lambda c: Context(0), None, run_ctx),
    "Searcher-16384": (lambda c: Searcher(c, max_blocks=2), prep_searcher, run_searcher),
    "Searcher-65536": (lambda c: Searcher(c, max_blocks=2, nsamples=acq.NSAMPLES_10MS, fft_len=acq.FFT_LEN_10MS), prep_searcher, run_searcher),
    "Waterfall": (lambda c: Waterfall(c, nchan=2), prep_waterfall, lambda w: w.frames([0], IQ[None])),
    "Ddc": (lambda c: Ddc(c, nchan=2, max_samples=1 << 16), prep_ddc, lambda d: d.push(np.zeros(1 << 14, np.int16), [0])),
    "RxDdc-std": (lambda c: RxDdc(c, nchan=2, max_samples=1 << 16, mode=ddc.RX_STD), lambda r: r.set_freq(0, 12345),
                  lambda r: r.push(np.zeros(1 << 15, np.int16), [0])),
    "RxDdc-wide": (lambda c: RxDdc(c, nchan=2, max_samples=1 << 16, mode=ddc.RX_WIDE), lambda r: r.set_freq(0, 12345),
                   lambda r: r.push(np.zeros(1 << 15, np.int16), [0])),
    "RxDdc-rx14": (lambda c: RxDdc(c, nchan=2, max_samples=1 << 16, mode=ddc.RX_14), lambda r: r.set_freq(0, 12345),
                   lambda r: r.push(np.zeros(1 << 15, np.int16), [0])),
    "FastFir": (lambda c: FastFir(c, nchan=2, max_in=1024), lambda f: f.setup(0, 300.0, 2700.0, 0.0, 12000.0),
                lambda f: f.process(0, np.ones(1024, np.complex64))),
    "Post": (lambda c: Post(c, nchan=2), prep_post, run_post),
    "Adpcm": (lambda c: Adpcm(c, nchan=2), None, lambda a: a.encode([0], np.zeros((1, 512), np.int16))),
    "Aperture": (lambda c: Aperture(c, nchan=2), None, run_aperture),
    "NoiseBlanker": (lambda c: NoiseBlanker(c, nchan=2, max_in=1024), lambda b: b.setup(0, 12000.0, [100.0, 50.0]),
                     lambda b: b.process(0, rng_of(11).standard_normal((512, 2)).astype(np.float32))),
    "RxBank": (lambda c: RxBank(2, 8192 * 16), None, run_bank),
    "Tracker": (lambda c: Tracker(c, 2), prep_tracker, run_tracker),
    "NavSync": (lambda c: NavSync(c, 2, [nav.L1, nav.E1B]), None, run_nav),
    "Ephemerides": (lambda c: Ephemerides(c, 2), prep_eph, run_eph),
    "PositionSolver": (lambda c: PositionSolver(c), lambda p: p.set_mode(1, 1), run_pos),
}


def refused_until_it_works(monkeypatch, call, cap, after_refusal=None):
    """call() under KIWIGPU_FAIL_ALLOC = 1, 2, ...: status -4 naming the variable until the first success, which must come by k = cap
    and after at least one refusal -> (what the successful call returned, refusals).  The variables are gone afterwards."""
    monkeypatch.setenv("KIWIGPU_TUNING", "1")
    try:
        for k in range(1, cap + 1):
            monkeypatch.setenv("KIWIGPU_FAIL_ALLOC", str(k))
            try:
                out = call()
            except KiwiGpuError as e:
                assert e.status == NOMEM and "KIWIGPU_FAIL_ALLOC" in str(e), (k, e)
                if after_refusal:
                    after_refusal(k)
                continue
            assert k > 1, "allocation 1 was not refused: the call allocates nothing or the switch is dead"
            return out, k - 1
        pytest.fail("no success up to KIWIGPU_FAIL_ALLOC=%d" % cap)
    finally:
        monkeypatch.delenv("KIWIGPU_FAIL_ALLOC")
        monkeypatch.delenv("KIWIGPU_TUNING")


def as_bytes(x):
    return [as_bytes(v) for v in x] if isinstance(x, (list, tuple)) else np.ascontiguousarray(x).tobytes()


def test_live_allocations_return_exactly():
    gc.collect()
    live0 = live_allocs()
    ctx = Context(0)
    assert live_allocs() > live0
    use_everything(ctx)
    ctx.close()
    assert live_allocs() == live0
    for name in ("RxBank", "Tracker", "NavSync", "Ephemerides", "PositionSolver"):
        create, prep, run = CREATES[name]
        ctx = Context(0)
        obj = create(ctx)
        if prep:
            prep(obj)
        run(obj)
        if name == "Ephemerides":
            run_eph_sv(obj)
        obj.close()
        ctx.close()
        assert live_allocs() == live0, name


@pytest.mark.parametrize("name", list(CREATES))
def test_create_survives_every_refused_allocation(monkeypatch, name):
    create, prep, run = CREATES[name]
    gc.collect()
    live0 = live_allocs()
    ctx = None if name == "Context" else Context(0)
    live1 = live_allocs()

    def nothing_held(k):
        assert live_allocs() == live1, "after the refusal of allocation %d" % k

    obj, refusals = refused_until_it_works(monkeypatch, lambda: create(ctx), 400 if name == "RxBank" else 64, nothing_held)
    print("%s: %d allocations, each refused once" % (name, refusals))
    assert refusals >= 1
    if prep:
        prep(obj)
    run(obj)
    obj.close()
    if ctx is not None:
        ctx.close()
    assert live_allocs() == live0


def then(prep, run):
    return lambda o: ((prep(o) if prep else None), run(o))[1]


# name -> (create(ctx), what comes before (no refusal yet), the call that grows something); outputs compared with a fresh object's
GROWTHS = {
    "Waterfall.frames": CREATES["Waterfall"],
    "Waterfall.debug_frame": (CREATES["Waterfall"][0], then(*CREATES["Waterfall"][1:]), lambda w: w.debug_frame(0, IQ)),     # only the taps grow
    "Waterfall.debug_frame-first": (CREATES["Waterfall"][0], prep_waterfall, lambda w: w.debug_frame(0, IQ)),                # staging and taps
    "FastFir.process": CREATES["FastFir"],
    "NoiseBlanker.process": CREATES["NoiseBlanker"],
    "kg_ctx_stage": (CREATES["Aperture"][0], None, lambda a: (a.update([0], ROW[None], APER_CFG), a.get(0))[1]),   # a fresh context's ring
    "Ephemerides.push_frames": CREATES["Ephemerides"],
    "Ephemerides.sv": (CREATES["Ephemerides"][0], then(prep_eph, run_eph), run_eph_sv),
    "NavSync.push": CREATES["NavSync"],
    "Tracker.process": CREATES["Tracker"],
    "PositionSolver.solve": CREATES["PositionSolver"],
    "Aperture.report": (CREATES["Aperture"][0], lambda a: a.update([0], ROW[None], APER_CFG), lambda a: a.report([0])),
    # an extension's first use in a receiver bank: the object, its buffers and (Loran-C, FAX) the grown step-table slots
    "RxBank.fftext": (CREATES["RxBank"][0], prep_bank, bank_ext(tell_fftext, lambda b: [b.fftext_map(), b.fftext_rows()])),
    "RxBank.iqd": (CREATES["RxBank"][0], prep_bank, bank_ext(tell_iqd, lambda b: [b.iqd_rows(), b.iqd_status()])),
    "RxBank.lorc": (CREATES["RxBank"][0], prep_bank, bank_ext(tell_lorc, lambda b: b.lorc_rows())),
    "RxBank.fax": (CREATES["RxBank"][0], prep_bank, bank_ext(lambda b: b.fax_start(0), fax_flat)),
}


@pytest.mark.parametrize("name", list(GROWTHS))
def test_growth_survives_every_refused_allocation(monkeypatch, name):
    create, prepare, call = GROWTHS[name]
    gc.collect()
    live0 = live_allocs()

    def fresh():
        c = Context(0)
        o = create(c)
        if prepare:
            prepare(o)
        return c, o

    ctx, obj = fresh()
    first, refusals = refused_until_it_works(monkeypatch, lambda: call(obj), 64)
    print("%s: %d allocations, each refused once" % (name, refusals))
    assert refusals >= 1
    again = call(obj)                                   # the variable is gone: the same call on the same object
    obj.close()
    ctx.close()
    assert live_allocs() == live0
    ctx, obj = fresh()                                  # an object that never saw a refusal
    want = [as_bytes(call(obj)), as_bytes(call(obj))]
    obj.close()
    ctx.close()
    assert [as_bytes(first), as_bytes(again)] == want
    assert live_allocs() == live0
