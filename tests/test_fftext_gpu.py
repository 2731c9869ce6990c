"""The FFT extension on the device (extensions/FFT/FFT.cpp; kg_fftext): kg_fftext_process_dev against every byte, bin and final sum
of the reference's scripts (tests/golden/fftext_ref.npz), the same bytes whatever the split of a script into calls, rows behind a real
kg_fir_process_taps_dev against the host model (csrc/kg_fftext.h through tools/fftext_host_driver.cpp) of the spectra that call
stored -- nothing is compared across transforms --, containment on guarded layouts, the limiter through the C ABI and the refusals."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, fftext, snd
from flydog_sdr_gps_amd._lib import check, ptr

from . import fftext_common as fc
from .guarded import contain

pytestmark = pytest.mark.gpu
PAD = 64
KG_ERR_INVALID, KG_ERR_STATE = -2, -5


@pytest.fixture(scope="module")
def golden():
    return fc.load()


@pytest.fixture(scope="module")
def pool():
    return fc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return fc.build_driver(tmp_path_factory.mktemp("fftext"))


@pytest.mark.parametrize("name", sorted(fc.scripts()))
def test_scripts_equal_the_reference(gpu_ctx, golden, pool, name):
    """every row byte, bin, taken / ignored / dropped block, ncma, fi, bins, both scales and all 200 x 1024 sums, with the blocks
    between two commands in ONE call; a padded row stride stays untouched"""
    fx = fftext.FftExt(gpu_ctx, nchan=1)
    try:
        got = fc.run_script_dev(fx, gpu_ctx, fc.scripts()[name], pool[1], row_stride=fc.W + PAD)
    finally:
        fx.close()
    fc.check_against_golden(golden, name, got)
    assert got["pad"], "bytes outside the rows were written"
    assert got["calls"] <= sum(1 for l in fc.scripts()[name] if l[0] != "B") + 1


@pytest.mark.parametrize("name", ["integ_bins3", "clear_itime_mid", "wf_to_integ"])
def test_any_split_into_calls_gives_the_same_bytes(gpu_ctx, golden, pool, name):
    """cut after every block in turn, and after all of them (one block a call): registers or memory, the sums are the same"""
    lines = fc.scripts()[name]
    nb = fc.nblocks(lines)
    fx = fftext.FftExt(gpu_ctx, nchan=1)
    try:
        for cuts in [{c} for c in range(1, nb)] + [set(range(1, nb))]:
            fx.restart(0)                                                  # a new connection: also zeroes the sums of the run before
            got = fc.run_script_dev(fx, gpu_ctx, lines, pool[1], cuts=cuts)
            fc.check_against_golden(golden, name, got)
    finally:
        fx.close()


def test_behind_the_fir_taps(gpu_ctx, driver, tmp_path):
    """five channels, several blocks an entry, two calls: each channel's rows and sums equal the host model of the filtered spectra
    that kg_fir_process_taps_dev stored for it"""
    ctx = gpu_ctx
    NCH, N, MAXBLK = 5, 1621, 4
    setup = [("I 0.1", "S 2 0 2"), (None, "S 0 0 2"), (None, "S 1 0 2"), ("I 0.05", "S 2 0 2"), (None, None)]      # channel 4: off
    chans = np.arange(NCH, dtype=np.int32)
    out_stride, tap_stride, row_stride = MAXBLK * 512, MAXBLK * 1024, fc.W + PAD
    F = snd.FastFir(ctx, nchan=NCH, max_in=2048)
    fx = fftext.FftExt(ctx, nchan=NCH, sample_rate=12000.0)
    d_in, d_out, d_post = ctx.alloc(NCH * N * 8), ctx.alloc(NCH * out_stride * 8), ctx.alloc(NCH * tap_stride * 8)
    d_rows = ctx.alloc(NCH * MAXBLK * row_stride)
    try:
        for ch in range(NCH):
            F.setup(ch, 300.0 - 100 * ch, 2700.0, 0.0, 12000.0)
            it, run = setup[ch]
            if it:
                fx.set_itime(ch, float(it[2:]))
            if run:
                fx.set_run(ch, int(run.split()[1]))
        rng = np.random.default_rng(0xFF7E)
        blocks = [[] for _ in range(NCH)]
        rows_got = [[] for _ in range(NCH)]
        bins_got = [[] for _ in range(NCH)]
        for call in range(2):
            x = (rng.standard_normal((NCH, N)) + 1j * rng.standard_normal((NCH, N))).astype(np.complex64) * np.float32(3000.0)
            ctx.upload(d_in, x)
            nout = np.zeros(NCH, np.int32)
            check(F.lib.kg_fir_process_taps_dev(F.h, ptr(chans), NCH, ptr(int(d_in)), N, N, ptr(int(d_out)), out_stride, ptr(nout), None,
                                                ptr(int(d_post)), tap_stride), "kg_fir_process_taps_dev")
            nblk = nout // 512
            assert nblk.min() >= 3
            fill = np.full((NCH * MAXBLK, row_stride), 0x5A, np.uint8)
            ctx.upload(d_rows, fill)
            m = fx.process_dev(chans, nblk, [fc.PASSBAND] * NCH, d_post, tap_stride, d_rows, row_stride, NCH * MAXBLK)
            ctx.sync()
            post = np.zeros((NCH, tap_stride), np.complex64)
            ctx.download(d_post, post)
            ctx.download(d_rows, fill)
            assert m.shape[0] == int(nblk[:4].sum()) and (fill[m.shape[0]:] == 0x5A).all() and (fill[:, fc.W:] == 0x5A).all()
            want_map = [(ch, ch, b) for ch in range(4) for b in range(int(nblk[ch]))]       # rows in list order, then block order
            assert [tuple(r[:3]) for r in m.tolist()] == want_map
            for r, (ch, ent, blk, b) in enumerate(m.tolist()):
                rows_got[ch].append(fill[r, :fc.W].copy())
                bins_got[ch].append(b)
            for ch in range(NCH):
                blocks[ch] += [post[ch, 1024 * b:1024 * (b + 1)] for b in range(int(nblk[ch]))]
        for ch in range(4):
            it, run = setup[ch]
            lines = ["R 12000"] + ([it] if it else []) + [run] + ["B 0 %d" % k for k in range(len(blocks[ch]))]
            want = fc.run_script_exe(driver, lines, np.stack(blocks[ch]), tmp_path)
            assert want["sent"].all() and np.array_equal(want["bins"], np.array(bins_got[ch])), (ch, want["bins"], bins_got[ch])
            have = np.stack(rows_got[ch])
            bad = np.argwhere(have != want["rows"])
            assert bad.size == 0, (ch, "first differing byte (row, column)", bad[0], int(have[tuple(bad[0])]), int(want["rows"][tuple(bad[0])]))
            info, ncma, pwr = fx.state(ch, sums=True)
            assert np.array_equal(pwr.view(np.uint32), want["pwr"].view(np.uint32)) and np.array_equal(ncma, want["ncma"]), ch
            assert (float(info["fi"]), int(info["bins"])) == (want["fi"], want["nbins"]), ch
            assert want["rows"].min() >= 55 and len(np.unique(want["rows"])) > 20          # a real spectrum, not a constant row
        assert len(set(bins_got[0])) >= 2 and len(set(bins_got[3])) >= 1 and max(np.bincount(bins_got[0])) >= 2
        info, ncma, pwr = fx.state(4, sums=True)
        assert int(info["run"]) == fc.OFF and not pwr.any() and not ncma.any()
    finally:
        for d in (d_in, d_out, d_post, d_rows):
            ctx.free(d)
        fx.close()
        F.close()


def test_containment(gpu_ctx, pool):
    """strided spectra and rows between guard bands, fills 0x00 and 0xFF: no byte outside the rows is written, none outside the listed
    blocks is read; three entries of two channels, the channel-null one ignored"""
    spec = pool[1]
    ent = [np.ascontiguousarray(spec[[4, 5, 6]]), np.ascontiguousarray(spec[[7, 1]]), np.ascontiguousarray(spec[[0, 8, 2]])]
    chans, inst, nblk = [1, 0, 1], [fc.PASSBAND, fc.CHAN_NULL, fc.PASSBAND], [3, 2, 3]
    MAXR = 8

    def case(lay):
        fx = fftext.FftExt(gpu_ctx, nchan=2, sample_rate=20250.0)
        try:
            fx.set_itime(1, 0.06)
            fx.set_run(1, fc.INTEG)
            fx.set_run(0, fc.WF)
            g_in, s_in = lay.inp([e.reshape(-1) for e in ent], 8)
            g_rows, s_rows = lay.out(MAXR, 1024, 1, 4, mult=4)
            m = fx.process_dev(chans, nblk, inst, g_in.ptr, s_in, g_rows.ptr, s_rows, MAXR)
            gpu_ctx.sync()
            rows = lay.take(g_rows, [1024] * m.shape[0] + [0] * (MAXR - m.shape[0]))
            _, ncma, pwr = fx.state(1, sums=True)
            return rows, m, ncma, pwr
        finally:
            fx.close()

    rows, m, ncma, pwr = contain(gpu_ctx, case)
    m = np.frombuffer(m[2], np.int32).reshape(-1, 4)
    assert m[:, :3].tolist() == [[1, 0, 0], [1, 0, 1], [1, 0, 2], [1, 2, 0], [1, 2, 1], [1, 2, 2]] and m[:, 3].max() >= 1


def test_limiter_through_the_abi(gpu_ctx, golden):
    fx = fftext.FftExt(gpu_ctx, nchan=2)
    try:
        for k, clocks in fc.limiter_scripts().items():
            fx.set_run(1, fc.SPEC)                                         # the command zeroes last_ms
            for i, c in enumerate(clocks):
                assert int(fx.due(1, c)) == int(golden["limiter_%s_sent" % k][i]), (k, i)
                assert int(fx.state(1)[0]["last_ms"]) == int(golden["limiter_%s_last" % k][i]), (k, i)
        for run in (fc.WF, fc.INTEG):                                      # only spec is limited
            fx.set_run(0, run)
            assert all(fx.due(0, c) for c in (0, 1, 50, 99, 100, 101))
    finally:
        fx.close()


def test_refusals_change_nothing(gpu_ctx, pool):
    ctx, spec = gpu_ctx, np.ascontiguousarray(pool[1][[4, 5, 6]])
    fx = fftext.FftExt(ctx, nchan=2)
    d_spec, d_rows = ctx.alloc(spec.nbytes), ctx.alloc(4 * 1024)
    try:
        ctx.upload(d_spec, spec)
        fill = np.full(4 * 1024, 0xC3, np.uint8)
        ctx.upload(d_rows, fill)
        call = lambda **kw: fx.process_dev(kw.get("chans", [0]), kw.get("nblk", [3]), kw.get("inst", [0]), kw.get("d_spec", d_spec), 3 * 1024,
                                           kw.get("d_rows", d_rows), kw.get("row_stride", 1024), kw.get("max_rows", 4))

        def refused(status, before=None, **kw):
            before = before or fx.state(0)
            with pytest.raises(KiwiGpuError) as e:
                call(**kw)
            assert e.value.status == status, e.value
            after = fx.state(0)
            assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])
            got = np.zeros_like(fill)
            ctx.sync()
            ctx.download(d_rows, got)
            assert np.array_equal(got, fill), "a refused call wrote rows"

        with pytest.raises(KiwiGpuError) as e:
            fx.set_run(0, 3)
        assert e.value.status == KG_ERR_INVALID
        for bad in (0.0, -12000.0, float("nan"), float("inf")):
            with pytest.raises(KiwiGpuError) as e:
                fx.set_rate(bad)
            assert e.value.status == KG_ERR_INVALID
        assert call().shape[0] == 0                                        # off: nothing taken, nothing refused
        fx.set_run(0, fc.INTEG)
        fx.clear(0)
        refused(KG_ERR_STATE)                                              # a latched reset and no rate
        fx.set_rate(12000.0)
        refused(KG_ERR_STATE)                                              # integ while time is the never-set 0
        for t in (-1.0, float("nan"), float("inf"), 2.0 ** 31 * fc.FFT_SEC[12000] + 100):
            fx.set_itime(0, t)
            refused(KG_ERR_STATE)
        fx.set_itime(0, 0.13)
        refused(KG_ERR_INVALID, max_rows=2)                                # three rows do not fit
        refused(KG_ERR_INVALID, chans=[2])
        refused(KG_ERR_INVALID, inst=[2])
        refused(KG_ERR_INVALID, nblk=[-1])
        refused(KG_ERR_INVALID, d_spec=d_spec + 4)
        refused(KG_ERR_INVALID, d_rows=d_rows + 2)
        refused(KG_ERR_INVALID, row_stride=1022)
        assert call(chans=[0, 1], nblk=[3, 0], inst=[0, 0]).tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 2, 1]]      # then it runs; channel 1 is off
        assert fx.state(0)[1][:3].tolist() == [2, 1, 0]
    finally:
        ctx.free(d_spec)
        ctx.free(d_rows)
        fx.close()


def test_host_array_twin(gpu_ctx, golden, pool):
    """kg_fftext_process: the wf script's first rows from host memory"""
    fx = fftext.FftExt(gpu_ctx, nchan=1, sample_rate=12000.0)
    try:
        fx.set_run(0, fc.WF)
        rows, m = fx.process([0], pool[1][None, :5], [fc.PASSBAND])
        assert np.array_equal(rows, golden["s_wf_rows"][:5]) and m.tolist() == [[0, 0, b, 0] for b in range(5)]
    finally:
        fx.close()


# ---- seeded random scripts (tests/ext_random.py) under random call partitions: the device against the host model, in full
PARTS = 4                                                                  # the 40 seeds, ten a test


@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er, ext_random_dev as ed
    return er.load("fftext")


@pytest.fixture(scope="module")
def random_host(driver, pool, tmp_path_factory):
    """the host driver's result of every seed: made once, shared, left unchanged"""
    from . import ext_random as er, ext_random_dev as ed
    tmp = tmp_path_factory.mktemp("fftext_random")
    return [fc.run_script_exe(driver, er.fftext_script(seed), pool[1], tmp) for seed in range(er.NSEED)]


@pytest.mark.parametrize("part", range(PARTS))
def test_random_scripts_under_a_random_partition(gpu_ctx, random_ref, random_host, pool, part):
    """every seed's script cut into calls by a generator of its own (cuts, entries merged or not), and again a call a block: both equal
    the host model in every row byte, bin, taken / ignored / dropped block and the whole end state with all 200 x 1024 sums, hence
    each other, and the fixture's digests"""
    from . import ext_random as er, ext_random_dev as ed
    for seed in range(part * er.NSEED // PARTS, (part + 1) * er.NSEED // PARTS):
        lines = er.fftext_script(seed)
        nb = fc.nblocks(lines)
        cuts, merge = ed.partition("fftext", seed, nb)
        fx = fftext.FftExt(gpu_ctx, nchan=1)
        try:
            got = fc.run_script_dev(fx, gpu_ctx, lines, pool[1], cuts=cuts, merge=merge, row_stride=fc.W + PAD)
            fx.restart(0)                                                  # a new connection: also zeroes the sums of the run before
            each = fc.run_script_dev(fx, gpu_ctx, lines, pool[1], cuts=set(range(1, nb)))
        finally:
            fx.close()
        ed.fftext_same(got, random_host[seed], "seed %d" % seed, "cuts %s, merge %s" % (sorted(cuts), merge))
        ed.fftext_same(each, random_host[seed], "seed %d" % seed, "a call a block")
        assert got["pad"] and each["pad"] and each["calls"] >= got["calls"]
        er.check_record("fftext", seed, lines, got, er.unpack(random_ref, seed))


def _side_by_side(gpu_ctx, random_ref, random_host, pool, group, resident):
    from . import ext_random as er, ext_random_dev as ed
    seeds, scripts, steps, rng = ed.planned("fftext", group, resident)
    chans = [2, 0, 1]                                                      # not in channel order
    fx = fftext.FftExt(gpu_ctx, nchan=3)
    try:
        got, calls, shared = ed.fftext_run_plan(fx, gpu_ctx, steps, chans, scripts, pool[1], resident=resident, rng=rng)
    finally:
        fx.close()
    for seed, lines, g in zip(seeds, scripts, got):
        ed.fftext_same(g, random_host[seed], "seed %d of %s" % (seed, seeds), "channel %d" % chans[seeds.index(seed)])
        er.check_record("fftext", seed, lines, g, er.unpack(random_ref, seed))
    # the calls were the plan's: tests/test_fftext_cpu.py::test_random_side_by_side_plans_share_their_calls holds the plans to their share
    assert (calls, shared) == ed.calls_of(steps)[:2] and shared >= 1


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_side_by_side(gpu_ctx, random_ref, random_host, pool, group):
    """the seeds three at a time on three channels of one object, out of order: every call carries every channel whose script stands at
    the round's sample rate (the object's, taken up at a channel's reset), a random number of blocks each, their entries shuffled into
    each other; the commands go between the calls.  Each channel equals the host model of its own script in full, and the fixture"""
    _side_by_side(gpu_ctx, random_ref, random_host, pool, group, False)


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_from_device_resident_input(gpu_ctx, random_ref, random_host, pool, group):
    """the same from ONE device buffer that holds every call's spectra, uploaded ahead of the first call: an entry's spectra stand at a
    stride larger than its blocks and -- entries of no block between them -- not at the row of its position among the entries that
    have some; the buffer is NaN outside the blocks.  A gap: the row list itself (spec_row of kg_fftext_process_rows_) is the bank's,
    not part of the ABI, so here every entry still reads row i of its list, and the spec_row[i] branch of the host walk stays with
    tests/test_fftext_bank_gpu.py"""
    _side_by_side(gpu_ctx, random_ref, random_host, pool, group, True)
