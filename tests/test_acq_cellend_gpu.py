"""GPU parity of the C/A correlator's cell boundary (acq_correlate_kernel leaves four wave records per cell and crosses the
boundary without a barrier; the index of the cell three ahead is claimed at the top of a cell and crosses the workgroup
through two LDS slots; acq_select_kernel merges the records, divides and writes cells[]) against the CPU oracle, on walks
long enough for every workgroup to use its three static cells and claimed ones, at every count of cells per XCD group at
which another of a workgroup's cells is the first that does not exist, on the spread walk, on windows that end inside the
first row, launch after launch without a synchronisation, with both kinds of pair in one launch, and at P = 16.

Bars as tests/test_acq_horner_gpu.py: every cell's peak index, the winning Doppler bin and `valid` equal; snr, max_pwr and
tot_pwr within 1e-5 relative."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Searcher, acq, prn, sats, synth
from flydog_sdr_gps_amd._lib import check as kg_check, ptr
from tests.fixtures import e1b_chips, oracle_next_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N10, FFT10 = acq.NSAMPLES_10MS, acq.FFT_LEN_10MS
NB, NSV = 8, 8                      # the deep walk: 8 blocks x 8 SVs x 41 bins = 2624 cells, 328 per XCD group


def ca(sat):
    _, t1, t2, _ = sats.SATS[sat]
    return prn.cacode(t1, t2)


def check(res, cells, want, wcells, tag):
    assert np.array_equal(cells["idx"], wcells["idx"]), tag
    assert np.array_equal(res["dop"], want["dop"]), tag
    assert np.array_equal(res["idx"], want["idx"]), tag
    assert np.array_equal(res["valid"], want["valid"]), tag
    for k in ("snr", "max_pwr", "tot_pwr"):
        err = float(np.max(np.abs(cells[k] - wcells[k]) / np.abs(wcells[k])))
        print("%s: %s max rel err %.3g" % (tag, k, err))
    np.testing.assert_allclose(res["snr"], want["snr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["snr"], wcells["snr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["max_pwr"], wcells["max_pwr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["tot_pwr"], wcells["tot_pwr"], rtol=RTOL, err_msg=tag)


def launch_grid(s, sv):
    """Workgroups of the C/A correlator's persistent grid, read from a launch: the diagnostic instantiation stamps every
    workgroup's start (kg_acq_debug_corr_stamps, slots 512 + 4 b)."""
    cs = np.zeros(512 + 4 * 1024, np.uint64)
    svs = np.asarray([sv], np.int32)
    kg_check(s.lib.kg_acq_debug_corr_stamps(s.h, 1, ptr(svs), 1, ptr(cs), cs.size), "kg_acq_debug_corr_stamps")
    return int(np.count_nonzero(cs[512::4]))


@pytest.fixture(scope="module")
def scenes(oracle):
    """Eight distinct blocks (one or two injected SVs each) and the codes of SVs 0..7, with the oracle's spectra of both;
    computed once, read-only."""
    sc = []
    for b in range(NB):
        one = [(ca(b), 50.25 + 37.0 * b, -4000.0 + 1100.0 * b, 0.3 + 0.4 * b)]
        if b & 1:
            one.append((ca((b + 3) % NSV), 900.5 - 61.0 * b, 2600.0 - 700.0 * b, 1.1 * b))
        sc.append(one)
    bits = [synth.gps_scene_bits(one, seed=41 + b) for b, one in enumerate(sc)]
    data = [oracle.sample_bits(x) for x in bits]
    codes = np.stack([oracle.code_fft(ca(sat)) for sat in range(NSV)])
    for a in data + [codes]:
        a.setflags(write=False)
    return {"bits": bits, "data": data, "codes": codes}


def new_searcher(ctx, scenes, nblocks, lo, hi, svs=range(NSV), limits=None):
    s = Searcher(ctx, max_sats=NSV, max_blocks=nblocks, dop_lo=lo, dop_hi=hi)
    for k, sat in enumerate(svs):
        s.set_code(sat, ca(sat), limit=None if limits is None else limits[k])
    for b in range(nblocks):
        s.sample(scenes["bits"][b], block=b)
    return s


def oracle_blocks(oracle, scenes, s, svs, blocks, lo, hi, limits=None):
    svs = list(svs)
    limits = [sats.L1_LIMIT] * len(svs) if limits is None else limits
    nexts = oracle_next_rows(oracle, s, svs)
    return [oracle.correlate_many(scenes["codes"][svs], scenes["data"][b], limits, dop_lo=lo, dop_hi=hi, nthreads=4,
                                  nexts=nexts) for b in blocks]


@pytest.fixture(scope="module")
def deep_want(gpu_ctx, oracle, scenes):
    """The oracle's 2624 cells of the deep walk, computed once."""
    s = new_searcher(gpu_ctx, scenes, 1, acq.DOP_LO, acq.DOP_HI)
    try:
        return oracle_blocks(oracle, scenes, s, range(NSV), range(NB), acq.DOP_LO, acq.DOP_HI)
    finally:
        s.close()


@pytest.fixture(scope="module")
def grid(gpu_ctx, scenes):
    s = new_searcher(gpu_ctx, scenes, 1, 0, 0, svs=[0])
    try:
        g = launch_grid(s, 0)
    finally:
        s.close()
    assert g >= 8 and g % 8 == 0
    return g


def check_deep(res, cells, deep_want, tag):
    for b in range(NB):
        check(res[b], cells[b], deep_want[b][0], deep_want[b][1], "%s, block %d" % (tag, b))


def test_deep_walk(gpu_ctx, scenes, deep_want, grid):
    """Five to six cells per workgroup: the three static cells and claimed ones, all 2624 cells checked."""
    s = new_searcher(gpu_ctx, scenes, NB, acq.DOP_LO, acq.DOP_HI)
    try:
        print("grid %d workgroups, %.1f cells per workgroup" % (grid, NB * NSV * s.ndop / grid))
        res, cells = s.correlate_many(list(range(NSV)), nblocks=NB)
        check_deep(res, cells, deep_want, "deep")
        hit = [(b, int(res[b, b]["dop"])) for b in range(NB) if res[b, b]["snr"] >= 16]
        assert len(hit) == NB, hit                             # every block's own SV is found
    finally:
        s.close()


def test_deep_walk_one_workgroup_per_cu(gpu_ctx, scenes, deep_want, grid, monkeypatch):
    """The same launch on half the grid (the library's A/B switch, read when the Searcher is created): twice the cells per
    workgroup."""
    monkeypatch.setenv("KIWIGPU_TUNING", "1")
    monkeypatch.setenv("KIWIGPU_ACQ_WGS_PER_CU", "1")
    s = new_searcher(gpu_ctx, scenes, NB, acq.DOP_LO, acq.DOP_HI)
    try:
        half = launch_grid(s, 0)
        print("grid %d -> %d workgroups" % (grid, half))
        assert half < grid and half >= grid // 2 - 7
        res, cells = s.correlate_many(list(range(NSV)), nblocks=NB)
        check_deep(res, cells, deep_want, "deep, one workgroup per CU")
    finally:
        s.close()


def group_shape(cells_per_group):
    """(blocks g, Doppler bins) of a launch of g x 8 pairs -- g pairs and g x bins cells in every XCD group -- whose cells per
    group are the count asked for, or the nearest count such a launch reaches."""
    for g in range(NB, 0, -1):
        if cells_per_group % g == 0 and cells_per_group // g <= 201:
            return g, cells_per_group // g
    g = min(NB, -(-cells_per_group // 201))
    return g, max(1, int(round(cells_per_group / g)))


@pytest.mark.parametrize("which", ["1", "n-1", "n", "n+1", "2n+1", "3n+1"])
def test_static_cell_boundaries(gpu_ctx, oracle, scenes, grid, which):
    """Cells per XCD group around the counts at which a workgroup's second static cell, its third or its first claimed one is
    the first that does not exist; n = the workgroups of a group, read from the launch."""
    n = grid // 8
    target = {"1": 1, "n-1": n - 1, "n": n, "n+1": n + 1, "2n+1": 2 * n + 1, "3n+1": 3 * n + 1}[which]
    g, ndop = group_shape(max(target, 1))
    print("n = %d: asked for %d cells per group, launch of %d blocks x 8 SVs x %d bins = %d per group"
          % (n, target, g, ndop, g * ndop))
    lo = -(ndop // 2)
    hi = lo + ndop - 1
    s = new_searcher(gpu_ctx, scenes, g, lo, hi)
    try:
        res, cells = s.correlate_many(list(range(NSV)), nblocks=g)
        want = oracle_blocks(oracle, scenes, s, range(NSV), range(g), lo, hi)
        for b in range(g):
            check(res[b], cells[b], want[b][0], want[b][1], "%s cells per group, block %d" % (which, b))
    finally:
        s.close()


@pytest.mark.parametrize("npairs,ndop", [(1, 1), (2, 3), (7, 12)])
def test_spread_walk(gpu_ctx, oracle, scenes, npairs, ndop):
    """Fewer than eight pairs: the cells are dealt round-robin; with one cell every other workgroup exits at once."""
    lo = -(ndop // 2)
    hi = lo + ndop - 1
    svs = list(range(npairs))
    s = new_searcher(gpu_ctx, scenes, 1, lo, hi, svs=svs)
    try:
        res, cells = s.correlate_many(svs)
        (want, wcells), = oracle_blocks(oracle, scenes, s, svs, [0], lo, hi)
        check(res[0], cells[0], want, wcells, "spread %d x %d" % (npairs, ndop))
    finally:
        s.close()


def test_windows(gpu_ctx, oracle):
    """Nine pairs, windows of 4092 / 4096 / 1000 lags and of 1 / 256 / 257 lags: the divisions by the window now live in the
    select kernel.  The SV with the one-lag window is injected at lag 0 in every block: one lag's power is held to 1e-5
    relative only where it is not the residue of a cancellation."""
    lo, hi = -2, 2
    svs = [0, 1, 2]
    codes = np.stack([oracle.code_fft(ca(sat)) for sat in svs])
    sc = [[(ca(0), 0.0, 100.0, 0.3, 52.0), (ca(1), 30.25, -300.0, 1.0)],
          [(ca(0), 0.0, -150.0, 1.3, 52.0), (ca(2), 63.5, 400.0, 2.0)],
          [(ca(0), 0.0, 60.0, 2.3, 52.0), (ca(1), 10.0, -500.0, 0.7)]]
    allbits = [synth.gps_scene_bits(one, seed=61 + b) for b, one in enumerate(sc)]
    data = [oracle.sample_bits(bits) for bits in allbits]
    s = Searcher(gpu_ctx, max_sats=4, max_blocks=3, dop_lo=lo, dop_hi=hi)
    try:
        for limits in ([4092, 4096, 1000], [1, 256, 257]):
            for sat, limit in zip(svs, limits):
                s.set_code(sat, ca(sat), limit=limit)
            for b, bits in enumerate(allbits):
                s.sample(bits, block=b)
            res, cells = s.correlate_many(svs, nblocks=3)
            nexts = oracle_next_rows(oracle, s, svs)
            for b in range(3):
                want, wcells = oracle.correlate_many(codes, data[b], limits, dop_lo=lo, dop_hi=hi, nthreads=4, nexts=nexts)
                check(res[b], cells[b], want, wcells, "windows %s, block %d" % (limits, b))
                assert np.all(cells[b]["idx"] < np.asarray(limits)[:, None])
    finally:
        s.close()


def test_launch_after_launch(gpu_ctx, scenes, deep_want):
    """A deep launch and at once, with no synchronisation, a small one with another SV list, first_block != 0 and other data;
    then the deep one again: stale wave records, stale claim slots or counters not reset would show in one of the three."""
    s = new_searcher(gpu_ctx, scenes, NB, acq.DOP_LO, acq.DOP_HI)
    try:
        deep, small, first = list(range(NSV)), [3, 1], 5
        res, cells = s.correlate_many(deep, nblocks=NB)
        check_deep(res, cells, deep_want, "deep, first")
        s.correlate_async(deep, nblocks=NB)
        res, cells = s.correlate_many(small, nblocks=2, first_block=first)
        for k in range(2):
            want, wcells = deep_want[first + k]
            check(res[k], cells[k], want[small], wcells[small], "small behind deep, block %d" % (first + k))
        res, cells = s.correlate_many(deep, nblocks=NB)
        check_deep(res, cells, deep_want, "deep, again")
    finally:
        s.close()


def test_mixed_list(gpu_ctx, oracle, scenes):
    """Two C/A SVs and one E1B SV in one launch: the select kernel finishes the cells of the former and only reads the
    latter's."""
    lo, hi = -5, 6
    e1b = e1b_chips()[11]
    s = Searcher(gpu_ctx, max_sats=4, dop_lo=lo, dop_hi=hi)
    try:
        s.set_code(0, ca(0))
        s.set_code(1, e1b, boc=True)
        s.set_code(2, ca(2))
        bits = synth.gps_scene_bits([(ca(0), 100.25, 700.0, 0.3), (e1b, 2000.5, -500.0, 1.0, 45.0, True)], seed=71)
        s.sample(bits)
        svs = [0, 1, 2]
        res, cells = s.correlate_many(svs)
        codes = np.stack([oracle.code_fft(ca(0)), oracle.code_fft(e1b, boc=True), oracle.code_fft(ca(2))])
        want, wcells = oracle.correlate_many(codes, oracle.sample_bits(bits), [sats.L1_LIMIT, sats.E1B_LIMIT, sats.L1_LIMIT],
                                             dop_lo=lo, dop_hi=hi, nthreads=4, nexts=oracle_next_rows(oracle, s, svs))
        check(res[0], cells[0], want, wcells, "mixed C/A + E1B")
        assert res[0, 0]["snr"] >= 16 > res[0, 2]["snr"]
    finally:
        s.close()


@pytest.mark.parametrize("nblocks,nsv", [(1, 2), (3, 3)])
def test_p16(gpu_ctx, oracle, nblocks, nsv):
    """10 ms / 65536 points, dop -9..8: thirty-two barriers between a claim slot's store and its loads; two pairs walk
    spread, nine grouped."""
    lo, hi = -9, 8
    svs = list(range(nsv))
    s = Searcher(gpu_ctx, max_sats=4, max_blocks=nblocks, dop_lo=lo, dop_hi=hi, nsamples=N10, fft_len=FFT10)
    try:
        for sat in svs:
            s.set_code(sat, ca(sat))
        allbits = [synth.gps_scene_bits([(ca(b % nsv), 100.25 + 50 * b, 250.0 - 200.0 * b, 0.3)], seed=81 + b, n=N10)
                   for b in range(nblocks)]
        for b, bits in enumerate(allbits):
            s.sample(bits, block=b)
        res, cells = s.correlate_many(svs, nblocks=nblocks)
        codes = np.stack([oracle.code_fft(ca(sat), fft_len=FFT10) for sat in svs])
        nexts = oracle_next_rows(oracle, s, svs)
        for b, bits in enumerate(allbits):
            data = oracle.sample_bits(bits, nsamples=N10, fft_len=FFT10)
            want, wcells = oracle.correlate_many(codes, data, [sats.L1_LIMIT] * nsv, dop_lo=lo, dop_hi=hi, nthreads=4, nexts=nexts)
            check(res[b], cells[b], want, wcells, "P=16 %d x %d, block %d" % (nblocks, nsv, b))
    finally:
        s.close()
