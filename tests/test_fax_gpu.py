"""kg_fax on the device against tests/golden/fax_ref.npz (the reference's own statements, tools/make_ref_fax_golden.py): the lines every
block completed, every line's record, every row byte and the end state -- every scalar and array -- bit for bit, under seeded random
partitions of 1 to 64 blocks a push.  A script pushed a block at a time equals the same pushed at once; connections with different
scripts side by side in one push equal each alone; a refused command leaves the object as it was (the push on device-resident audio is
the receiver bank's: tests/test_fax_bank_gpu.py holds it to the host-array push).  The shapes: 240 lpm (3000 samples a line, the
detector's cap exactly), 120 lpm (the cap below the line), 60 lpm at 20250 Hz (the longest line), a push that ends one sample short of
a line, a skip larger than a block.  The largest push of the hand-written scripts holds 64 blocks (the 256 asked for `shift_mid` are cut
to 40 by its commands).

The seeded random scripts and the shape scripts of tests/ext_random.py go further: pushes of 1, 2, 7, 64 and 256 blocks (256 is the
most kg_fax_push takes), lines of 10 to 24576 samples -- exact multiples of the demodulator's chunk of 1024, a last chunk shorter than
the 16 carried products, lines shorter than them and than the workgroup, 2999 and 3001 around the detector's cap --, rate ratios of
exactly 0.5 (1024 picks a block, the pick walk's bound) and 2, an imagewidth of 1 and of the whole line; against the host model
(csrc/kg_fax.h through tools/fax_host_driver.cpp) in full and against tests/golden/fax_rand_ref.npz, the reference's record of the
same scripts.  Every comparison is an equality."""
import zlib

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, FaxDecoder, KiwiGpuError

from . import fax_common as fc
from .ext_random import shape_names

pytestmark = pytest.mark.gpu

NAMES = sorted(fc.scripts())
SIDE = ["shift_mid", "p0a0_debug", "all_zero", "restart_mid_line", "silence_then_signal", "one_short_240"]


@pytest.fixture(scope="module")
def golden():
    return fc.load()


@pytest.fixture(scope="module")
def pool():
    return fc.pool()


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def _cuts(seed, most=64):
    rng = np.random.Generator(np.random.PCG64(seed))
    return lambda: int(rng.integers(1, most + 1))


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_reference(golden, pool, ctx, name):
    q = FaxDecoder(ctx, nconn=2)
    got = fc.run_script_dev(q, fc.scripts()[name], pool, conn=1, cuts=_cuts(zlib.crc32(name.encode())))
    fc.check_against_golden(golden, name, got)
    assert got["calls"] >= 1
    q.close()


def test_a_push_of_k_blocks_equals_k_pushes_of_one(golden, pool, ctx):
    lines = fc.scripts()["shift_mid"]
    runs = []
    for cut in (1, 256):
        q = FaxDecoder(ctx, nconn=1)
        runs.append(fc.run_script_dev(q, lines, pool, cuts=lambda: cut))
        fc.check_against_golden(golden, "shift_mid", runs[-1])
        q.close()
    assert runs[0]["calls"] == 100 and runs[1]["calls"] == 3                     # the two shifts cut the blocks into three stretches
    assert np.array_equal(fc.all_bytes(runs[0]), fc.all_bytes(runs[1])) and runs[0]["recs"].tobytes() == runs[1]["recs"].tobytes()


def test_one_sample_short_of_a_line(golden, pool, ctx):
    """the first push ends with 2999 of 3000 samples in the line; the second completes it on its first sample"""
    lines = fc.scripts()["one_short_240"]
    sizes = iter([6, 1, 13])
    q = FaxDecoder(ctx, nconn=1)
    got = fc.run_script_dev(q, lines, pool, cuts=lambda: next(sizes))
    fc.check_against_golden(golden, "one_short_240", got)
    assert got["calls"] == 3 and got["nlines"][:6].sum() == 0 and got["nlines"][6] == 1 and got["recs"]["off"][0] == 1
    # and the state behind the first push alone
    q2 = FaxDecoder(ctx, nconn=1)
    fc.apply_command(q2, 0, lines[0], 0.0)
    fc.apply_command(q2, 0, lines[1], 0.0)
    offs = [int(l.split()[1]) for l in lines[2:8]]
    recs, rows = q2.push([0], np.stack([pool[o:o + fc.BLK] for o in offs])[None], [12000.0])
    assert recs[0].size == 0 and rows[0].shape[0] == 0 and q2.state(0)[0]["samp_idx"] == 2999 and q2.state(0)[0]["skip"] == 0
    q.close()
    q2.close()


def test_connections_side_by_side_equal_each_alone(golden, pool, ctx):
    """six scripts on six connections of one object, in lockstep: every round ONE push feeds every connection with blocks left, 1 to 24
    consecutive blocks each, listed out of connection order; each equals the reference, which is what it gives alone"""
    rng = np.random.Generator(np.random.PCG64(0xFA51DE))
    q = FaxDecoder(ctx, nconn=len(SIDE) + 1)
    got, _, shared = fc.run_side_by_side(q, [fc.scripts()[n] for n in SIDE], pool, rng)
    assert shared >= 5
    for c, name in enumerate(SIDE):
        fc.check_against_golden(golden, name, got[c])
    assert q.state(len(SIDE))[0]["spl"] == 0                                     # the idle connection is still the zeroed object
    q.close()


def test_a_refusal_changes_nothing_on_the_device(pool, ctx):
    q = FaxDecoder(ctx, nconn=1)
    q.start(0, lpm=120)
    x = pool[fc.AT["a120"]:fc.AT["a120"] + 20 * fc.BLK].reshape(1, 20, fc.BLK)
    q.push([0], x, [12000.0])
    before = [np.asarray(a).tobytes() for a in q.state(0)]
    for kw in (dict(lpm=0), dict(deviation=0), dict(bandwidth=3), dict(bandwidth=-1), dict(imagewidth=0), dict(imagewidth=6001), dict(lpm=29), dict(nom_rate=0.0),
               dict(srate=5999.0), dict(srate=float("nan"))):
        with pytest.raises(KiwiGpuError):
            q.start(0, **kw)
    for sh in (-0.25, 1.5, float("nan"), float("inf")):
        with pytest.raises(KiwiGpuError):
            q.set_shift(0, sh)
    with pytest.raises(KiwiGpuError):
        q.push([0], x, [24001.0])
    with pytest.raises(KiwiGpuError):
        q.push([0, 0], np.concatenate([x, x]), [12000.0, 12000.0])
    assert [np.asarray(a).tobytes() for a in q.state(0)] == before
    # a stopped connection takes nothing
    q.stop(0)
    recs, rows = q.push([0], x, [12000.0])
    assert recs[0].size == 0 and rows[0].shape[0] == 0
    after = q.state(0)
    assert after[0]["started"] == 0 and [np.asarray(a).tobytes() for a in after[1:]] == before[1:]
    q.close()


# ---- seeded random scripts and shape scripts (tests/ext_random.py): the device against the host model in full, and the fixture.  A
# script begins on a fresh object: what a restart carries over would otherwise come from the script before it.
PARTS = 4                                                                  # the 40 seeds, ten a test


@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("fax")


@pytest.fixture(scope="module")
def random_host(pool, tmp_path_factory):
    """k -> the host driver's result of seed k, or of shape script k - NSEED, sample by sample: made once when first asked for, shared,
    left unchanged"""
    from . import ext_random as er
    tmp = tmp_path_factory.mktemp("fax_random")
    driver, scripts, made = fc.build_driver(tmp), [er.fax_script(s) for s in range(er.NSEED)] + list(er.fax_shapes().values()), {}

    def host(k):
        if k not in made:
            made[k] = fc.run_script_exe(driver, scripts[k], pool, tmp)
        return made[k]
    return host


@pytest.mark.parametrize("part", range(PARTS))
def test_random_scripts_under_a_random_partition(ctx, random_ref, random_host, pool, part):
    """every seed's script with 1, 2, 7, 64 or 256 blocks a push (drawn push by push by a generator of its own) on one connection, and
    a block a push on another: both equal the host model in full, hence each other, and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    for seed in range(part * er.NSEED // PARTS, (part + 1) * er.NSEED // PARTS):
        lines = er.fax_script(seed)
        q = FaxDecoder(ctx, nconn=2)
        try:
            got = fc.run_script_dev(q, lines, pool, conn=0, cuts=ed.partition("fax", seed, fc.nblocks(lines)))
            each = fc.run_script_dev(q, lines, pool, conn=1, cuts=lambda: 1)
        finally:
            q.close()
        ed.fax_same(got, random_host(seed), "seed %d" % seed, "the partition")
        ed.fax_same(each, random_host(seed), "seed %d" % seed, "a push a block")
        assert each["calls"] == fc.nblocks(lines) >= got["calls"]
        er.check_record("fax", seed, lines, got, er.unpack(random_ref, seed))


@pytest.mark.parametrize("name", shape_names("fax"))
def test_shape_scripts(ctx, random_ref, random_host, pool, name):
    """a kernel-shape edge (ext_random.fax_shapes), once with up to 256 blocks a push and once with one: both equal the host model
    in full and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    k = er.NSEED + er.shape_names("fax").index(name)
    lines, runs = er.fax_shapes()[name], []
    for cut in (256, 1):
        q = FaxDecoder(ctx, nconn=1)
        try:
            runs.append(fc.run_script_dev(q, lines, pool, cuts=lambda: cut))
        finally:
            q.close()
        ed.fax_same(runs[-1], random_host(k), name, "%d blocks a push" % cut)
        er.check_record("fax", k, lines, runs[-1], er.unpack(random_ref, k))
    assert runs[1]["calls"] == fc.nblocks(lines) > runs[0]["calls"]

@pytest.mark.parametrize("group", range(14))
def test_random_scripts_side_by_side(ctx, random_ref, random_host, pool, group):
    """the seeds three at a time on three connections of one object, in lock step (fax_common.run_side_by_side, drawn from
    ext_random_dev.plan_rng): each connection equals the host model of its own script in full, and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    q = FaxDecoder(ctx, nconn=3)
    try:
        seeds, got, calls, shared = ed.side_by_side("fax", q, pool, group)
    finally:
        q.close()
    for seed, g in zip(seeds, got):
        ed.fax_same(g, random_host(seed), "seed %d of %s" % (seed, seeds))
        er.check_record("fax", seed, er.fax_script(seed), g, er.unpack(random_ref, seed))
    assert shared >= 1 and calls >= shared
