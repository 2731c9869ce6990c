"""kg_cw on the device against tests/golden/cw_ref.npz (the reference's own statements, tools/make_ref_cw_golden.py): the events of every
sound block, every event's fields and the end state -- every scalar, the ring, data[] and the sample buffer -- bit for bit, under seeded
random partitions of 1 to 64 blocks a push.  A push of 7 blocks (which straddles Goertzel blocks: 512 is no multiple of 88) equals 7
pushes of one; four connections with different scripts side by side in one push equal each alone; a pboff between two pushes lands in
mid Goertzel block; a refused command leaves the object as it was; one connection with one block gives 5 Goertzel blocks and carries 72
samples.  The largest push of the hand-written scripts holds 40 blocks (233 Goertzel blocks): their N lines, the clock, cut every
stretch of blocks, so phase A's loop over the Goertzel blocks of a push takes one turn there.

The seeded random scripts and the shape scripts of tests/ext_random.py go further: pushes of 1, 2, 7, 64 and 256 blocks (256 is the
most kg_cw_push takes: 1489 or 1490 Goertzel blocks, six turns of that loop and the whole of its magnitudes), training intervals of 1
and 255, nominal rates of 88 and 1000, ratios of 0.5 and 2, thresholds of 0 and below, a clock that jumps backwards or passes 2^32;
against the host model (csrc/kg_cw.h through tools/cw_host_driver.cpp) in full and against tests/golden/cw_rand_ref.npz, the
reference's record of the same scripts.  Every comparison is an equality."""
import zlib

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, CwDecoder, KiwiGpuError

from . import cw_common as cc
from .ext_random import shape_names

pytestmark = pytest.mark.gpu

NAMES = sorted(cc.scripts())
SIDE = ["gaps", "glitch_dropped", "restart_mid", "auto_threshold"]


@pytest.fixture(scope="module")
def golden():
    return cc.load()


@pytest.fixture(scope="module")
def pool():
    return cc.pool()


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def _cuts(seed, most=64):
    rng = np.random.Generator(np.random.PCG64(seed))
    return lambda: int(rng.integers(1, most + 1))


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_reference(golden, pool, ctx, name):
    q = CwDecoder(ctx, nconn=2)
    got = cc.run_script_dev(q, cc.scripts()[name], pool, conn=1, cuts=_cuts(zlib.crc32(name.encode())))
    cc.check_against_golden(golden, name, got)
    assert got["calls"] >= 5 and q.state(0)["blocksize"] == 0                      # the idle connection is still the zeroed object
    q.close()


def test_a_push_of_7_blocks_equals_7_pushes_of_one(golden, pool, ctx):
    lines = cc.scripts()["jitter_25"]
    runs = []
    for cut in (1, 7):
        q = CwDecoder(ctx, nconn=1)
        runs.append(cc.run_script_dev(q, lines, pool, cuts=lambda: cut))
        cc.check_against_golden(golden, "jitter_25", runs[-1])
        q.close()
    assert runs[0]["calls"] == cc.nblocks(lines) and runs[1]["calls"] < runs[0]["calls"] // 4
    assert runs[0]["evs"].tobytes() == runs[1]["evs"].tobytes() and runs[0]["info"].tobytes() == runs[1]["info"].tobytes()


def test_minimal_shape_one_connection_one_block(golden, pool, ctx):
    """512 samples: 5 Goertzel blocks and 72 samples carried; the second block completes the sixth with 16 of its own"""
    lines = cc.scripts()["clean_fixed"]
    q = CwDecoder(ctx, nconn=1)
    now = 0
    for l in lines[:lines.index(next(x for x in lines if x[0] == "B"))]:
        now = cc.apply_command(q, 0, l, now)
    offs = [int(l.split()[1]) for l in lines if l[0] == "B"][:2]
    want = np.frombuffer(np.ascontiguousarray(golden["s_clean_fixed_evs"]).tobytes(), cc.ev_dtype)
    nev = golden["s_clean_fixed_nev"]
    ev = q.push([0], pool[offs[0]:offs[0] + cc.BLK].reshape(1, 1, cc.BLK), [now])[0]
    st = q.state(0)
    assert ev.tobytes() == want[:nev[0]].tobytes() and ev["gblk"].max() == 4 and st["sample_counter"] == 72 and st["slowdown"] == 5 % 3
    assert np.array_equal(st["raw"][:72], pool[offs[0] + 440:offs[0] + 512].astype(np.float32) / 4) and np.array_equal(
        st["raw"][72:], pool[offs[0] + 424:offs[0] + 440].astype(np.float32) / 4)
    ev = q.push([0], pool[offs[1]:offs[1] + cc.BLK].reshape(1, 1, cc.BLK), [now])[0]
    w2 = want[nev[0]:nev[0] + nev[1]].copy()
    w2["blk"] = 0
    assert ev.tobytes() == w2.tobytes() and ev["gblk"].max() == 5 and q.state(0)["sample_counter"] == (1024 % 88)
    q.close()


def test_a_pboff_between_two_pushes_lands_in_mid_goertzel_block(golden, pool, ctx):
    """the reference runs the Goertzel over the whole buffered block when its last sample arrives: the new coefficients hold for the 64
    samples that were waiting"""
    lines = cc.scripts()["pboff_mid"]
    q = CwDecoder(ctx, nconn=1)
    got = cc.run_script_dev(q, lines, pool, cuts=lambda: 256)
    cc.check_against_golden(golden, "pboff_mid", got)
    at = [i for i, l in enumerate(lines) if l[0] == "P"]
    assert len(at) == 3 and (cc.nblocks(lines[:at[1]]) * cc.BLK) % cc.GBLK == 64 and (cc.nblocks(lines[:at[2]]) * cc.BLK) % cc.GBLK != 0
    q.close()


def test_connections_side_by_side_equal_each_alone(golden, pool, ctx):
    """four scripts on four connections of one object, in lockstep: every round ONE push feeds every connection with blocks left, 1 to
    24 consecutive blocks each under its own now_sec, listed out of connection order; each equals the reference, which is what it gives
    alone"""
    rng = np.random.Generator(np.random.PCG64(0xC351DE))
    q = CwDecoder(ctx, nconn=len(SIDE) + 1)
    got, _, shared = cc.run_side_by_side(q, [cc.scripts()[n] for n in SIDE], pool, rng)
    assert shared >= 10
    for c, name in enumerate(SIDE):
        cc.check_against_golden(golden, name, got[c])
    assert q.state(len(SIDE))["blocksize"] == 0 and q.state(len(SIDE))["slowdown"] == 0
    q.close()


def test_a_refusal_changes_nothing_on_the_device(pool, ctx):
    q = CwDecoder(ctx, nconn=2)
    q.start(0, 40)
    q.set_pboff(0, cc.PBOFF)
    q.set_threshold(0, 20000)
    x = pool[cc.AT["clean"]:cc.AT["clean"] + 20 * cc.BLK].reshape(1, 20, cc.BLK)
    assert len(q.push([0], x, [100])[0]) >= 38
    before = q.state(0).tobytes()
    for conn in (-1, 2):
        for call in (lambda: q.start(conn, 40), lambda: q.set_pboff(conn, 818), lambda: q.set_wsc(conn, 0), lambda: q.set_threshold(conn, 1),
                     lambda: q.set_auto_threshold(conn, 1), lambda: q.set_wpm(conn, 30, 40), lambda: q.stop(conn), lambda: q.state(conn)):
            with pytest.raises(KiwiGpuError):
                call()
    for kw in (dict(training_interval=0), dict(training_interval=256), dict(nom_rate=87.0), dict(nom_rate=1000001.0), dict(srate=5999.0), dict(srate=24001.0),
               dict(srate=0.0), dict(srate=float("nan")), dict(srate=float("inf"))):
        with pytest.raises(KiwiGpuError):
            q.start(0, **{"training_interval": 40, **kw})
    for call in (lambda: q.set_wpm(0, -1, 40), lambda: q.set_wpm(0, 0, 0), lambda: q.set_wpm(0, 0, 256), lambda: q.set_pboff(0, 6069), lambda: q.set_pboff(0, 4000000000),
                 lambda: q.set_pboff(1, 818), lambda: q.set_wpm(1, 30, 40)):                          # connection 1 was never started
        with pytest.raises(KiwiGpuError):
            call()
    with pytest.raises(KiwiGpuError):
        q.push([0, 0], np.concatenate([x, x]), [100, 100])
    with pytest.raises(KiwiGpuError):
        q.push([2], x, [100])
    assert q.state(0).tobytes() == before and not np.frombuffer(q.state(1).tobytes(), np.uint8).any()
    # the accepted neighbours move it
    q.set_pboff(0, 6068)
    assert q.state(0)["g_a"] == 44
    # a stopped connection takes nothing
    q.stop(0)
    mid = q.state(0)
    assert len(q.push([0], x, [100])[0]) == 0
    after = q.state(0)
    assert after["started"] == 0 and mid["started"] == 0 and after.tobytes() == mid.tobytes()
    q.close()


# ---- seeded random scripts and shape scripts (tests/ext_random.py): the device against the host model in full, and the fixture.  A
# script begins on a fresh object: what a restart carries over would otherwise come from the script before it.
PARTS = 4                                                                  # the 40 seeds, ten a test


@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("cw")


@pytest.fixture(scope="module")
def random_host(pool, tmp_path_factory):
    """k -> the host driver's result of seed k, or of shape script k - NSEED, sample by sample: made once when first asked for, shared,
    left unchanged"""
    from . import ext_random as er
    tmp = tmp_path_factory.mktemp("cw_random")
    driver, scripts, made = cc.build_driver(tmp), [er.cw_script(s) for s in range(er.NSEED)] + list(er.cw_shapes().values()), {}

    def host(k):
        if k not in made:
            made[k] = cc.run_script_exe(driver, scripts[k], pool, tmp)
        return made[k]
    return host


@pytest.mark.parametrize("part", range(PARTS))
def test_random_scripts_under_a_random_partition(ctx, random_ref, random_host, pool, part):
    """every seed's script with 1, 2, 7, 64 or 256 blocks a push (drawn push by push by a generator of its own) on one connection, and
    a block a push on another: both equal the host model in full, hence each other, and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    for seed in range(part * er.NSEED // PARTS, (part + 1) * er.NSEED // PARTS):
        lines = er.cw_script(seed)
        q = CwDecoder(ctx, nconn=2)
        try:
            got = cc.run_script_dev(q, lines, pool, conn=0, cuts=ed.partition("cw", seed, cc.nblocks(lines)))
            each = cc.run_script_dev(q, lines, pool, conn=1, cuts=lambda: 1)
        finally:
            q.close()
        ed.cw_same(got, random_host(seed), "seed %d" % seed, "the partition")
        ed.cw_same(each, random_host(seed), "seed %d" % seed, "a push a block")
        assert each["calls"] == cc.nblocks(lines) >= got["calls"]
        er.check_record("cw", seed, lines, got, er.unpack(random_ref, seed))


@pytest.mark.parametrize("name", shape_names("cw"))
def test_shape_scripts(ctx, random_ref, random_host, pool, name):
    """a kernel-shape edge (ext_random.cw_shapes), once with up to 256 blocks a push and once with one: both equal the host model
    in full and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    k = er.NSEED + er.shape_names("cw").index(name)
    lines, runs = er.cw_shapes()[name], []
    for cut in (256, 1):
        q = CwDecoder(ctx, nconn=1)
        try:
            runs.append(cc.run_script_dev(q, lines, pool, cuts=lambda: cut))
        finally:
            q.close()
        ed.cw_same(runs[-1], random_host(k), name, "%d blocks a push" % cut)
        er.check_record("cw", k, lines, runs[-1], er.unpack(random_ref, k))
    assert runs[1]["calls"] == cc.nblocks(lines) > runs[0]["calls"]
    if name == "one_push_256":                                                 # the device's own count: 256 * 512 = 1489 * 88 + 40, then 40 + 512 = 6 * 88 + 24
        assert runs[0]["gblocks"] == [(256, 1489), (1, 6)]


@pytest.mark.parametrize("group", range(14))
def test_random_scripts_side_by_side(ctx, random_ref, random_host, pool, group):
    """the seeds three at a time on three connections of one object, in lock step (cw_common.run_side_by_side, drawn from
    ext_random_dev.plan_rng): each connection equals the host model of its own script in full, and the fixture"""
    from . import ext_random as er, ext_random_dev as ed
    q = CwDecoder(ctx, nconn=3)
    try:
        seeds, got, calls, shared = ed.side_by_side("cw", q, pool, group)
    finally:
        q.close()
    for seed, g in zip(seeds, got):
        ed.cw_same(g, random_host(seed), "seed %d of %s" % (seed, seeds))
        er.check_record("cw", seed, er.cw_script(seed), g, er.unpack(random_ref, seed))
    assert shared >= 1 and calls >= shared
