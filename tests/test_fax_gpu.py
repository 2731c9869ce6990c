"""kg_fax on the device against tests/golden/fax_ref.npz (the reference's own statements, tools/make_ref_fax_golden.py): the lines every
block completed, every line's record, every row byte and the end state -- every scalar and array -- bit for bit, under seeded random
partitions of 1 to 64 blocks a push.  A script pushed a block at a time equals the same pushed at once; connections with different
scripts side by side in one push equal each alone; a refused command leaves the object as it was (the push on device-resident audio is
the receiver bank's: tests/test_fax_bank_gpu.py holds it to the host-array push).  The shapes: 240 lpm (3000 samples a line, the
detector's cap exactly), 120 lpm (the cap below the line), 60 lpm at 20250 Hz (the longest line), a push that ends one sample short of
a line, a skip larger than a block.  Every comparison is an equality."""
import zlib

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, FaxDecoder, KiwiGpuError

from . import fax_common as fc

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


def _items(lines):
    out, seen = [], 0
    for l in lines:
        if l[0] == "B":
            out.append(("blk", int(l.split()[1]), seen))
            seen += 1
        else:
            out.append(("cmd", l))
    return out


def test_connections_side_by_side_equal_each_alone(golden, pool, ctx):
    """six scripts on six connections of one object, in lockstep: every round ONE push feeds every connection with blocks left, 1 to 24
    consecutive blocks each, listed out of connection order; each equals the reference, which is what it gives alone"""
    rng = np.random.Generator(np.random.PCG64(0xFA51DE))
    scripts = [fc.scripts()[n] for n in SIDE]
    q = FaxDecoder(ctx, nconn=len(SIDE) + 1)
    items = [_items(s) for s in scripts]
    at, rate, width = [0] * len(items), [0.0] * len(items), [0] * len(items)
    rec = [fc.Recorder(fc.nblocks(s)) for s in scripts]
    shared = 0
    while any(a < len(it) for a, it in zip(at, items)):
        for c, it in enumerate(items):
            while at[c] < len(it) and it[at[c]][0] == "cmd":
                rate[c] = fc.apply_command(q, c, it[at[c]][1], rate[c])
                if it[at[c]][1][0] == "C":
                    width[c] = int(it[at[c]][1].split()[2])
                at[c] += 1
        take = {}
        for c, it in enumerate(items):
            n = 0
            lim = int(rng.integers(1, 25))
            while n < lim and at[c] + n < len(it) and it[at[c] + n][0] == "blk":
                n += 1
            if n:
                take[c] = it[at[c]:at[c] + n]
        if not take:
            break
        conns = sorted(take, key=lambda c: -c)
        most = max(len(v) for v in take.values())
        x = np.zeros((len(conns), most, fc.BLK), np.int16)
        for e, c in enumerate(conns):
            for b, (_, off, _) in enumerate(take[c]):
                x[e, b] = pool[off:off + fc.BLK]
        recs, rows = q.push(conns, x, [rate[c] for c in conns], nblk=[len(take[c]) for c in conns])
        for e, c in enumerate(conns):
            rec[c].add([b for _, _, b in take[c]], recs[e], rows[e], width[c])
            at[c] += len(take[c])
        shared += len(conns) > 1
    assert shared >= 5
    for c, name in enumerate(SIDE):
        fc.check_against_golden(golden, name, rec[c].result(fc.state_of(q, c)))
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
