"""kg_cw on the device against tests/golden/cw_ref.npz (the reference's own statements, tools/make_ref_cw_golden.py): the events of every
sound block, every event's fields and the end state -- every scalar, the ring, data[] and the sample buffer -- bit for bit, under seeded
random partitions of 1 to 64 blocks a push.  A push of 7 blocks (which straddles Goertzel blocks: 512 is no multiple of 88) equals 7
pushes of one; four connections with different scripts side by side in one push equal each alone; a pboff between two pushes lands in
mid Goertzel block; a refused command leaves the object as it was; one connection with one block gives 5 Goertzel blocks and carries 72
samples.  Every comparison is an equality."""
import zlib

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, CwDecoder, KiwiGpuError

from . import cw_common as cc

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
    """four scripts on four connections of one object, in lockstep: every round ONE push feeds every connection with blocks left, 1 to
    24 consecutive blocks each under its own now_sec, listed out of connection order; each equals the reference, which is what it gives
    alone"""
    rng = np.random.Generator(np.random.PCG64(0xC351DE))
    scripts = [cc.scripts()[n] for n in SIDE]
    q = CwDecoder(ctx, nconn=len(SIDE) + 1)
    items = [_items(s) for s in scripts]
    at, now = [0] * len(items), [0] * len(items)
    rec = [cc.Recorder(cc.nblocks(s)) for s in scripts]
    shared = 0
    while any(a < len(it) for a, it in zip(at, items)):
        for c, it in enumerate(items):
            while at[c] < len(it) and it[at[c]][0] == "cmd":
                now[c] = cc.apply_command(q, c, it[at[c]][1], now[c])
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
        x = np.zeros((len(conns), most, cc.BLK), np.int16)
        for e, c in enumerate(conns):
            for b, (_, off, _) in enumerate(take[c]):
                x[e, b] = pool[off:off + cc.BLK]
        evs = q.push(conns, x, [now[c] for c in conns], nblk=[len(take[c]) for c in conns])
        for e, c in enumerate(conns):
            rec[c].add([b for _, _, b in take[c]], evs[e])
            at[c] += len(take[c])
        shared += len(conns) > 1
    assert shared >= 10
    for c, name in enumerate(SIDE):
        cc.check_against_golden(golden, name, rec[c].result(q.state(c)))
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
