"""kg_ft8 on the device against tests/golden/ft8_ref.npz (the reference's own statements; tools/make_ref_ft8_golden.py) and against the
host twin (tools/ft8_host_driver.cpp).
(a) kg_ft8_load_wf equals the golden bit for bit: the candidates, their order, freq_hz / time_sec / snr, log174 with its NaNs.
(b) The monitor scenes: schedule, events and last_frame equal; every waterfall byte within 1 of build A's (the reference's kiss_fftr);
    the count of differing bytes of a scene at most 4 * max(n_AB, 1), n_AB being what the reference's builds A and B differ in over
    the same bytes -- the device is a third correct fp32 transform, two independent errors meet (x 2), and x 2 for the spread between
    scenes --; max_mag within 4 x the recorded A-B difference or 1e-4 dB, whichever is larger; silence exact.  The counts reached are
    written for profiles/ft8_rows.txt with KIWIGPU_FT8_ROWS_OUT=<file>.
(c) End to end: the device's candidates and log174 equal the twin run on the device's OWN waterfall bytes, bit for bit, and every
    planted frame is among the candidates at its planted (time_offset, time_sub, freq_offset, freq_sub).
(d) Any partition of a stream into pushes equals one-callback pushes; 14 connections at unequal phases and mixed protocols equal each
    alone.  And the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, Ft8, KiwiGpuError, ft8, live_allocs

from . import ft8_common as F

pytestmark = pytest.mark.gpu
INVALID, STATE, NOMEM = -2, -5, -4


@pytest.fixture(scope="module")
def golden():
    return F.load()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return F.build_driver(tmp_path_factory.mktemp("ft8"))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def run_stream(q, conns, streams, cuts):
    """streams: per connection (samples [ncb, ns], times [ncb]); cuts: the callbacks at which a push ends, ascending, the last one at
    least the longest stream -> per connection dict(events, slots, info, last_frame, mag, last_mag)"""
    out = {c: dict(events=[], slots=[]) for c in conns}
    at = 0
    for cut in cuts:
        n = cut - at
        ncb = np.array([max(0, min(n, streams[i][0].shape[0] - at)) for i in range(len(conns))], np.int32)
        if n <= 0 or not ncb.any():
            at = max(at, cut)
            continue
        x = np.zeros((len(conns), n, F.NS), np.int16)
        t = np.zeros((len(conns), n))
        for i in range(len(conns)):
            x[i, :ncb[i]] = streams[i][0][at:at + ncb[i]]
            t[i, :ncb[i]] = streams[i][1][at:at + ncb[i]]
        ev, sl = q.push(conns, x, t, ncb=ncb)
        for e in ev:
            out[int(e["conn"])]["events"].append((int(e["cb"]) + at, int(e["kind"]), int(e["a"]), int(e["b"]), int(e["t"])))
        for s in sl:
            out[int(s["conn"])]["slots"].append(s.copy())
        at = cut
    for c in conns:
        info, lf, mag = q.state(c)
        out[c].update(info=info.copy(), last_frame=lf, mag=mag, last_mag=q.state(c, previous=True)[2])
    return out


def even_cuts(ncb, step):
    return list(range(step, ncb, step)) + [ncb]


def state_of(info):
    return [int(info[f]) for f in ("tsync", "in_pos", "frame_pos", "num_blocks", "slot", "decode_time")]


# ---- (a)
@pytest.mark.parametrize("name", sorted(F.LOADS))
def test_load_wf_equals_the_golden(golden, ctx, name):
    p, kw, ncand, min_score = F.LOADS[name]
    q = Ft8(ctx, nconn=2)
    sl = q.load_wf(1, p, F.waterfall(p, **kw), ncand, min_score)
    k = "l_%s_" % name
    n = int(golden[k + "head"][2])
    keep = F.LDPC_N if name == F.FULL_LOG else F.KEEP
    assert sl["ncand"] == n and sl["num_blocks"] == int(golden[k + "head"][1]) and sl["due"] == 1 and sl["conn"] == 1 and sl["max_mag"] == np.float32(-120.0)
    assert sl["cand"][:n].tobytes() == np.ascontiguousarray(golden[k + "cand"]).tobytes(), (name, "candidates, their order, freq_hz, time_sec, snr")
    assert not sl["cand"][n:].tobytes().strip(b"\0") and not sl["log174"][n:].tobytes().strip(b"\0"), (name, "zeros behind ncand")
    assert F.bits(sl["log174"][:n][:keep]).tobytes() == F.bits(golden[k + "log174"]).tobytes(), (name, "log174")
    assert F.digest(np.ascontiguousarray(sl["log174"][:n]).tobytes()) == bytes(golden[k + "log_sha"]), (name, "log174 of every candidate")
    if "_const_" in name:
        assert np.isnan(sl["log174"][:n]).all()
    q.close()


# ---- (b)
@pytest.mark.parametrize("name", sorted(F.MONITOR))
def test_monitor_scene(golden, ctx, name):
    p, make = F.STREAMS[name]
    x, t = make()
    q = Ft8(ctx, nconn=2)
    q.init(1, p)
    got = run_stream(q, [1], [(x, t)], even_cuts(x.shape[0], 24))[1]
    k = "s_%s_" % name
    assert np.array_equal(np.array(got["events"], np.int64).reshape(-1, 5), golden[k + "events"]), (name, "events")
    assert state_of(got["info"]) == [int(v) for v in golden[k + "state"]], (name, "the schedule's state")
    assert F.digest(got["last_frame"].tobytes()) == bytes(golden[k + "last_frame_sha"]), (name, "last_frame")
    mine = [got["mag"].ravel()]
    want = [golden[k + "end_mag"]]
    mm = [(float(got["info"]["max_mag"]), float(golden[k + "max_mag_a"][-1]))]
    if k + "tail_mag" in golden:
        tail = golden[k + "tail_mag"]
        assert len(got["slots"]) == 1 and got["slots"][0]["num_blocks"] == F.SIZES[p]["slot_blocks"] == got["last_mag"].shape[0]
        mine.append(got["last_mag"].ravel()[-tail.size:])
        want.append(tail)
        mm.append((float(got["slots"][0]["max_mag"]), float(golden[k + "max_mag_a"][0])))
        assert float(got["info"]["last_max_mag"]) == float(got["slots"][0]["max_mag"])
    else:
        assert not got["slots"]
    mine, want = np.concatenate(mine).astype(np.int32), np.concatenate(want).astype(np.int32)
    assert mine.size == want.size
    d = np.abs(mine - want)
    n_ab, bar_mm = int(golden[k + "n_ab_kept"][0]), max(4.0 * float(golden[k + "max_mag_ab"][0]), 1e-4)
    line = "%s: %d of %d waterfall bytes differ from build A's (largest difference %d; builds A and B: %d; bar %d); max_mag off by %.3g dB (bar %.3g)" % (
        name, (d != 0).sum(), d.size, d.max(initial=0), n_ab, 4 * max(n_ab, 1), max(abs(a - b) for a, b in mm), bar_mm)
    print(line)
    if os.environ.get("KIWIGPU_FT8_ROWS_OUT"):
        with open(os.environ["KIWIGPU_FT8_ROWS_OUT"], "a") as f:
            f.write(line + "\n")
    assert d.max(initial=0) <= 1, line
    assert (d != 0).sum() <= 4 * max(n_ab, 1), line
    for a, b in mm:
        assert abs(a - b) <= bar_mm, line
    if name.startswith("silence"):
        assert not mine.any() and got["info"]["max_mag"] == np.float32(-120.0), name
    q.close()


# ---- (c)
@pytest.mark.parametrize("p", [F.FT8, F.FT4])
def test_end_to_end_equals_the_twin_on_the_device_bytes(ctx, driver, tmp_path, p):
    x, t = F.STREAMS["e2e_" + F.pname(p)][1]()
    q = Ft8(ctx, nconn=1)
    q.init(0, p)
    got = run_stream(q, [0], [(x, t)], even_cuts(x.shape[0], 40))[0]
    assert len(got["slots"]) == 1
    sl = got["slots"][0]
    n = int(sl["ncand"])
    twin = F.run_exe(driver, F.load_bytes(p, got["last_mag"]), tmp_path)["slots"][0]
    assert n == twin["ncand"] and sl["num_blocks"] == F.SIZES[p]["slot_blocks"]
    assert sl["cand"][:n].tobytes() == twin["cand"].tobytes(), "candidates"
    assert F.bits(sl["log174"][:n]).tobytes() == F.bits(twin["log174"]).tobytes(), "log174"
    have = {tuple(int(c[f]) for f in ("time_offset", "time_sub", "freq_offset", "freq_sub")) for c in sl["cand"][:n]}
    for fr in F.E2E_FRAMES[p]:
        assert fr in have, ("the frame planted at (time_offset, time_sub, freq_offset, freq_sub) is not a candidate", fr)
    q.close()


# ---- (d)
def same_run(a, b, what):
    assert a["events"] == b["events"], (what, "events")
    assert len(a["slots"]) == len(b["slots"]), what
    for s, r in zip(a["slots"], b["slots"]):
        s, r = s.copy(), r.copy()
        s["conn"] = r["conn"] = 0
        assert s.tobytes() == r.tobytes(), (what, "slot record")
    assert state_of(a["info"]) == state_of(b["info"]) and a["info"]["max_mag"].tobytes() == b["info"]["max_mag"].tobytes(), (what, "state")
    for f in ("last_frame", "mag", "last_mag"):
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def test_any_partition_equals_one_callback_pushes(ctx):
    p = F.FT4
    x, t = F.STREAMS["boundary_ft4"][1]()
    ncb = x.shape[0]
    runs = []
    r = np.random.default_rng(F.BASE + 77)
    for cuts in (list(range(1, ncb + 1)), sorted(set(r.integers(1, ncb, 12).tolist())) + [ncb], [ncb]):      # the last: the whole slot and the next one's start in ONE push
        q = Ft8(ctx, nconn=1)
        q.init(0, p)
        runs.append(run_stream(q, [0], [(x, t)], cuts)[0])
        q.close()
    assert len(runs[0]["slots"]) == 1 and runs[0]["info"]["num_blocks"] >= 3
    same_run(runs[0], runs[1], "a random partition")
    same_run(runs[0], runs[2], "one push")


def test_14_connections_equal_each_alone(ctx):
    streams, protos = [], []
    for c in range(14):
        p = F.FT4 if c % 2 else F.FT8
        x, t = F.STREAMS["boundary_" + F.pname(p)][1]()
        streams.append((x[c:], t[c:]))                                     # unequal phases: the sync finds each at another in_pos
        protos.append(p)
    longest = max(s[0].shape[0] for s in streams)
    q = Ft8(ctx, nconn=16)
    conns = [15 - c for c in range(14)]
    for c, p in zip(conns, protos):
        q.init(c, p)
    together = run_stream(q, conns, streams, even_cuts(longest, 48))
    q.close()
    for i in range(14):
        one = Ft8(ctx, nconn=1)
        one.init(0, protos[i])
        alone = run_stream(one, [0], [streams[i]], even_cuts(streams[i][0].shape[0], 48))[0]
        one.close()
        assert len(alone["slots"]) == 1
        same_run(together[conns[i]], alone, "connection %d" % conns[i])


# ---- the refusals
def test_refusals(ctx):
    allocs = live_allocs()
    q = Ft8(ctx, nconn=3)
    lib = q.lib

    def refused(status, call):
        with pytest.raises(KiwiGpuError) as e:
            call()
        assert e.value.status == status, e.value

    assert lib.kg_ft8_init(None, 0, 0, 12000.0) == INVALID and lib.kg_ft8_set_snr_adj(None, 0.0) == INVALID
    refused(INVALID, lambda: Ft8(ctx, nconn=0))
    refused(INVALID, lambda: Ft8(ctx, nconn=65))
    refused(INVALID, lambda: q.init(3, F.FT8))
    refused(INVALID, lambda: q.init(-1, F.FT8))
    refused(INVALID, lambda: q.init(0, 2))
    refused(INVALID, lambda: q.init(0, F.FT8, 20250.0))                    # nfft 6480 / 1944: refused, not faked
    refused(INVALID, lambda: q.set_snr_adj(float("nan")))
    x = np.zeros((1, 2, F.NS), np.int16)
    refused(STATE, lambda: q.push([0], x, 100.0))                          # before init
    q.init(0, F.FT4)
    q.init(1, F.FT8)
    refused(INVALID, lambda: q.push([0, 0], np.zeros((2, 2, F.NS), np.int16), 100.0))
    refused(INVALID, lambda: q.push([3], x, 100.0))
    refused(STATE, lambda: q.push([0, 2], np.zeros((2, 2, F.NS), np.int16), 100.0))
    for bad in (np.nan, np.inf, -1.0, 2.0 ** 41):
        refused(INVALID, lambda: q.push([0], x, [[100.0, bad]]))
    refused(INVALID, lambda: q.push([0], np.zeros((1, 1, 2049), np.int16), 100.0))
    two = 2 * int(7.5 * F.RATE / F.NS) + 8                                 # two FT4 slots in one push
    refused(INVALID, lambda: q.push([0], np.zeros((1, two, F.NS), np.int16), F.clock(7500.8125, two)[None]))
    refused(INVALID, lambda: q.push([0], np.zeros((1, two // 2, F.NS), np.int16), F.clock(7500.8125, two // 2)[None], max_slots=0))
    refused(INVALID, lambda: q.push([0], x, 7500.8125, max_events=0))
    assert state_of(q.state(0)[0]) == [0, 0, 0, 0, 0, 0]                   # nothing changed
    assert q.plan([0], [two // 2], F.NS, F.clock(7500.8125, two // 2)[None]) == (150, 3, 1) and state_of(q.state(0)[0]) == [0, 0, 0, 0, 0, 0]
    mag = np.zeros((2, 2, 2, 481), np.uint8)
    refused(INVALID, lambda: q.load_wf(0, F.FT8, mag, 0, 10))
    refused(INVALID, lambda: q.load_wf(0, F.FT8, mag, 141, 10))
    refused(INVALID, lambda: q.load_wf(3, F.FT8, mag))
    refused(INVALID, lambda: q.load_wf(0, F.FT8, np.zeros((94, 2, 2, 481), np.uint8)))
    assert lib.kg_ft8_load_wf(q.h, 0, 0, 2, None, 140, 10, None) == INVALID
    ev, sl = q.push([1, 0], np.zeros((2, 2, F.NS), np.int16), [[15000.8125, 15000.85], [7500.8125, 7500.85]])
    assert [(int(e["conn"]), int(e["kind"]), int(e["a"])) for e in ev] == [(1, ft8.EV_SLOT_START, 1), (0, ft8.EV_SLOT_START, 1)] and sl.size == 0
    q.close()
    assert live_allocs() == allocs


def test_a_failed_create_leaves_nothing_behind(ctx, monkeypatch):
    allocs = live_allocs()
    monkeypatch.setenv("KIWIGPU_TUNING", "1")
    refusals = 0
    for k in range(1, 12):
        monkeypatch.setenv("KIWIGPU_FAIL_ALLOC", str(k))
        try:
            q = Ft8(ctx, nconn=2)
        except KiwiGpuError as e:
            assert e.status == NOMEM and live_allocs() == allocs, (k, e)
            refusals += 1
            continue
        q.close()
        break
    monkeypatch.delenv("KIWIGPU_FAIL_ALLOC")
    monkeypatch.delenv("KIWIGPU_TUNING")
    assert refusals == 7 and live_allocs() == allocs                       # the seven buffers of kg_ft8_create


def test_the_drop_in_example_finds_its_frame():
    """examples/ft8_dropin.cpp: a host that passes its callbacks and their clock readings to kg_ft8_push and reads the slot record"""
    import subprocess
    exe = os.path.join(F.ROOT, "examples", "ft8_dropin")
    assert os.path.exists(exe), "examples/ft8_dropin is not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "found the frame at block 3, bin 100" in r.stdout, (r.stdout, r.stderr)
