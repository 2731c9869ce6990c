"""Stage 2 of kg_wspr on the device against tests/golden/wspr_dec_ref.npz (the reference's own statements with the seeds of
kg_libm_dtrig.h, tools/make_ref_wspr_dec_golden.py): every scene through load_iq + decode, every pass, every field of every record BIT
FOR BIT.  np is 45000 by definition, so the edges come from the scenes (tests/wspr_dec_common.py; tests/test_wspr_dec_cpu.py holds the
golden to what each is named for): drift 0, driftp / driftm winning, symbols at k <= 0 with k == 0 inside a sum, symbols at k >= np
from a caller-given shift0 of 3900, decodes at positive and negative ii, TIME_UP at (200, 2) and then 129 jiggles at (1000, 1) with
ignore carried over, NO_CHANGE, MINSYNC1, silence, quickmode, twelve candidates with images, second passes that skip; fourteen
connections at once; kg_wspr_fano alone; the refusals; and a pushed cycle's candidates decoded as the same candidates handed in."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, KiwiGpuError, Wspr, wspr

from . import wspr_common as W1
from . import wspr_dec_common as W

pytestmark = pytest.mark.gpu
NCONN = 14


@pytest.fixture(scope="module")
def golden():
    return W.load()


@pytest.fixture(scope="module")
def q(golden):
    ctx = Context(0)
    q = Wspr(ctx, nconn=NCONN)
    for c in range(NCONN):
        q.init(c, 375.0)
    q.set_metric_table(golden["mettab"])
    yield q
    q.close()
    ctx.close()


def recs_of(g, name):
    return np.ascontiguousarray(g["s_%s_recs" % name]).view(W.rec_dtype)[..., 0]


def load_scene(q, conn, half, name):
    x, cands, passes = W.scene_inputs(name)
    q.load_iq(conn, half, x, [tuple(c) for c in cands.tolist()])
    return cands.size, passes


def same_records(got, want, what):
    assert got.dtype == wspr.dec_dtype and want.dtype == W.rec_dtype
    for f in W.rec_dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), (what, f, got[f].tolist(), want[f].tolist())


@pytest.mark.parametrize("name", sorted(W.SCENES))
def test_scene_equals_the_golden(golden, q, name):
    ncand, passes = load_scene(q, 0, 1, name)
    want = recs_of(golden, name)
    for ps, (maxcycles, iifac, quick) in enumerate(passes.tolist()):
        out, n = q.decode([0], maxcycles, iifac, quick)
        assert n[0] == ncand
        same_records(out[0][:ncand], want[ps], (name, ps))
        assert out[0][ncand:].tobytes() == bytes(304 * (W.MAX_NPK - ncand))                                  # behind the last candidate: zeros


def test_fourteen_connections_at_once_equal_each_alone(golden, q):
    names = [n for n in sorted(W.SCENES) if W.SCENES[n]["passes"][0] == W.P0][:NCONN]                      # the scenes whose first pass is (200, 2)
    assert len(names) == NCONN
    for c, name in enumerate(names):
        load_scene(q, c, c & 1, name)
    order = [5, 0, 13, 2, 7, 1, 9, 3, 11, 4, 12, 6, 10, 8]                                                  # a list that is not the identity
    out, n = q.decode(order, 200, 2)
    for e, c in enumerate(order):
        want = recs_of(golden, names[c])[0]
        assert n[e] == want.size
        same_records(out[e][:want.size], want, (names[c], "connection", c))
    out2, _ = q.decode(order, 1000, 1)                                                                      # ignore carried per connection
    for e, c in enumerate(order):
        if len(W.SCENES[names[c]]["passes"]) > 1 and W.SCENES[names[c]]["passes"][1] == W.P1 and W.SCENES[names[c]]["passes"][0] == W.P0:
            same_records(out2[e][:n[e]], recs_of(golden, names[c])[1], (names[c], "second pass", c))


def test_fano_alone(golden, q):
    fs = W.fano_sets()
    for mc in sorted({v[1] for v in fs.values()}):
        names = [n for n in sorted(fs) if fs[n][1] == mc]
        ok, metric, cycles, maxnp, data = q.fano(np.stack([fs[n][0] for n in names]), mc)
        for k, n in enumerate(names):
            want = golden["f_%s" % n].view(W.fano_dtype)[0]
            assert (ok[k], metric[k], cycles[k], maxnp[k], bytes(data[k])) == (want["ok"], want["metric"], want["cycles"], want["maxnp"], bytes(want["data"])), n
    # the golden's gated sets: a record whose last jiggle passed the gate holds that jiggle's deinterleaved symbols and its fano run
    n = 0
    for name in W.SCENES:
        for ps, (maxcycles, iifac, quick) in enumerate(W.SCENES[name]["passes"]):
            for r in recs_of(golden, name)[ps]:
                if r["result"] == W.DECODED:
                    ok, metric, cycles, maxnp, data = q.fano(r["symbols"], maxcycles)
                    assert (ok[0], metric[0], cycles[0], maxnp[0], bytes(data[0])) == (1, r["metric"], r["cycles"], r["maxnp"], bytes(r["decdata"][:10])), name
                    n += 1
    assert n >= 13
    # 40 sets in one call, more than a workgroup's lanes: each equals itself alone
    many = np.stack([fs["noisy"][0], fs["random"][0], fs["saturated"][0], fs["too_noisy"][0]] * 10)
    ok, metric, cycles, maxnp, data = q.fano(many, 200)
    one = q.fano(many[:4], 200)
    for k in range(40):
        assert (ok[k], metric[k], cycles[k], maxnp[k], bytes(data[k])) == (one[0][k % 4], one[1][k % 4], one[2][k % 4], one[3][k % 4], bytes(one[4][k % 4]))


def test_refusals_leave_the_object_unchanged(golden, q):
    ctx = q.ctx
    bare = Wspr(ctx, nconn=1)
    bare.init(0, 375.0)
    x, cands, _ = W.scene_inputs("strong")
    bare.load_iq(0, 0, x, [tuple(c) for c in cands.tolist()])
    for call in (lambda: bare.decode([0]), lambda: bare.fano(np.zeros(162, np.uint8))):
        with pytest.raises(KiwiGpuError) as e:
            call()
        assert e.value.status == -5                                                                         # KG_ERR_STATE: no table
    bare.close()
    load_scene(q, 3, 0, "strong")
    bad = [lambda: q.load_iq(3, 0, x, [(114.0, 768, 0.0, 0.5)]), lambda: q.load_iq(3, 0, x, [(10.0, 45001, 0.0, 0.5)]), lambda: q.load_iq(3, 0, x, [(10.0, 768, -4.5, 0.5)]),
           lambda: q.load_iq(3, 0, x, [(float("nan"), 768, 0.0, 0.5)]), lambda: q.load_iq(3, 2, x, []), lambda: q.load_iq(3, 0, x, [(1.0, 1, 0.0, 0.0)] * 13),
           lambda: q.decode([3], 200, 0), lambda: q.decode([3], 200, 129), lambda: q.decode([3], 0, 2), lambda: q.decode([3], (1 << 20) + 1, 2),
           lambda: q.decode([3, 3]), lambda: q.decode([NCONN]), lambda: q.fano(np.zeros(162, np.uint8), 0),
           lambda: q.set_metric_table(np.full((2, 256), (1 << 20) + 1, np.int32))]
    for call in bad:
        with pytest.raises(KiwiGpuError) as e:
            call()
        assert e.value.status == -2
    out, n = q.decode([3], 200, 2)                                                                          # samples, candidates, ignore and table as they were
    same_records(out[0][:1], recs_of(golden, "strong")[0], "after the refusals")
    out, n = q.decode([3], 1, 128)                                                                          # the neighbours of the refusals are taken
    assert out[0][0]["result"] == W.SKIPPED


def test_a_pushed_cycles_candidates_decode_as_the_same_candidates_handed_in(golden, q):
    """the held list a cycle end leaves (kg_wspr_push) against kg_wspr_load_iq of the same samples and candidates: equal records.  The
    scene's 4-FSK signal carries seeded symbols, not a code word: its candidate passes the gate on every jiggle and fano times out"""
    pool = W1.pool()
    lines = [l.split() for l in W1.scripts()["e2e_a"] if l.startswith("B ")][:88]
    iq = np.stack([pool[int(l[1]):int(l[1]) + 512] for l in lines]).reshape(1, 88, 512)
    p = Wspr(q.ctx, nconn=2)
    p.set_metric_table(golden["mettab"])
    for c in range(2):
        p.init(c, 375.0)
    p.set_capture(1, 1)
    rows, m, ev, cyc, counts = p.push([1], iq, [[int(l[3]) for l in lines]], [[int(l[4]) for l in lines]])
    assert cyc[0]["due"] == 1 and cyc[0]["npk"] >= 1
    npk, half = int(cyc[0]["npk"]), int(cyc[0]["half"])
    out, n = p.decode([1], 200, 2)
    first = out[0][0]
    assert n[0] == npk and first["result"] == wspr.TIME_UP and first["gates"] == first["idt"] == 65 and first["sync1"] > 0.3 and first["ignore"] == 0
    samples = p.state(1, samples=True)[3]
    p.load_iq(0, half, (samples[0][half], samples[1][half]), cyc[0]["cand"][:npk])
    out0, n0 = p.decode([0], 200, 2)
    assert n0[0] == npk and out0[0].tobytes() == out[0].tobytes()
    later = p.decode([1], 1000, 1)[0][0][:npk]                                                              # ignore carried from the pass above
    assert (later["result"][out[0][:npk]["ignore"] == 1] == wspr.SKIPPED).all()
    p.close()


def test_set_decode_runs_pass_0_behind_a_pushed_cycle_end(golden, q):
    """kg_wspr_set_decode on: the push that holds the cycle end leaves the records that kg_wspr_decode (200, 2) gives by hand on an object
    pushed the same with it off; rows, row map, cycle record, counts and state are those of the push with it off, and so are the events
    but for KG_WSPR_EV_DECODES between PEAKS and the resume; ignore is carried into the next pass; before the table it is refused"""
    pool = W1.pool()
    lines = [l.split() for l in W1.scripts()["e2e_a"] if l.startswith("B ")][:88]
    iq = np.stack([pool[int(l[1]):int(l[1]) + 512] for l in lines]).reshape(1, 88, 512)
    mi, se = [[int(l[3]) for l in lines]], [[int(l[4]) for l in lines]]
    on, off = Wspr(q.ctx, nconn=2), Wspr(q.ctx, nconn=2)
    for p in (on, off):
        for c in range(2):
            p.init(c, 375.0)
        p.set_capture(1, 1)
    with pytest.raises(KiwiGpuError) as e:
        on.set_decode(1, 1)
    assert e.value.status == -5
    for p in (on, off):
        p.set_metric_table(golden["mettab"])
    on.set_decode(1, 1)
    on.set_decode(0, 1)
    on.set_decode(0, 0)
    got, want = [], []
    for a in range(0, 88, 8):                                                                               # eleven pushes; the last holds group 85
        got.append(on.push([1], iq[:, a:a + 8], [mi[0][a:a + 8]], [se[0][a:a + 8]]))
        want.append(off.push([1], iq[:, a:a + 8], [mi[0][a:a + 8]], [se[0][a:a + 8]]))
        assert on.decodes(1).size == (0 if a < 80 else got[-1][3][0]["npk"])
    for g, w in zip(got, want):
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes() and g[3].tobytes() == w[3].tobytes() and g[4].tobytes() == w[4].tobytes()
        assert g[2][g[2]["kind"] != wspr.EV_DECODES].tobytes() == w[2].tobytes()
    ev = got[-1][2]
    k = int(np.flatnonzero(ev["kind"] == wspr.EV_DECODES)[0])
    assert (ev["kind"] == wspr.EV_DECODES).sum() == 1 and ev[k - 1]["kind"] == wspr.EV_PEAKS and ev[k + 1]["kind"] == wspr.EV_STATUS and ev[k]["a"] == ev[k - 1]["a"]
    assert sum(int((g[2]["kind"] == wspr.EV_DECODES).sum()) for g in got[:-1]) == 0
    npk = int(got[-1][3][0]["npk"])
    assert npk >= 1 and off.decodes(1).size == 0
    by_hand, n = off.decode([1], 200, 2)
    assert n[0] == npk and on.decodes(1).tobytes() == by_hand[0][:npk].tobytes() and by_hand[0][0]["result"] == wspr.TIME_UP
    assert on.decode([1], 1000, 1)[0].tobytes() == off.decode([1], 1000, 1)[0].tobytes()                     # ignore as the pass by hand left it
    assert on.decodes(1).tobytes() == by_hand[0][:npk].tobytes()                                            # a pass by hand leaves the push's records alone
    for c in range(2):
        a, b = on.state(c, planes=True, samples=True), off.state(c, planes=True, samples=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    on.close()
    off.close()


def test_cpp_caller_decodes_the_message_it_encoded():
    """examples/wspr_decode_dropin.cpp: a host with its own metric table -- mettab by the reference's formula, kg_wspr_set_metric_table,
    load_iq, the passes of kg_wspr_decode -- through include/kiwigpu.h alone; it checks its own decode"""
    import os
    import subprocess
    exe = os.path.join(W.ROOT, "examples", "wspr_decode_dropin")
    assert os.path.exists(exe), "examples/wspr_decode_dropin is not built (run __graft_entry__.build())"
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert lines[0].startswith("pass 0 candidate 0: result 4 ") and " jiggles 1 cycles 82" in lines[0] and lines[-1].startswith("decoded ") and len(lines) == 2
