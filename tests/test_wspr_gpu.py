"""kg_wspr on the device against tests/golden/wspr_ref.npz (the reference's own statements, tools/make_ref_wspr_golden.py), at snd_rate
375 and 750 (int_decimate 1 and 2: the 750 Hz stream is the 375 Hz one with a noise sample ahead of every sample, which the
drop-sample decimation discards).

(a) the `_load` path: peaks and candidates from the golden's planes, bit for bit.
(b) the push path: what passes through the transform -- pwr_samp against the double-precision DFT of the windowed samples, pwr_sampavg
    against the golden -- within the project's bar, 1e-5 of the plane's maximum (dft_truth.OLD_BAR); the transform's magnitudes within
    dft_truth's fp32 bar on the same inputs; the row bytes within what the reference's own two builds (exact stand-in for FFTW against
    an fp32 one) differ by on the same scenes: twice that count plus one a row, never more than 1 LSB.  The schedule, the events and
    the end state are equalities.
(c) end to end: shift0, drift0 and freq0 of the candidates of the synthetic 4-FSK scenes equal the golden's.
(d) the schedule's edges: whatever way a stream is cut into pushes, every output is bit-identical to one-block pushes."""
import os
import zlib

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, KiwiGpuError, Wspr, wspr

from . import dft_truth as T
from . import wspr_common as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return W.load()


@pytest.fixture(scope="module")
def pool():
    return W.pool()


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def run_script_dev(q, lines, pool, conn=0, cut=lambda: 1, dec=1):
    """the script on connection conn; runs of B lines of one size go out in pushes of cut() blocks -> what W.golden_of() holds, in full"""
    ev, rows, meta, cyc, calls = [], [], [], [], 0
    nb, i = 0, 0
    while i < len(lines):
        l = lines[i].split()
        if l[0] == "I":
            q.init(conn, float(l[1]) * dec)
        elif l[0] == "C":
            q.set_capture(conn, int(l[1]))
        elif l[0] == "Y":
            q.set_type(conn, int(l[1]))
        elif l[0] == "M":
            q.set_more_candidates(conn, int(l[1]))
        elif l[0] == "B":
            n, take = int(l[2]), cut()
            j = i
            while j < len(lines) and j - i < take and lines[j].startswith("B ") and int(lines[j].split()[2]) == n:
                j += 1
            b = [lines[k].split() for k in range(i, j)]
            x = np.stack([pool[int(f[1]):int(f[1]) + n] for f in b])
            if dec == 2:
                x = np.stack([W.interleave(r, seed=100 + nb + k) for k, r in enumerate(x)])
            rb, m, e, cy, counts = q.push([conn], x[None], [[int(f[3]) for f in b]], [[int(f[4]) for f in b]])
            calls += 1
            assert counts[0, 0] == m.size and counts[0, 1] == cy[0]["due"]
            for v in e:
                if v["kind"] == wspr.EV_STATUS:
                    ev.append((-1 if v["blk"] < 0 else nb + int(v["blk"]), int(v["a"])))
            for r in m:
                meta.append((nb + int(r["blk"]), int(r["group"]), int(r["half"]), int(r["tsync"])))
                rows.append(rb[int(r["off"]):int(r["off"]) + W.NBINS + 1].copy())
                assert rows[-1][0] == r["tsync"]
            if cy[0]["due"]:
                pe = [v for v in e if v["kind"] == wspr.EV_PEAKS]
                assert len(pe) == 1 and counts[0, 2] == cy[0]["npk"]
                cyc.append((nb + int(pe[0]["blk"]), cy[0].copy()))
            nb += j - i
            i = j - 1
        i += 1
    info, avg, planes, iq = q.state(conn, planes=True, samples=True)
    return dict(ev=np.array(ev, np.int32).reshape(-1, 2), rows=np.array(rows, np.uint8).reshape(-1, W.NBINS + 1), meta=np.array(meta, np.int32).reshape(-1, 4),
                cyc=cyc, info=np.array([int(info[n]) for n in wspr.info_dtype.names[:18]], np.int32), pwr_sampavg=avg, pwr_samp=planes, iq=iq, calls=calls)


def cycle_words(blk, cy):
    """a device cycle record as the golden's 111 words"""
    w = [blk, int(cy["half"]), int(cy["npk"])]
    for p in cy["pk"]:
        w += [int(p["bin0"]), int(p["freq0"].view(np.int32)), int(p["snr0"].view(np.int32))]
    for c in cy["cand"]:
        w += [int(c["freq0"].view(np.int32)), int(c["shift0"]), int(c["drift0"].view(np.int32)), int(c["sync0"].view(np.int32)), int(c["freq_idx"]), int(c["bin0"])]
    return np.array(w, np.int32)


# ---- (a)
@pytest.mark.parametrize("name", sorted(W.LOADS))
def test_load_path_equals_the_reference_bit_for_bit(golden, ctx, name):
    kw, head = W.LOADS[name]
    q = Wspr(ctx, nconn=2)
    q.init(1, 375.0)
    for l in head:
        (q.set_more_candidates if l[0] == "M" else q.set_type)(1, int(l.split()[1]))
    ps, pa = W.planes(**kw)
    cy = q.load(1, 0, ps, pa)
    want = golden["s_load_%s_cyc" % name][0]
    got = cycle_words(int(want[0]), cy)
    assert cy["due"] == 1 and got.tobytes() == want.tobytes(), (name, np.flatnonzero(got != want)[:8])
    info, avg, planes, _ = q.state(1, planes=True)
    assert planes[0].tobytes() == ps.tobytes() and avg[0].tobytes() == pa.tobytes() and not planes[1].any()      # handed out as the reference lays them out
    q.close()


# ---- (b), (c)
@pytest.fixture(scope="module")
def pushed(golden, pool, ctx):
    """every pushed scene at both rates, once: name, dec -> the run"""
    out = {}
    for name in ("e2e_a", "resync", "silence"):
        for dec in (1, 2):
            q = Wspr(ctx, nconn=1)
            rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode()) + dec))
            out[name, dec] = run_script_dev(q, W.scripts()[name], pool, cut=lambda: int(rng.integers(1, 9)), dec=dec)
            q.close()
    return out


def truth_planes(iq_half, ntr):
    """pwr_samp [512, ntr] of one half from its i / q data: the window of wspr_main.cpp:1187, the float products, the DFT in double"""
    win = np.sin(np.arange(W.NFFT) * np.pi / (W.NFFT - 1)).astype(np.float32)
    x = (iq_half[0] + 1j * iq_half[1]).astype(np.complex64)
    out = np.zeros((W.NFFT, ntr))
    spec = []
    for i in range(ntr):
        seg = x[128 * i:128 * i + 512]
        xin = (seg.real * win + 1j * (seg.imag * win)).astype(np.complex64)
        y = T.dft(xin)
        spec.append((xin, y))
        out[:, i] = np.roll(T.power(y), 256)
    return out, spec


@pytest.mark.parametrize("dec", [1, 2])
@pytest.mark.parametrize("name", ["e2e_a", "resync"])
def test_planes_within_the_bar(golden, pushed, oracle, name, dec):
    got = pushed[name, dec]
    half = int(got["cyc"][0][1]["half"])
    want, spec = truth_planes(got["iq"][:, half], 344)
    dev = got["pwr_samp"][half][:, :344].astype(np.float64)
    e = np.abs(dev - want).max() / want.max()
    print("pwr_samp %s dec %d: %.3e of the maximum" % (name, dec, e))
    assert e < T.OLD_BAR
    avg = golden["s_%s_pwr_sampavg" % name][half].astype(np.float64)
    ea = np.abs(got["pwr_sampavg"][half] - avg).max() / avg.max()
    print("pwr_sampavg %s dec %d: %.3e of the maximum" % (name, dec, ea))
    assert ea < T.OLD_BAR
    # the transform at fp32 accuracy: its magnitudes against the oracle's own fp32 transform on the same windowed inputs
    white = T.spectrum_errors(oracle.fft(T.white(512, 1), prec=0), T.dft(T.white(512, 1)))
    for i in (0, 100, 343):
        xin, y = spec[i]
        mag = np.roll(np.sqrt(dev[:, i]), -256)
        e_dev = np.abs(mag - np.abs(y)).max() / np.abs(y).max()
        e_ref = np.abs(np.abs(oracle.fft(xin, prec=0).astype(np.complex128)) - np.abs(y)).max() / np.abs(y).max()
        ok, bar = T.judge("wspr %s dec %d transform %d" % (name, dec, i), e_dev, e_ref, white[1])
        assert ok, (i, e_dev, bar)


@pytest.mark.parametrize("dec", [1, 2])
@pytest.mark.parametrize("name", ["e2e_a", "resync", "silence"])
def test_pushed_scenes_against_the_reference(golden, pushed, name, dec):
    """schedule, events and end state equal; i / q data equal (by digest); the row bytes within the bar of the reference's two builds;
    the candidates' shift0, drift0 and freq0 equal"""
    got, k = pushed[name, dec], "s_%s_" % name
    assert np.array_equal(got["ev"], golden[k + "ev"]) and np.array_equal(got["meta"], golden[k + "meta"])
    want_info = golden[k + "info"].copy()
    want_info[16] = dec
    assert np.array_equal(got["info"], want_info), (got["info"], want_info)
    assert W.digest(got["iq"].tobytes()) == bytes(golden[k + "iq_sha"])
    d = np.abs(got["rows"].astype(np.int32) - golden[k + "rows"].astype(np.int32))
    n, allowed = (d != 0).sum(axis=1), 2 * golden[k + "rows32_diff"] + 1
    line = "%s dec %d: %d of %d row bytes differ (most in a row %d, largest difference %d); the reference's two builds: %d" % (
        name, dec, n.sum(), d.size, n.max(), d.max(), golden[k + "rows32_diff"].sum())
    print(line)
    path = os.environ.get("KIWIGPU_WSPR_ROWS_OUT")
    if path:
        open(path, "a").write(line + "\n")
    assert (n <= allowed).all() and d.max() <= 1, line
    assert len(got["cyc"]) == golden[k + "cyc"].shape[0] == 1
    blk, cy = got["cyc"][0]
    _, half, npk, pk, cand = W.cycle_fields(golden[k + "cyc"][0])
    assert (blk, int(cy["half"]), int(cy["npk"])) == (int(golden[k + "cyc"][0][0]), half, npk)
    for r in range(npk):                                                  # (c)
        c = cy["cand"][r]
        assert (int(c["shift0"]), int(c["drift0"].view(np.int32)), int(c["freq0"].view(np.int32)), int(c["bin0"])) == (cand[r][1], cand[r][2], cand[r][0], cand[r][5]), (name, r)
    if name == "silence":
        assert npk == 0 and (got["rows"][:, 1:] == 0).all()


# ---- (d)
def same_run(a, b, what):
    for f in ("ev", "rows", "meta", "info", "pwr_sampavg", "pwr_samp", "iq"):
        assert a[f].tobytes() == b[f].tobytes(), (what, f)
    assert len(a["cyc"]) == len(b["cyc"])
    for (ba, ca), (bb, cb) in zip(a["cyc"], b["cyc"]):
        assert ba == bb and ca.tobytes() == cb.tobytes(), (what, "cycle end")


@pytest.fixture(scope="module")
def one_block(pool, ctx):
    out = {}
    for name in ("edges_sched", "resync"):
        q = Wspr(ctx, nconn=1)
        out[name] = run_script_dev(q, W.scripts()[name], pool)
        q.close()
    return out


def test_schedule_edges_equal_the_reference(golden, one_block):
    """edges_sched: a callback that ends a group in mid-block, two groups due in one callback, capture off and on again, a resync at the
    even minute before the cycle is full, the wait at didx >= TPOINTS, the callback that holds group 85"""
    got, k = one_block["edges_sched"], "s_edges_sched_"
    assert np.array_equal(got["ev"], golden[k + "ev"]) and np.array_equal(got["meta"], golden[k + "meta"]) and np.array_equal(got["info"], golden[k + "info"])
    assert W.digest(got["iq"].tobytes()) == bytes(golden[k + "iq_sha"])
    assert got["info"][8] > 0 and len(got["cyc"]) == 1                    # a cycle under way behind a cycle end


@pytest.mark.parametrize("most", [2, 7, 64])
@pytest.mark.parametrize("name", ["edges_sched", "resync"])
def test_any_partition_equals_one_block_pushes(pool, ctx, one_block, name, most):
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode()) + most))
    q = Wspr(ctx, nconn=1)
    got = run_script_dev(q, W.scripts()[name], pool, cut=lambda: int(rng.integers(1, most + 1)))
    q.close()
    assert got["calls"] < one_block[name]["calls"]
    same_run(got, one_block[name], (name, most))


def test_14_connections_at_unequal_phases_in_one_call(pool, ctx):
    """connection c joins c pushes late: in every call the 14 stand at different places of their cycles; each equals itself alone"""
    nconn, nb, ns, npush = 14, 3, 512, 20
    x = pool[W.AT["noise"]:][:ns * nb * (npush + nconn)].reshape(-1, nb, ns)
    q = Wspr(ctx, nconn=nconn)
    rows = {c: [] for c in range(nconn)}
    for c in range(nconn):
        q.init(c, 375.0)
        q.set_capture(c, 1)
    for p in range(npush):
        live = [c for c in range(nconn) if p >= c]
        iq = np.stack([x[p - c] for c in live])
        rb, m, e, cy, counts = q.push(live, iq, 1, 0)                     # an odd minute: free running
        assert counts[:, 0].sum() == m.size
        for r in m:
            rows[int(r["conn"])].append((p - int(r["conn"]), int(r["blk"]), int(r["group"]), rb[int(r["off"]):int(r["off"]) + 412].tobytes()))
    for c in (0, 5, 13):
        alone = Wspr(ctx, nconn=1)                                        # a fresh object: what a connection has not reached yet is zeros
        alone.init(0, 375.0)
        alone.set_capture(0, 1)
        want = []
        for p in range(npush - c):
            rb, m, e, cy, counts = alone.push([0], x[p][None], 1, 0)
            want += [(p, int(r["blk"]), int(r["group"]), rb[int(r["off"]):int(r["off"]) + 412].tobytes()) for r in m]
        assert rows[c] == want and len(want) == 3 * (npush - c) - 1, c
        a, b = q.state(c, planes=True, samples=True), alone.state(0, planes=True, samples=True)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), c
        alone.close()
    q.close()


def test_refusals_change_nothing(pool, ctx):
    q = Wspr(ctx, nconn=2)
    x = pool[W.AT["noise"]:][:1024].reshape(1, 2, 512)
    with pytest.raises(KiwiGpuError):
        q.push([0], x, 0, 0)                                              # before init
    for bad in (374.0, float("nan"), float("inf")):
        with pytest.raises(KiwiGpuError):
            q.init(0, bad)
    q.init(0, 375.0)
    q.set_capture(0, 1)
    before = q.state(0, planes=True, samples=True)
    with pytest.raises(KiwiGpuError):
        q.set_type(0, 3)
    for mi, se in ((60, 0), (0, 60), (-1, 0)):
        with pytest.raises(KiwiGpuError):
            q.push([0], x, [[0, mi]], [[0, se]])                          # the second block's time: the first is not taken either
    after = q.state(0, planes=True, samples=True)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(before, after))
    assert q.plan([0], [2], 512, 0, 0) == (3, 1, 3, 0)                    # a clear, one copy run, a group; the pending IDLE and SYNC and the RUNNING of the sync
    rb, m, e, cy, counts = q.push([0], x, 0, 0)
    assert m.size == 1 and [int(v["a"]) for v in e] == [wspr.IDLE, wspr.SYNC, wspr.RUNNING] and q.state(0)[0]["didx"] == 1024
    q.close()
