"""What the FFT-extension tests share (tests/test_fftext_cpu.py, test_fftext_gpu.py, tools/make_ref_fftext_golden.py): the seeded pool
of 1024-point spectra that tests/golden/fftext_ref.npz was made from (the file holds the pool's digest, not the spectra), the command
/ block scripts, the limiter's clock scripts, the parser of what the reference harness and the host driver write, the host driver
tools/fftext_host_driver.cpp (csrc/kg_fftext.h compiled for the host with the reference's flags) and the runner of a script on the
device object.

No spectrum of the pool holds a NaN: (int) NaN is undefined in the reference, so NaN input is outside the row's contract."""
import os
import subprocess

import numpy as np

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W, MAX_BINS = 1024, 200
SEED = 0x46465445
OFF, WF, SPEC, INTEG = -1, 0, 1, 2
PASSBAND, CHAN_NULL = 0, 1
USB, SAM, QAM = 2, 11, 15                       # the reference's mode_e numbers (rx/mode.h:69-70)
# FFT.cpp:211 (a float denominator under a double quotient) times the three boosts (the golden decides; these only place the edge set)
_S0 = np.float32(20.0 / float(np.float32(32767.0) * np.float32(32767.0) * np.float32(1024.0) * np.float32(1024.0)))
SCALES = {"1e4": np.float32(_S0 * np.float32(1e4)), "1e6": np.float32(_S0 * np.float32(1e6)), "100": np.float32(_S0 * np.float32(100.0))}
FFT_SEC = {12000: 1.0 / (12000.0 * 2 / 1024), 20250: 1.0 / (20250.0 * 2 / 1024)}


EDGE_STEPS = (-64, -16, -3, -1, 0, 1, 3, 16, 64)


def _edge(scale):
    """re with re * re * scale within a few ulps of 10^(k/10) for every integer k in -200..0: where the (int) truncation decides
    (tests/spec_common.py says why these nine steps).  Two rows."""
    out = []
    for k in range(-200, 1):
        re0 = np.float32(np.sqrt(10.0 ** (k / 10.0) / float(scale)))
        bits = int(re0.view(np.uint32))
        out += [np.uint32(bits + d).view(np.float32) for d in EDGE_STEPS]
    out = np.array(out, np.float32)
    pad = np.full(2 * W - out.size, out[-1], np.float32)
    return np.concatenate([out, pad]).reshape(2, W)


def pool():
    """-> (names, complex64 [rows, 1024]).  One generator, drawn in a fixed order."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    names, rows = [], []

    def add(name, re, im):
        names.append(name)
        c = np.empty(W, np.complex64)               # (not re + 1j * im: an infinite part would make the other one NaN)
        c.real, c.imag = np.asarray(re, np.float32), np.asarray(im, np.float32)
        rows.append(c)

    # zeros; signs; denormals (and a power that underflows)
    re = np.zeros(W, np.float32)
    re[256:512] = rng.choice([-1.0, 1.0], 256) * rng.uniform(0.5, 2000.0, 256)
    re[512:640] = rng.choice([-1.0, 1.0], 128) * np.float32(1e-40) * rng.integers(1, 1000, 128)
    re[640:768] = rng.choice([-1.0, 1.0], 128) * 10.0 ** rng.uniform(-25, -15, 128)
    re[768:] = -0.0
    im = rng.standard_normal(W)
    im[:128] = 0.0
    add("zeros_signs_denormals", re, im)
    # |re|, |im| log-uniform over 1e-12 .. 1e12: floor and ceiling both reached
    for r in range(3):
        add("loguniform_%d" % r, rng.choice([-1.0, 1.0], W) * 10.0 ** rng.uniform(-12, 12, W), rng.choice([-1.0, 1.0], W) * 10.0 ** rng.uniform(-12, 12, W))
    # what a receiver hands over: both parts of comparable size, a few decades of level across the row -- the sums move at every addition
    for r in range(4):
        lvl = 10.0 ** rng.uniform(1, 5, W)
        add("signal_%d" % r, lvl * rng.standard_normal(W), lvl * rng.standard_normal(W))
    # +-inf, powers and products that overflow to inf, re = 0 beside a large im
    re = rng.choice([-1.0, 1.0], W) * 10.0 ** rng.uniform(0, 6, W)
    im = rng.standard_normal(W)
    re[0:64] = np.inf
    re[64:128] = -np.inf
    re[128:192] = rng.choice([-1.0, 1.0], 64) * 10.0 ** rng.uniform(19.5, 38, 64)       # re * re = inf
    re[192:256] = rng.choice([-1.0, 1.0], 64) * np.float32(1.8e19)                     # re * re finite, the largest powers
    re[256:512] = 0.0
    im[256:512] = rng.choice([-1.0, 1.0], 256) * 10.0 ** rng.uniform(6, 30, 256)
    im[504:512] = np.inf
    add("inf_overflow_zero_re", re, im)
    # the edge set after each of the three boosts; im = 0, so that re * re + im * im is the same power
    for k in ("1e4", "1e6", "100"):
        e = _edge(SCALES[k])
        for r in range(2):
            add("edge_%s_%d" % (k, r), e[r] * rng.choice([-1.0, 1.0], W).astype(np.float32), np.zeros(W, np.float32))
    spec = np.stack(rows)
    assert not np.isnan(spec.real).any() and not np.isnan(spec.imag).any()
    return names, spec


def load():
    return np.load(os.path.join(GOLD, "fftext_ref.npz"))


# ---- the scripts.  R rate | S run isSAM mode | I itime | C | B inst k   (tools/ref/ref_fftext_main.cpp)
NPOOL = 15
FULL = ("wf", "spec", "spec_sam", "integ_bins3", "wf_to_integ")      # rows kept in full; the others by digest


def _B(ks, inst=PASSBAND):
    return ["B %d %d" % (inst, k % NPOOL) for k in ks]


def scripts():
    allp = range(NPOOL)
    sig = [4, 5, 6, 7, 1, 0, 4, 6, 5, 7, 2, 4]               # twelve blocks: the signal rows, a log-uniform one, the zeros
    s = {
        # each function and each boost case over the whole pool
        "wf": ["R 12000", "S 0 0 %d" % USB] + _B(allp),
        "spec": ["R 12000", "S 1 0 %d" % USB] + _B(allp),
        "spec_sam": ["R 12000", "S 1 1 %d" % SAM] + [l for k in allp for l in (_B([k]) + _B([k], CHAN_NULL))],      # passband blocks ignored
        "spec_qam": ["R 12000", "S 1 1 %d" % QAM] + _B(allp, CHAN_NULL),
        "integ_pool": ["R 12000", "I 3.0", "S 2 0 %d" % USB] + _B(allp),                                         # bins 70: a bin per block
        "integ_sam": ["R 12000", "I 0.13", "S 2 1 %d" % SAM] + _B(sig[:6]) + _B(sig[:2], CHAN_NULL),            # integ stays on the passband
        # bins = 3 over 12 blocks: 0.13 s / 42.67 ms = 3.05
        "integ_bins3": ["R 12000", "I 0.13", "S 2 0 %d" % USB] + _B(sig),
        "integ_bins3_20250": ["R 20250", "I 0.08", "S 2 0 %d" % USB] + _B(sig),                                  # 0.08 s / 25.28 ms = 3.16
        "wf_20250": ["R 20250", "S 0 0 %d" % USB, "C"] + _B(sig[:4]),
        "integ_bins0": ["R 12000", "I 0.01", "S 2 0 %d" % USB] + _B(sig[:6]),
        # bins = 205 over 210 blocks: bins 200 .. 204 are dropped while fi goes on, then the wrap
        "integ_bins205": ["R 12000", "I 8.768", "S 2 0 %d" % USB] + _B(range(210)),
        "clear_itime_mid": ["R 12000", "I 0.13", "S 2 0 %d" % USB] + _B(sig[:6]) + ["C"] + _B(sig[6:10]) + ["I 0.2"] + _B(sig[:5]) + ["C", "C"] + _B(sig[:2]),
        # the function changed without a clear: the stale pwr[0], ncma and fi carry over
        "wf_to_integ": ["R 12000", "I 0.13", "S 2 0 %d" % USB] + _B(sig[:4]) + ["S 0 0 %d" % USB] + _B(sig[4:6]) + ["S 2 0 %d" % USB] + _B(sig[6:11]),
        "interleaved": ["R 12000", "I 0.13", "S 2 0 %d" % USB] + [l for k in sig[:8] for l in (_B([k]) + _B([k + 1], CHAN_NULL))],
        "off_on": ["R 12000", "S 0 0 %d" % USB] + _B([4]) + ["S -1 0 %d" % USB] + _B([5, 6]) + ["S 1 0 %d" % USB] + _B([5]) + ["I 0.5"] + _B([6, 7]),
        "rate_change": ["R 12000", "I 0.13", "S 2 0 %d" % USB] + _B(sig[:4]) + ["R 20250"] + _B(sig[4:8]) + ["C"] + _B(sig[8:12]),      # captured at the reset only
    }
    return s


def limiter_scripts():
    blk12k, blk20k = 512 / 12000.0 * 1e3, 512 / 20250.0 * 1e3      # 42.67 and 25.28 ms a block
    return {
        "first_at_100": [100, 101, 150, 201, 202, 301, 302],
        "first_below": [0, 1, 60, 99, 100, 105, 204, 205, 206],
        "first_above": [101, 102, 201, 202, 250, 302],
        "cadence_42_67": [int(1000 + k * blk12k) for k in range(60)],
        "cadence_25_28": [int(777 + k * blk20k) for k in range(100)],
        "long_gap": [int(500 + k * blk12k) for k in range(12)] + [int(5000 + k * blk12k) for k in range(40)],
        "wraps": [4294967000, 4294967100, 4294967200, 4294967290, 5, 100, 200],
    }


STATE_BYTES = 16 + 8 + 24 + 4 * MAX_BINS + 4 * MAX_BINS * W


def parse(raw, nblocks):
    """out.bin of the reference harness or the host driver -> dict: sent int32 [nblocks], bins int32 [rows], rows uint8 [rows, 1024],
    and the final state (run, instance, nbins, reset, fft_scale, spectrum_scale, fi, fft_sec, time, ncma int32 [200], pwr float32 [200, 1024])"""
    at, sent, bins, rows = 0, [], [], []
    for _ in range(nblocks):
        s = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        sent.append(s)
        if s:
            bins.append(int(np.frombuffer(raw[at:at + 4], np.int32)[0]))
            rows.append(np.frombuffer(raw[at + 4:at + 4 + W], np.uint8))
            at += 4 + W
    assert len(raw) - at == STATE_BYTES, (len(raw), at)
    iv = np.frombuffer(raw[at:at + 16], np.int32)
    fv = np.frombuffer(raw[at + 16:at + 24], np.float32)
    dv = np.frombuffer(raw[at + 24:at + 48], np.float64)
    ncma = np.frombuffer(raw[at + 48:at + 48 + 4 * MAX_BINS], np.int32).copy()
    pwr = np.frombuffer(raw[at + 48 + 4 * MAX_BINS:], np.float32).reshape(MAX_BINS, W).copy()
    return {"sent": np.array(sent, np.int32), "bins": np.array(bins, np.int32), "rows": np.array(rows, np.uint8).reshape(-1, W),
            "run": int(iv[0]), "instance": int(iv[1]), "nbins": int(iv[2]), "reset": int(iv[3]), "fft_scale": np.float32(fv[0]),
            "spectrum_scale": np.float32(fv[1]), "fi": float(dv[0]), "fft_sec": float(dv[1]), "time": float(dv[2]), "ncma": ncma, "pwr": pwr}


def row_digests(rows):
    return np.array([np.frombuffer(digest(r.tobytes()), np.uint8) for r in rows], np.uint8).reshape(-1, 16)


def nblocks(lines):
    return sum(1 for l in lines if l[0] == "B")


def check_against_golden(g, name, got):
    """got: what parse() answers, or the same keys from a device run.  Equality on everything the golden keeps."""
    k = "s_%s_" % name
    assert np.array_equal(got["sent"], g[k + "sent"]), (name, "sent", got["sent"], g[k + "sent"])
    assert np.array_equal(got["bins"], g[k + "bins"]), (name, "bins", got["bins"], g[k + "bins"])
    assert got["rows"].shape[0] == g[k + "bins"].size, name
    if k + "rows" in g.files:
        bad = np.argwhere(got["rows"] != g[k + "rows"])
        assert bad.size == 0, (name, "first differing byte (row, column)", bad[0], int(got["rows"][tuple(bad[0])]), int(g[k + "rows"][tuple(bad[0])]))
    d = row_digests(got["rows"])
    bad = np.flatnonzero((d != g[k + "row_sha"]).any(axis=1))
    assert bad.size == 0, (name, "first differing row", int(bad[0]))
    st = g[k + "state"]
    assert (got["run"], got["instance"], got["nbins"], got["reset"]) == tuple(int(v) for v in st), (name, "state", st)
    assert np.array_equal(np.array([got["fft_scale"], got["spectrum_scale"]], np.float32).view(np.uint32), g[k + "scales"].view(np.uint32)), (name, "scales")
    assert np.array_equal(np.array([got["fi"], got["fft_sec"], got["time"]], np.float64).view(np.uint64), g[k + "times"].view(np.uint64)), \
        (name, "fi, fft_sec, time", got["fi"], got["fft_sec"], got["time"], g[k + "times"])
    assert np.array_equal(got["ncma"], g[k + "ncma"]), (name, "ncma")
    assert digest(got["pwr"].tobytes()) == bytes(g[k + "pwr_sha"]), (name, "sums")
    if k + "pwr_head" in g.files:
        h = g[k + "pwr_head"]
        assert np.array_equal(got["pwr"][:h.shape[0]].view(np.uint32), h.view(np.uint32)), (name, "sums of the leading bins")


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "fftext_host_driver")


def run_script_exe(exe, lines, spec, tmpdir, expect=0):
    out = script_common.run_script(exe, ["script"], lines, spec, np.complex64, tmpdir, expect)
    return parse(out, nblocks(lines)) if expect == 0 else None


def run_limiter_exe(exe, clocks, tmpdir):
    """-> (sent int32 [n], last_ms uint32 [n])"""
    P = lambda f: os.path.join(str(tmpdir), f)
    np.array(clocks, np.uint32).tofile(P("clk.bin"))
    subprocess.run([exe, "limiter", P("clk.bin"), P("out.bin")], check=True)
    a = np.fromfile(P("out.bin"), np.uint32).reshape(-1, 2)
    return a[:, 0].astype(np.int32), a[:, 1].copy()


# ---- a script on the device object
def run_script_dev(fx, ctx, lines, spec, cuts=None, row_stride=W, fill=0xAA, merge=False):
    """Runs a script on channel 0 of fx (a FftExt): consecutive B lines are ONE kg_fftext_process_dev call of one entry per line -- or
    with `merge` one entry per run of lines of one instance --, cut where a command stands between them and after the block counts in
    `cuts` (block numbers of the script).  -> the keys of parse(),
    plus "calls", and "pad": whether every byte of the row buffer outside the rows still holds `fill`."""
    nb = nblocks(lines)
    d_rows = ctx.alloc(max(nb, 1) * row_stride)
    d_spec = [0, 0]                                  # a call gathers its blocks: the buffer and its bytes, grown to the largest call
    host_rows = np.full((max(nb, 1), row_stride), fill, np.uint8)
    sent, bins, calls, at, seen = np.zeros(nb, np.int32), [], 0, 0, 0
    cuts = set(cuts or ())
    pend = []

    def flush():
        nonlocal at, calls
        if not pend:
            return
        ents = []                                    # [instance, [positions in pend]]
        for i, p in enumerate(pend):
            if merge and ents and ents[-1][0] == p[0]:
                ents[-1][1].append(i)
            else:
                ents.append([p[0], [i]])
        # entry i reads its spectra from i * spec_stride on, so the blocks are gathered per call (one entry per block: back to back)
        most = max(len(e[1]) for e in ents)
        blocks = np.zeros((len(ents), most, W), np.complex64)
        for i, e in enumerate(ents):
            blocks[i, :len(e[1])] = spec[[pend[j][1] for j in e[1]]]
        if blocks.nbytes > d_spec[1]:                # (the call before has drained: every call ends in a sync)
            if d_spec[0]:
                ctx.free(d_spec[0])
            d_spec[0], d_spec[1] = 0, 0
            d_spec[0], d_spec[1] = ctx.alloc(blocks.nbytes), blocks.nbytes
        ctx.upload(d_spec[0], blocks)
        m = fx.process_dev([0] * len(ents), [len(e[1]) for e in ents], [e[0] for e in ents], d_spec[0], most * W, d_rows + at * row_stride, row_stride, len(pend))
        ctx.sync()                                   # the next call's upload reuses d_spec
        for ch, ent, blk, b in m:
            assert ch == 0 and (merge or blk == 0)
            bins.append(int(b))
            sent[pend[ents[ent][1][blk]][2]] = 1
        at += m.shape[0]
        calls += 1
        pend.clear()

    try:
        ctx.upload(d_rows, host_rows)
        for l in lines:
            op = l[0]
            if op == "B":
                _, inst, k = l.split()
                pend.append((int(inst), int(k), seen))
                seen += 1
                if seen in cuts:
                    flush()
                continue
            flush()
            if op == "R":
                fx.set_rate(float(l[2:]))
            elif op == "S":
                run, sam, mode = (int(v) for v in l[2:].split())
                fx.set_run(0, run, sam != 0, mode == QAM)
            elif op == "I":
                fx.set_itime(0, float(l[2:]))
            elif op == "C":
                fx.clear(0)
        flush()
        ctx.sync()
        ctx.download(d_rows, host_rows)
    finally:
        if d_spec[0]:
            ctx.free(d_spec[0])
        ctx.free(d_rows)
    info, ncma, pwr = fx.state(0, sums=True)
    n = len(bins)
    pad = bool((host_rows[:n, W:] == fill).all() and (host_rows[n:] == fill).all())
    return {"sent": sent, "bins": np.array(bins, np.int32), "rows": host_rows[:n, :W].copy(), "run": int(info["run"]), "instance": int(info["instance"]),
            "nbins": int(info["bins"]), "reset": int(info["reset"]), "fft_scale": np.float32(info["fft_scale"]),
            "spectrum_scale": np.float32(info["spectrum_scale"]), "fi": float(info["fi"]), "fft_sec": float(info["fft_sec"]), "time": float(info["time"]),
            "ncma": ncma, "pwr": pwr, "calls": calls, "pad": pad}
