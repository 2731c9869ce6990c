"""What the FAX tests share (tests/test_fax_cpu.py, test_fax_gpu.py, test_fax_bank_gpu.py, tools/make_ref_fax_golden.py): the seeded
pool of 16-bit audio that tests/golden/fax_ref.npz was made from (the file holds the pool's digest, not the samples), the command /
block scripts, the parser of what the reference harness and the host driver write, the host driver tools/fax_host_driver.cpp
(csrc/kg_fax.h compiled for the host with the reference's flags) and the runner of a script on the device object.

A fax signal here is an FM tone at 1900 Hz +- 400 Hz (black 1500, white 2300), amplitude 9000, under Gaussian noise; a segment is a
list of (kind, lines): image lines, the 300 Hz start tone and the 450 Hz stop tone as black / white square waves, phasing lines of 95 %
black with a 5 % white pulse (or the opposite polarity) rotated by some samples."""
import os

import numpy as np

from flydog_sdr_gps_amd.fax import info_dtype, rec_dtype

from . import script_common
from .script_common import digest, script_steps  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 0x46415821
BLK = 512
MAX_SPL = 24576
ROTATE = 1234

# name -> (sample rate, lpm, noise sigma, [(kind, lines)])
SEGMENTS = (
    ("a120", 12000, 120, 300.0, [("image", 4), ("start", 12), ("phasing", 44), ("image", 12), ("stop", 12), ("image", 8), ("start", 12), ("image", 5)]),
    ("rev120", 12000, 120, 300.0, [("image", 2), ("start", 12), ("phasing_rev", 44), ("image", 4)]),
    ("a240", 12000, 240, 200.0, [("image", 3), ("start", 22), ("phasing", 44), ("image", 8), ("stop", 22), ("image", 3)]),
    ("a60", 12000, 60, 200.0, [("image", 1), ("start", 4), ("phasing", 44), ("image", 3), ("stop", 4), ("image", 2)]),
    ("a90", 12000, 90, 200.0, [("image", 2), ("start", 8), ("image", 4), ("stop", 8), ("image", 2)]),
    ("a60_20250", 20250, 60, 200.0, [("image", 1), ("start", 4), ("phasing", 44), ("image", 2)]),
    ("zeros", 12000, 120, 0.0, [("zero", 4)]),
)
AT, NBLK, POOL = {}, {}, 0
for _name, _fs, _lpm, _sig, _plan in SEGMENTS:
    _n = sum(l for _, l in _plan) * (_fs * 60 // _lpm)
    AT[_name] = POOL
    NBLK[_name] = (_n + BLK - 1) // BLK
    POOL += NBLK[_name] * BLK

assert rec_dtype.itemsize == 48 and info_dtype.itemsize == 472
IMAGE, START, STOP = 0, 1, 2
F_SPS_CHANGED, F_AUTOSTOPPED_0, F_AUTOSTOPPED_1, F_PHASED, F_ROW_SENT, F_PHASING_REJECTED, F_MEDIAN = 1, 2, 4, 8, 16, 32, 64


def _brightness(kind, n, spl, fs, lpm, line0):
    """brightness 0 .. 1 of n samples that begin at line line0 of the segment"""
    t = np.arange(n)
    pos = (t % spl) / spl
    line = line0 + t // spl
    if kind == "image":
        return 0.5 + 0.35 * np.sin(2 * np.pi * (3 * pos + 0.11 * line)) + 0.1 * ((pos * 16).astype(np.int64) % 2)
    if kind in ("start", "stop"):
        hz = 300.0 if kind == "start" else 450.0
        return ((t * hz / fs) % 1.0 < 0.5).astype(np.float64)
    if kind == "phasing":
        return (((t + spl - ROTATE) % spl) / spl < 0.05).astype(np.float64)
    if kind == "phasing_rev":
        return 1.0 - (((t + spl - ROTATE) % spl) / spl < 0.05).astype(np.float64)
    raise ValueError(kind)


_pool = None


def pool():
    """-> int16 [POOL].  One generator, drawn in a fixed order; built once a process."""
    global _pool
    if _pool is not None:
        return _pool
    rng = np.random.Generator(np.random.PCG64(SEED))
    out = np.zeros(POOL, np.int16)
    for name, fs, lpm, sigma, plan in SEGMENTS:
        spl = fs * 60 // lpm
        if plan[0][0] == "zero":
            continue
        b, line0 = [], 0
        for kind, lines in plan:
            b.append(_brightness(kind, lines * spl, spl, fs, lpm, line0))
            line0 += lines
        b = np.concatenate(b)
        hz = 1900.0 + 400.0 * (2.0 * np.clip(b, 0, 1) - 1.0)
        ph = 2 * np.pi * np.cumsum(hz) / fs
        x = 9000.0 * np.cos(ph) + sigma * rng.standard_normal(b.size)
        out[AT[name]:AT[name] + b.size] = np.round(x).astype(np.int16)
    out.setflags(write=False)
    _pool = out
    return out


def load():
    return np.load(os.path.join(GOLD, "fax_ref.npz"))


# ---- the scripts.  C lpm imagewidth carrier deviation bandwidth headers phasing autostop debug nom srate | R srate | H shift | T | B off
def _B(seg, first, n):
    assert first + n <= NBLK[seg], (seg, first, n)
    return ["B %d" % (AT[seg] + BLK * (first + k)) for k in range(n)]


def _C(lpm, w=1024, car=1900, dev=400, bw=1, hdr=1, ph=1, stop=1, dbg=0, nom=12000, srate=None):
    return "C %d %d %d %d %d %d %d %d %d %d %r" % (lpm, w, car, dev, bw, hdr, ph, stop, dbg, nom, float(nom if srate is None else srate))


def scripts():
    s = {
        # the whole story at the reference's own parameters: start, phasing, phased, stop, a second start behind the stop
        "nominal_120": [_C(120)] + _B("a120", 0, NBLK["a120"]),
        # a rate ratio above 1 through the phasing
        "rate_hi_120": [_C(120, srate=12001.37)] + _B("a120", 0, 760),
        # a ratio below 1 arriving in mid-stream (fax_sps_changed), no autostop
        "rate_lo_120": [_C(120, stop=0)] + _B("a120", 0, 100) + ["R 11998.9"] + _B("a120", 100, 200),
        # phasing lines of the opposite polarity: rejected by the 10 % / 90 % spread
        "reverse_rejected": [_C(120, bw=2)] + _B("rev120", 0, NBLK["rev120"]),
        # no phasing, autostop, no headers: stop tone, counted lines, the second start tone, then rows blended with the zero line
        "p0a1_120": [_C(120, hdr=0, ph=0)] + _B("a120", 690, NBLK["a120"] - 690),
        # neither: header detection is skipped; debug rows; other carrier, deviation and filter
        "p0a0_debug": [_C(120, car=1800, dev=450, bw=2, ph=0, stop=0, dbg=1)] + _B("a120", 0, 60),
        # 240 lpm: the detector's cap of 3000 exactly; no headers: rows only behind the phasing
        "lpm240_hdr0": [_C(240, hdr=0, stop=0)] + _B("a240", 0, NBLK["a240"]),
        "lpm60": [_C(60, bw=0)] + _B("a60", 0, NBLK["a60"]),
        # 90 lpm: typecount == 3.5 never holds; an image wider than pi * 576 (a row a line, every one blended)
        "lpm90_w1900": [_C(90, w=1900)] + _B("a90", 0, NBLK["a90"]),
        # the longest line: 60 lpm at 20250 Hz
        "lpm60_20250": [_C(60, nom=20250, srate=20250.77)] + _B("a60_20250", 0, NBLK["a60_20250"]),
        # shifts in mid-stream: a part of a line, then a whole line (a skip larger than a block)
        "shift_mid": [_C(120, w=640)] + _B("a120", 0, 30) + ["H 0.37"] + _B("a120", 30, 30) + ["H 1.0"] + _B("a120", 60, 40),
        # a restart in mid-line with a skip pending: Iprev, Qprev, m_lineBlend, m_skip and frac_prev are carried over
        "restart_mid_line": [_C(120, srate=12000.5)] + _B("a120", 0, 40) + ["H 0.9"] + _B("a120", 40, 3) + [_C(240, w=512, ph=0)] + _B("a120", 43, 60)
                            + ["T"] + _B("a120", 103, 4) + [_C(120)] + _B("a120", 107, 30),
        # silence, then signal: NaN pixels as byte 0, then Iprev / Qprev recover
        "silence_then_signal": [_C(120, ph=0)] + _B("zeros", 0, 40) + _B("a120", 0, 50),
        # a skip of 73 samples at 3000 a line: six blocks end ONE sample short of the first line, which completes on the seventh's first
        "one_short_240": [_C(240, w=800, ph=0, stop=0), "H 0.0245"] + _B("a240", 0, 20),
        # all-zero audio runs to rows of zeros; the end state holds the NaN
        "all_zero": [_C(240, ph=0, stop=0)] + _B("zeros", 0, 30),
    }
    return s


def nblocks(lines):
    return sum(1 for l in lines if l[0] == "B")


def last_config(lines):
    """(spl, imagewidth) behind the script's last C"""
    c = [l for l in lines if l[0] == "C"][-1].split()
    return int(float(c[10]) * 60.0 / int(c[1])), int(c[2])


def parse(raw, lines):
    """out.bin of the reference harness or the host driver -> dict: nlines int32 [blocks], recs (rec_dtype [lines]), rows (list of uint8
    arrays, one per record with the row flag), info (one record of info_dtype), samples, demod, prev, out"""
    at, nl, recs, rows = 0, [], [], []
    for _ in range(nblocks(lines)):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        nl.append(n)
        for _ in range(n):
            r = np.frombuffer(raw[at:at + 48], rec_dtype)[0]
            at += 48
            recs.append(r)
            if int(r["flags"]) & F_ROW_SENT:
                w = rows_width(lines, len(nl) - 1)
                rows.append(np.frombuffer(raw[at:at + 1 + w], np.uint8))
                at += 1 + w
    info = np.frombuffer(raw[at:at + info_dtype.itemsize], info_dtype)[0].copy()
    at += info_dtype.itemsize
    spl, w = int(info["spl"]), int(info["imagewidth"])
    assert len(raw) - at == 3 * spl + 2 * w, (len(raw), at, spl, w)
    return {"nlines": np.array(nl, np.int32), "recs": np.array(recs, rec_dtype), "rows": rows, "info": info,
            "samples": np.frombuffer(raw[at:at + 2 * spl], np.int16).copy(), "demod": np.frombuffer(raw[at + 2 * spl:at + 3 * spl], np.uint8).copy(),
            "prev": np.frombuffer(raw[at + 3 * spl:at + 3 * spl + w], np.uint8).copy(), "out": np.frombuffer(raw[at + 3 * spl + w:], np.uint8).copy()}


def rows_width(lines, block):
    """the imagewidth in force at block number `block` of the script"""
    w, seen = None, 0
    for l in lines:
        if l[0] == "C":
            w = int(l.split()[2])
        elif l[0] == "B":
            if seen == block:
                return w
            seen += 1
    raise IndexError(block)


def all_bytes(got):
    return np.concatenate([np.asarray(r, np.uint8) for r in got["rows"]]) if got["rows"] else np.zeros(0, np.uint8)


def golden_of(got):
    """what the golden file keeps of a reference run: everything"""
    return {"nlines": got["nlines"], "recs": np.frombuffer(got["recs"].tobytes(), np.int32).reshape(-1, 12), "rows": all_bytes(got),
            "info": np.frombuffer(got["info"].tobytes(), np.uint8), "samples": got["samples"], "demod": got["demod"], "prev": got["prev"], "out": got["out"]}


def _same_float(a, b):
    """bit for bit, a NaN equal to any NaN (the device's is the positive quiet one, x86's the negative)"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a.view(a.dtype.str.replace("f", "u")) == b.view(b.dtype.str.replace("f", "u"))) | (np.isnan(a) & np.isnan(b))))


def check_against_golden(g, name, got):
    """equality on everything: the lines of every block, every record, every row byte and the end state bit for bit"""
    k = "s_%s_" % name
    assert np.array_equal(got["nlines"], g[k + "nlines"]), (name, "lines per block", np.flatnonzero(got["nlines"] != g[k + "nlines"])[:8])
    want = np.frombuffer(np.ascontiguousarray(g[k + "recs"]).tobytes(), rec_dtype)
    have = got["recs"]
    assert have.size == want.size, (name, have.size, want.size)
    for f in rec_dtype.names:
        if f == "blk":
            continue
        bad = np.flatnonzero(have[f] != want[f])
        assert bad.size == 0, (name, "record field", f, "first differing line", int(bad[0]), int(have[f][bad[0]]), int(want[f][bad[0]]), int(bad.size))
    allb = all_bytes(got)
    assert allb.size == g[k + "rows"].size, (name, allb.size, g[k + "rows"].size)
    bad = np.flatnonzero(allb != g[k + "rows"])
    assert bad.size == 0, (name, "first differing row byte", int(bad[0]), int(allb[bad[0]]), int(g[k + "rows"][bad[0]]), int(bad.size))
    winfo = np.frombuffer(g[k + "info"].tobytes(), info_dtype)[0]
    for f in info_dtype.names:
        if f == "pad":
            continue
        a, b = np.asarray(got["info"][f]), np.asarray(winfo[f])
        same = _same_float(a, b) if a.dtype.kind == "f" else np.array_equal(a, b)
        assert same, (name, "state", f, a, b)
    for f in ("samples", "demod", "prev", "out"):
        a, b = np.asarray(got[f]), g[k + f]
        assert a.shape == b.shape, (name, f, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (name, f, "first differing entry", int(bad[0]), int(a[bad[0]]), int(b[bad[0]]), int(bad.size))


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "fax_host_driver")


def run_script_exe(exe, lines, samples, tmpdir, expect=0, keep_on=False):
    out = script_common.run_script(exe, ["-k"] if keep_on else [], lines, samples, np.int16, tmpdir, expect)
    return parse(out, lines) if expect == 0 else None


# ---- a script on the device object
class Recorder:
    """what a script leaves, in the keys of parse(): lines are added push by push"""

    def __init__(self, nblk):
        self.nlines = np.zeros(nblk, np.int32)
        self.recs, self.rows = [], []

    def add(self, blocks, recs, rows, width):
        """blocks: the script's block number of each block of the push; recs / rows: ONE connection's, in order"""
        k = 0
        for r in recs:
            self.nlines[blocks[int(r["blk"])]] += 1
            r = r.copy()
            r["blk"] = 0
            self.recs.append(r)
            if int(r["flags"]) & F_ROW_SENT:
                self.rows.append(np.asarray(rows[k][:1 + width]).copy())
                k += 1
        assert k == len(rows), (k, len(rows))

    def result(self, state):
        out = {"nlines": self.nlines, "recs": np.array(self.recs, rec_dtype), "rows": self.rows}
        out.update(state)
        return out


def state_of(q, conn):
    info, samples, demod, prev, out = q.state(conn)
    spl, w = int(info["spl"]), int(info["imagewidth"])
    return {"info": info, "samples": samples[:spl], "demod": demod[:spl], "prev": prev[:w], "out": out[:w]}


def apply_command(q, conn, l, rate):
    """-> the rate in force behind the command"""
    a = l.split()
    if a[0] == "C":
        v = [int(x) for x in a[1:10]]
        q.start(conn, lpm=v[0], imagewidth=v[1], carrier=v[2], deviation=v[3], bandwidth=v[4], include_headers=v[5], phasing=v[6], autostop=v[7], debug=v[8],
                nom_rate=float(a[10]), srate=float(a[11]))
        return float(a[11])
    if a[0] == "R":
        return float(a[1])
    if a[0] == "H":
        q.set_shift(conn, float(a[1]))
    elif a[0] == "T":
        q.stop(conn)
    else:
        raise ValueError(l)
    return rate


def _items(lines):
    out, seen = [], 0
    for l in lines:
        if l[0] == "B":
            out.append(("blk", int(l.split()[1]), seen))
            seen += 1
        else:
            out.append(("cmd", l))
    return out


def run_side_by_side(q, scripts, samples, rng, most=24):
    """scripts[c] on connection c of q (a FaxDecoder), in lockstep: every round each script takes its commands up to its next block,
    then ONE push feeds every connection with blocks left, 1 to `most` consecutive blocks each (drawn from rng, a numpy Generator),
    listed out of connection order.  Nothing of the schedule depends on what the device answers: with q None only the schedule is
    walked.  -> (per script the keys of parse() -- None without q --, pushes, pushes that carried more than one connection)"""
    items = [_items(s) for s in scripts]
    at, rate, width = [0] * len(items), [0.0] * len(items), [0] * len(items)
    rec = [Recorder(nblocks(s)) for s in scripts]
    shared = calls = 0
    while any(a < len(it) for a, it in zip(at, items)):
        for c, it in enumerate(items):
            while at[c] < len(it) and it[at[c]][0] == "cmd":
                if q is not None:
                    rate[c] = apply_command(q, c, it[at[c]][1], rate[c])
                if it[at[c]][1][0] == "C":
                    width[c] = int(it[at[c]][1].split()[2])
                at[c] += 1
        take = {}
        for c, it in enumerate(items):
            n = 0
            lim = int(rng.integers(1, most + 1))
            while n < lim and at[c] + n < len(it) and it[at[c] + n][0] == "blk":
                n += 1
            if n:
                take[c] = it[at[c]:at[c] + n]
        if not take:
            break
        conns = sorted(take, key=lambda c: -c)
        if q is not None:
            x = np.zeros((len(conns), max(len(v) for v in take.values()), BLK), np.int16)
            for e, c in enumerate(conns):
                for b, (_, off, _) in enumerate(take[c]):
                    x[e, b] = samples[off:off + BLK]
            recs, rows = q.push(conns, x, [rate[c] for c in conns], nblk=[len(take[c]) for c in conns])
        for e, c in enumerate(conns):
            if q is not None:
                rec[c].add([b for _, _, b in take[c]], recs[e], rows[e], width[c])
            at[c] += len(take[c])
        shared += len(conns) > 1
        calls += 1
    return [rec[c].result(state_of(q, c)) if q is not None else None for c in range(len(scripts))], calls, shared


def run_script_dev(q, lines, samples, conn=0, cuts=lambda: 64):
    """Runs a script on connection conn of q (a FaxDecoder): every push one call.  -> the keys of parse(), and "calls"."""
    rec, calls, rate, width = Recorder(nblocks(lines)), 0, 0.0, 0
    for st in script_steps(lines, cuts):
        if st[0] == "cmd":
            rate = apply_command(q, conn, st[1], rate)
            if st[1][0] == "C":
                width = int(st[1].split()[2])
            continue
        _, offs, blocks = st
        x = np.stack([samples[o:o + BLK] for o in offs])[None]
        recs, rows = q.push([conn], x, [rate])
        rec.add(blocks, recs[0], rows[0], width)
        calls += 1
    out = rec.result(state_of(q, conn))
    out["calls"] = calls
    return out
