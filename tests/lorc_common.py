"""What the Loran-C tests share (tests/test_lorc_cpu.py, test_lorc_gpu.py, test_lorc_bank_gpu.py, tools/make_ref_lorc_golden.py): the
seeded pool of complex samples that tests/golden/lorc_ref.npz was made from (the file holds the pool's digest, not the samples), the
command / block scripts, the parser of what the reference harness and the host driver write, the host driver
tools/lorc_host_driver.cpp (csrc/kg_lorc.h compiled for the host with the reference's flags) and the runner of a script on the device
object.

Amplitudes stay at or below 3e4 and no sample is NaN or infinite: the contract of csrc/kg_lorc.h."""
import os

import numpy as np

from flydog_sdr_gps_amd.lorc import chan_dtype

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 0x4C4F5243
FS = 12000.0
GRI_A, GRI_B = 7980, 9960                        # two chains: 957.6 and 1195.2 samples a GRI at 12 kHz
MAX_BUCKET, MAX_NS = 1199, 512
SEGMENTS = (("loran", 120), ("noise", 48), ("silence_noise", 48))          # name, blocks of 512
AT, POOL = {}, 0
for _n, _b in SEGMENTS:
    AT[_n] = POOL
    POOL += 512 * _b
SILENCE = 3000                                   # leading zeros of "silence_noise", ending inside a block
SCALARS = 16 + 2 * 64
STATE_BYTES = SCALARS + 2 * MAX_BUCKET * 4

scalars_dtype = np.dtype([("i_srate", "<u4"), ("redraw_legend", "<i4"), ("srate", "<f8"), ("ch", chan_dtype, (2,))])
assert chan_dtype.itemsize == 64 and scalars_dtype.itemsize == SCALARS


def pool():
    """-> complex64 [POOL].  One generator, drawn in a fixed order."""
    rng = np.random.Generator(np.random.PCG64(SEED))

    def noise(n, sigma):
        return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))

    def chain(n, gri, amp, phase, t0):
        """groups of eight pulses a millisecond apart (the master's ninth left out), a pulse a short envelope over four samples"""
        x = np.zeros(n, np.complex128)
        env = np.array([0.35, 1.0, 0.6, 0.2])
        k = 0
        while True:
            t = t0 + k * gri * 1e-5
            if t * FS >= n:
                break
            for p in range(8):
                i = int(round((t + p * 1e-3) * FS))
                sign = 1.0 if (p + k) % 3 else -1.0                      # a phase code of sorts
                for j, ev in enumerate(env):
                    if i + j < n:
                        x[i + j] += sign * amp * ev * np.exp(1j * phase)
            k += 1
        return x

    out = {}
    n = 512 * dict(SEGMENTS)["loran"]
    out["loran"] = noise(n, 900.0) + chain(n, GRI_A, 9000.0, 0.7, 0.013) + chain(n, GRI_B, 6000.0, -1.1, 0.031)
    out["noise"] = noise(512 * dict(SEGMENTS)["noise"], 3000.0)
    s = noise(512 * dict(SEGMENTS)["silence_noise"], 2500.0)
    s[:SILENCE] = 0
    out["silence_noise"] = s
    p = np.concatenate([out[name] for name, _ in SEGMENTS]).astype(np.complex64)
    assert p.size == POOL and np.isfinite(p.view(np.float32)).all() and np.abs(p.real).max() <= 3e4 and np.abs(p.imag).max() <= 3e4
    return p


def load():
    return np.load(os.path.join(GOLD, "lorc_ref.npz"))


# ---- the scripts.  N srate i_srate | I ch gri | O ch offset | G ch gain | A ch algo | P ch param | S | T | B ns off
def _B(seg, first, n, ns=512):
    return ["B %d %d" % (ns, AT[seg] + ns * (first + k)) for k in range(n)]


CMA, EMA, IIR = 0, 1, 2


def _setup(srate, i_srate, gri, algo, param, gain=(0, 0), offset=(0, 0)):
    l = ["N %r %d" % (float(srate), i_srate)]
    for ch in range(2):
        l += ["I %d %d" % (ch, gri[ch]), "A %d %d" % (ch, algo[ch]), "P %d %r" % (ch, param[ch])]
        if gain[ch]:
            l.append("G %d %d" % (ch, gain[ch]))
        if offset[ch]:
            l.append("O %d %d" % (ch, offset[ch]))
    return l + ["S"]


def scripts():
    s = {
        # the reference's own numbers: a row a second.  CMA over 2 s on chain A (the time-out resets it, no command does), EMA on chain B
        "cma_ema_12000": _setup(12000, 12000, (GRI_A, GRI_B), (CMA, EMA), (2, 8)) + _B("loran", 0, 110),
        # 20.25 kHz: both GRIs are halved; fixed gains that leave the bytes spread
        "halved_20250": _setup(20250, 20250, (GRI_A, GRI_B), (IIR, CMA), (0.0004, 3), gain=(-35, -33)) + _B("loran", 0, 100),
        # a small i_srate brings rows within a few blocks.  Both channels on one GRI with no offset: they emit on the same sample
        "same_sample": _setup(12000, 600, (GRI_A, GRI_A), (CMA, EMA), (1, 4), gain=(0, -34)) + _B("loran", 0, 24),
        "iir_auto": _setup(12000, 600, (GRI_A, GRI_B), (IIR, IIR), (0.0005, 0.003)) + _B("loran", 30, 24),
        "ema_fixed_clipped": _setup(12000, 600, (GRI_B, GRI_A), (EMA, EMA), (16, 1), gain=(30, 0)) + _B("loran", 10, 20),
        # leading silence under auto gain: max == 0, every byte 0
        "silence_auto": _setup(12000, 600, (GRI_A, GRI_B), (CMA, IIR), (3, 0.001)) + _B("silence_noise", 0, 16),
        # offsets: positive, negative below zero (the unsigned modulo does not give the residue), at the start (samp < offset) and in mid-run
        "offsets": _setup(12000, 600, (GRI_A, GRI_B), (CMA, EMA), (2, 6), offset=(37, -3)) + _B("loran", 0, 8) + ["O 0 -500", "O 1 700"]
                   + _B("loran", 8, 8) + ["O 0 -2000000000", "O 1 1000"] + _B("loran", 16, 8),
        # a command of each kind in mid-run
        "commands_mid_run": _setup(12000, 600, (GRI_A, GRI_B), (CMA, CMA), (2, 2)) + _B("loran", 0, 6) + ["I 0 %d" % GRI_B] + _B("loran", 6, 6)
                            + ["G 1 -34"] + _B("loran", 12, 5) + ["A 0 2", "P 0 0.002"] + _B("loran", 17, 6) + ["A 1 1", "P 1 3.5"] + _B("loran", 23, 6)
                            + ["I 1 5930", "G 1 0"] + _B("loran", 29, 6),
        # stop / start keeps the state; a second ext_server_init does the memset
        "stop_start_reinit": _setup(12000, 600, (GRI_A, GRI_B), (EMA, CMA), (5, 2)) + _B("loran", 0, 7) + ["T"] + _B("noise", 0, 3) + ["S"] + _B("loran", 7, 7)
                             + _setup(12000, 600, (GRI_B, GRI_A), (IIR, EMA), (0.002, 2))[:-1] + _B("loran", 14, 8),
        "ns170": _setup(12000, 600, (GRI_A, GRI_B), (CMA, IIR), (1, 0.0008)) + _B("loran", 0, 40, ns=170),
        "rate_12001.3": _setup(12001.3, 700, (GRI_A, 8970), (EMA, CMA), (3, 1)) + _B("loran", 40, 16),
        # nbucket 1 (samp_per_GRI 0.96: every sample has bn 0 and the guard leaves nothing) and nbucket 2 (1.08: bucket 0 alone is written)
        "nbucket_1_2": _setup(12000, 600, (8, 9), (CMA, EMA), (1, 4)) + _B("noise", 0, 4),
        "noise_cma_long": _setup(12000, 600, (GRI_A, 4990), (CMA, CMA), (1000, 1)) + _B("noise", 0, 48),
    }
    return s


def nblocks(lines):
    return sum(1 for l in lines if l[0] == "B")


def parse(raw, nblk):
    """out.bin of the reference harness or the host driver -> dict: nrows int32 [blocks], samp / ch / cmd / len int32 [rows], rows (list
    of uint8 arrays), scalars (one record of scalars_dtype) and avg float32 [2, 1199]"""
    at, nrows, head, rows = 0, [], [], []
    for _ in range(nblk):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        nrows.append(n)
        for _ in range(n):
            h = np.frombuffer(raw[at:at + 16], np.int32)
            head.append(h)
            rows.append(np.frombuffer(raw[at + 16:at + 16 + int(h[3])], np.uint8))
            at += 16 + int(h[3])
    assert len(raw) - at == STATE_BYTES, (len(raw), at)
    head = np.array(head, np.int32).reshape(-1, 4)
    return {"nrows": np.array(nrows, np.int32), "samp": head[:, 0].copy(), "ch": head[:, 1].copy(), "cmd": head[:, 2].copy(), "len": head[:, 3].copy(),
            "rows": rows, "scalars": np.frombuffer(raw[at:at + SCALARS], scalars_dtype)[0].copy(),
            "avg": np.frombuffer(raw[at + SCALARS:], np.float32).reshape(2, MAX_BUCKET).copy()}


def all_bytes(got):
    return np.concatenate([np.asarray(r, np.uint8) for r in got["rows"]]) if got["rows"] else np.zeros(0, np.uint8)


def golden_of(got):
    """what the golden file keeps of a reference run: everything"""
    return {"nrows": got["nrows"], "samp": got["samp"], "ch": got["ch"], "cmd": got["cmd"], "len": got["len"], "rows": all_bytes(got),
            "scalars": np.frombuffer(got["scalars"].tobytes(), np.uint8), "avg": got["avg"]}


def check_against_golden(g, name, got):
    """equality on everything: the rows (bytes, command, length, channel, the block and the sample they went out at, their order) and
    the end state bit for bit"""
    k = "s_%s_" % name
    assert np.array_equal(got["nrows"], g[k + "nrows"]), (name, "rows per block", got["nrows"], g[k + "nrows"])
    for f in ("samp", "ch", "cmd", "len"):
        assert np.array_equal(got[f], g[k + f]), (name, f, got[f], g[k + f])
    allb = all_bytes(got)
    assert allb.size == g[k + "rows"].size, name
    bad = np.flatnonzero(allb != g[k + "rows"])
    assert bad.size == 0, (name, "first differing row byte", int(bad[0]), int(allb[bad[0]]), int(g[k + "rows"][bad[0]]), int(bad.size))
    want = np.frombuffer(g[k + "scalars"].tobytes(), scalars_dtype)[0]
    have = got["scalars"]
    for f in ("i_srate", "redraw_legend", "srate"):
        assert have[f].tobytes() == want[f].tobytes(), (name, f, have[f], want[f])
    for ch in range(2):
        for f in chan_dtype.names:
            assert have["ch"][ch][f].tobytes() == want["ch"][ch][f].tobytes(), (name, "channel", ch, f, have["ch"][ch][f], want["ch"][ch][f])
    a, b = np.ascontiguousarray(got["avg"]).view(np.uint32), np.ascontiguousarray(g[k + "avg"]).view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, (name, "first differing average", bad[0].tolist(), got["avg"][tuple(bad[0])], g[k + "avg"][tuple(bad[0])], len(bad))


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "lorc_host_driver")


def run_script_exe(exe, lines, samples, tmpdir, expect=0, by_runs=False, keep_on=False):
    out = script_common.run_script(exe, (["-r"] if by_runs else []) + (["-k"] if keep_on else []), lines, samples, np.complex64, tmpdir, expect)
    return parse(out, nblocks(lines)) if expect == 0 else None


# ---- a script on the device object
def apply_command(q, conn, l):
    op, a = l[0], l[2:].split()
    if op == "N":
        q.init(conn, float(a[0]), int(a[1]))
    elif op == "I":
        q.set_gri(conn, int(a[0]), int(a[1]))
    elif op == "O":
        q.set_offset(conn, int(a[0]), int(a[1]))
    elif op == "G":
        q.set_gain(conn, int(a[0]), int(a[1]))
    elif op == "A":
        q.set_avg_algo(conn, int(a[0]), int(a[1]))
    elif op == "P":
        q.set_avg_param(conn, int(a[0]), float(a[1]))
    elif op == "S":
        q.start(conn)
    elif op == "T":
        q.stop(conn)
    else:
        raise ValueError(l)


def state_of(q, conn):
    info, avg = q.state(conn)
    sc = np.zeros(1, scalars_dtype)[0]
    sc["i_srate"], sc["redraw_legend"], sc["srate"] = info["i_srate"], info["redraw_legend"], info["srate"]
    for ch in range(2):
        for f in chan_dtype.names:
            sc["ch"][ch][f] = info["ch"][ch][f]
    return {"scalars": sc, "avg": avg}


class Recorder:
    """what a script leaves, in the keys of parse(): rows are added call by call"""

    def __init__(self, nblk):
        self.nrows = np.zeros(nblk, np.int32)
        self.head, self.rows = [], []

    def add(self, blocks, m, rows):
        """blocks: the script's block number of each block of the call; m: the call's row map of ONE connection, in send order"""
        for r in m:
            self.nrows[blocks[int(r["blk"])]] += 1
            self.head.append((int(r["samp"]), int(r["ch"]), int(r["cmd"]), int(r["len"])))
            self.rows.append(rows[int(r["off"]):int(r["off"]) + int(r["len"])].copy())

    def result(self, state):
        head = np.array(self.head, np.int32).reshape(-1, 4)
        out = {"nrows": self.nrows, "samp": head[:, 0].copy(), "ch": head[:, 1].copy(), "cmd": head[:, 2].copy(), "len": head[:, 3].copy(), "rows": self.rows}
        out.update(state)
        return out


def script_calls(lines, max_blocks=48):
    """a script as a list of steps: ("cmd", line) or ("push", ns, [pool offsets], [block numbers]) -- consecutive B lines of one ns,
    consecutive in the pool, at most max_blocks of them"""
    steps, seen = [], 0
    for l in lines:
        if l[0] == "B":
            ns, off = (int(v) for v in l.split()[1:])
            last = steps[-1] if steps else None
            if last and last[0] == "push" and last[1] == ns and len(last[2]) < max_blocks and last[2][-1] + ns == off:
                last[2].append(off)
                last[3].append(seen)
            else:
                steps.append(("push", ns, [off], [seen]))
            seen += 1
        else:
            steps.append(("cmd", l))
    return steps


def run_script_dev(q, lines, samples, conn=0, max_blocks=48):
    """Runs a script on connection conn of q (a LoranC): every push one kg_lorc_process call.  -> the keys of parse(), and "calls"."""
    rec, calls = Recorder(nblocks(lines)), 0
    for st in script_calls(lines, max_blocks):
        if st[0] == "cmd":
            apply_command(q, conn, st[1])
            continue
        _, ns, offs, blocks = st
        x = samples[offs[0]:offs[0] + ns * len(offs)].reshape(1, len(offs), ns)
        rows, m = q.process([conn], x)
        rec.add(blocks, m, rows)
        calls += 1
    out = rec.result(state_of(q, conn))
    out["calls"] = calls
    return out
