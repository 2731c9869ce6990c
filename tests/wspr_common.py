"""What the WSPR tests and tools/make_ref_wspr_golden.py share: the seeded pool of IQ samples, the planes of the `_load` cases, the
scripts (in the script language of tools/ref/wspr_harness.h), the runner of a harness binary and the reader of its records.  Test
infrastructure; never imported by the product package.

Inputs are rebuilt from seeds with the integer generator of tests/ext_random.py -- np.random.default_rng(base + seed) drawing integers --
under a base of this module's own (ext_random itself imports the five older extensions' modules and goldens), and kept in the golden by
digest."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BASE = 0x57535000
NBINS, NFFT, NT, NFFTS, TPOINTS, MAX_NPK, NSYM, SPS = 411, 512, 348, 343, 45000, 12, 162, 256
DF2 = 0.732421875
PR3 = np.array([int(c) for c in
                "110000001000111000100101111000000010010100000010110011010001101000011010101010010010110001101010001000001001001110110011010001110000010100110000000110101100011000"],
               np.int64)
assert PR3.size == NSYM and PR3.sum() == 63
IDLE, SYNC, RUNNING, DECODING = 1, 2, 3, 4
CYCLE = 45056                                       # 88 blocks of 512: the 45000 samples of a cycle and the wait behind them
SAVG_GROUPS = (0, 1, 42, 85)                        # the rows whose savg the golden keeps


def digest(b):
    return hashlib.sha256(b).digest()


def rng(seed):
    return np.random.default_rng(BASE + seed)


# ---- the pool: complex64, integer valued
def noise(n, seed, amp=300):
    r = rng(seed)
    return (r.integers(-amp, amp + 1, n) + 1j * r.integers(-amp, amp + 1, n)).astype(np.complex64)


def fsk(n, seed, signals, amp_noise=300):
    """n samples at 375 Hz: integer noise, and per signal (f0 Hz from the centre, start in samples, drift Hz over the message) a 4-FSK
    WSPR message -- symbol k is pr3[k] + 2 * a seeded data bit, tone f0 + (symbol - 1.5) * 375 / 256 Hz for 256 samples -- 20 dB above
    the noise: amplitude 10 * the noise's rms.  Rounded to integers."""
    x = noise(n, seed, amp_noise).astype(np.complex128)
    rms = np.sqrt(2 * (amp_noise * (amp_noise + 1) / 3.0))
    for m, (f0, start, drift) in enumerate(signals):
        data = rng(seed + 1000 + m).integers(0, 2, NSYM)
        sym = PR3 + 2 * data
        t = np.arange(NSYM * SPS)
        f = f0 + (np.repeat(sym, SPS) - 1.5) * (375.0 / 256) + drift * (t / float(NSYM * SPS) - 0.5)
        ph = 2 * np.pi * np.cumsum(f) / 375.0
        s = 10 * rms * np.exp(1j * ph)
        lo, hi = max(start, 0), min(start + s.size, n)
        x[lo:hi] += s[lo - start:hi - start]
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


E2E_A = [(20.0, 750, 0.0)]                                             # one signal at the nominal start (2 s), no drift
E2E_B = [(-61.0, 750 + 384, -2.0), (47.5, 750 - 512, 3.0)]            # two, off the nominal start, drifting
SEGMENTS = (("e2e_a", CYCLE), ("e2e_b", CYCLE), ("noise", CYCLE + 8192), ("zeros", CYCLE), ("free", 4096))
AT = {}
_at = 0
for _n, _l in SEGMENTS:
    AT[_n] = _at
    _at += _l
POOL = _at


def pool():
    """complex64 [POOL]: the segments at AT[name]; the scripts of rate 750 read them through interleave()"""
    p = np.zeros(POOL, np.complex64)
    p[AT["e2e_a"]:][:CYCLE] = fsk(CYCLE, 1, E2E_A)
    p[AT["e2e_b"]:][:CYCLE] = fsk(CYCLE, 2, E2E_B)
    p[AT["noise"]:][:CYCLE + 8192] = noise(CYCLE + 8192, 3)
    p[AT["free"]:][:4096] = noise(4096, 4)
    return p


def interleave(x, seed=9):
    """the 750 Hz stream whose drop-sample decimation by 2 (the second of every pair is kept, :760-762) is x"""
    y = noise(2 * x.size, seed)
    y[1::2] = x
    return y


# ---- the planes of the `_load` cases: integer valued, every sum exact in float
def ifd_of(ifr, k, idrift):
    return int(ifr + ((float(k) - 81.0) / 81.0 * float(idrift)) / (2.0 * DF2))


def planes(seed, planted=(), flat=False, hole=None, edge_bins=()):
    """pwr_samp [512, 348] of integer noise with sync patterns planted -- (bin0, k0, idrift, amplitude): per symbol the tone of pr3[k] and a
    seeded data bit at transform k0 + 2k -- and pwr_sampavg [512] as the row sums (exact); flat: pwr_sampavg constant (no local
    maximum); hole = bin: the 16 bins the candidate at that bin can touch are zero while pwr_sampavg keeps its peak; edge_bins: extra
    weight on pwr_sampavg there so that the bin is a kept peak"""
    r = rng(seed)
    ps = r.integers(0, 4001, (NFFT, NT)).astype(np.float64)
    for m, (bin0, k0, idrift, amp) in enumerate(planted):
        data = r.integers(0, 2, NSYM)
        if0 = bin0 + 51
        for k in range(NSYM):
            t = k0 + 2 * k
            if 0 <= t < NT:
                ifd = ifd_of(if0, k, idrift)
                ps[ifd + (-3, -1, 1, 3)[int(PR3[k] + 2 * data[k])], t] += amp
    if hole is not None:
        ps[hole + 51 - 8:hole + 51 + 8, :] = 0
    pa = ps[:, :NFFTS + 1].sum(axis=1)
    if hole is not None:
        pa[hole + 51 - 7:hole + 51 + 8] = (pa.max() // 8) * np.array([1, 2, 3, 4, 5, 6, 7, 8, 7, 6, 5, 4, 3, 2, 1])      # its 7-bin sums peak at one bin
    for b in edge_bins:
        pa[b + 51] += 40 * 4000 * NT // 8
    if flat:
        pa[:] = 1000.0
    assert ps.max() < 2 ** 24 and pa.max() < 2 ** 24
    return ps.astype(np.float32), pa.astype(np.float32)


# name -> (keyword arguments of planes(), script lines ahead of the L line)
LOADS = {
    "planted3": (dict(seed=11, planted=((150, 0, 0, 20000), (233, 5, -3, 16000), (301, -4, 4, 12000))), []),
    "edges": (dict(seed=12, planted=((55, 1, 1, 20000), (355, -2, -1, 20000)), edge_bins=(55, 355)), []),
    "lags": (dict(seed=13, planted=((120, -10, 2, 20000), (290, 21, -2, 20000))), []),
    "many": (dict(seed=14, planted=tuple((70 + 17 * m, m - 7, m % 9 - 4, 9000 + 500 * m) for m in range(16))), []),
    "flat": (dict(seed=15, flat=True), []),
    "more": (dict(seed=16, planted=((150, 0, 0, 20000), (232, 3, 2, 15000))), ["M 1"]),
    "power0": (dict(seed=17, planted=((140, 2, 1, 20000),), hole=260), []),
    "type15": (dict(seed=18, planted=((200, 0, -1, 20000),)), ["Y 15"]),
}


def clock(samples, rate, t0):
    """minute and second of the callback that begins `samples` samples after t0 seconds"""
    t = t0 + samples / float(rate)
    return int(t // 60) % 60, int(t) % 60


def blocks(seg, first, n, size, rate=375, t0=0.0, base=0):
    """B lines for n samples of segment seg from `first` on, cut into callbacks of `size`, the clock running from t0 at sample `base`"""
    out, k = [], 0
    while k < n:
        m = min(size, n - k)
        mi, se = clock(base + k, rate, t0)
        out.append("B %d %d %d %d" % (AT[seg] + first + k, m, mi, se))
        k += m
    return out


def scripts():
    sc = {}
    sc["e2e_a"] = ["I 375", "C 1"] + blocks("e2e_a", 0, CYCLE, 512) + blocks("noise", 0, 2048, 512, base=CYCLE)
    # free running from 1:57 on, the resync at the even minute 2:00, 3 s in and long before the cycle is full; then the whole cycle
    sc["resync"] = ["I 375", "C 1"] + blocks("free", 0, 1125, 375, t0=117.0) + blocks("e2e_b", 0, CYCLE, 1024, t0=120.0)
    # the schedule's edges on noise: odd callbacks, two groups in one, capture off and on, the wait at didx >= TPOINTS, a second cycle's start
    e = ["I 375", "C 1"] + blocks("noise", 0, 700, 700) + blocks("noise", 700, 1, 1, base=700) + blocks("noise", 701, 1500, 1500, base=701)
    e += ["C 0"] + blocks("noise", 2201, 512, 512, base=2201) + ["C 1"] + blocks("noise", 2713, 3000, 1000, t0=100.0)
    e += blocks("noise", 0, CYCLE + 4096, 4096, t0=120.0)
    sc["edges_sched"] = e
    sc["silence"] = ["I 375", "C 1"] + blocks("zeros", 0, CYCLE, 2048)
    for name, (kw, head) in LOADS.items():
        sc["load_" + name] = ["I 375"] + head + ["L " + name]
    return sc


E2E = ("e2e_a", "resync")                           # the end-to-end scenes: the winner's margin is held to 1e-3


# ---- running a harness binary
REC_WORDS = {1: 3, 4: 4 + 512, 2: 5 + 103, 3: 4 + 36 + 72 + 4, 5: 1 + 18}


def parse(words):
    ev, rows, meta, savg, cyc, info = [], [], [], {}, [], None
    i = 0
    while i < words.size:
        k = int(words[i])
        n = REC_WORDS[k]
        r = words[i:i + n]
        if k == 1:
            ev.append((int(r[1]), int(r[2])))
        elif k == 4:
            savg[len(rows)] = r[4:].view(np.float32).copy()
        elif k == 2:
            meta.append((int(r[1]), int(r[2]), int(r[3]), int(r[4])))
            rows.append(r[5:].copy().view(np.uint8))
        elif k == 3:
            cyc.append(r[1:].copy())
        else:
            info = r[1:].copy()
        i += n
    assert i == words.size and info is not None
    return dict(ev=np.array(ev, np.int32).reshape(-1, 2), rows=np.array(rows, np.uint8).reshape(-1, NBINS + 1), meta=np.array(meta, np.int32).reshape(-1, 4),
                savg=savg, cyc=np.array(cyc, np.int32).reshape(-1, 115), info=info)


def run_script_exe(exe, lines, samples, tmp, expect=0):
    tmp = str(tmp)
    pool_path = os.path.join(tmp, "pool.bin")
    if not os.path.exists(pool_path):
        samples.astype(np.complex64).tofile(pool_path)
    out = []
    for l in lines:
        if l.startswith("L "):
            ps, pa = planes(**LOADS[l[2:]][0])
            path = os.path.join(tmp, "planes_%s.bin" % l[2:])
            np.concatenate([ps.ravel(), pa]).astype(np.float32).tofile(path)
            l = "L " + path
        out.append(l)
    open(os.path.join(tmp, "script.txt"), "w").write("\n".join(out) + "\n")
    r = subprocess.run([exe, os.path.join(tmp, "script.txt"), pool_path, os.path.join(tmp, "out.bin"), os.path.join(tmp, "planes.bin")])
    assert r.returncode == expect, (r.returncode, expect)
    if expect:
        return None
    got = parse(np.fromfile(os.path.join(tmp, "out.bin"), np.int32))
    pl = np.fromfile(os.path.join(tmp, "planes.bin"), np.float32)
    got["pwr_sampavg"] = pl[:2 * NFFT].reshape(2, NFFT).copy()
    got["pwr_samp"] = pl[2 * NFFT:][:2 * NFFT * NT].reshape(2, NFFT, NT).copy()
    got["iq"] = pl[2 * NFFT + 2 * NFFT * NT:].reshape(2, 2, TPOINTS).copy()
    return got


def golden_of(got):
    """what the golden keeps of a run: integers and bytes in full, pwr_sampavg, the savg of a few rows, the large planes by digest"""
    keep = [r for r in sorted(got["savg"]) if got["meta"][r][1] in SAVG_GROUPS][:8]
    return dict(ev=got["ev"], rows=got["rows"], meta=got["meta"], cyc=got["cyc"][:, :111], cond=got["cyc"][:, 111:], info=got["info"],
                pwr_sampavg=got["pwr_sampavg"], savg_rows=np.array(keep, np.int32), savg=np.array([got["savg"][r] for r in keep], np.float32).reshape(-1, NFFT),
                pwr_samp_sha=np.frombuffer(digest(got["pwr_samp"].tobytes()), np.uint8), iq_sha=np.frombuffer(digest(got["iq"].tobytes()), np.uint8))


def cycle_fields(c):
    """one cycle record of the golden (111 words: blk half npk pk[12][3] cand[12][6]) -> (blk, half, npk, pk, cand) with the floats as bits"""
    return int(c[0]), int(c[1]), int(c[2]), c[3:39].reshape(12, 3), c[39:111].reshape(12, 6)


def build_driver(tmp):
    exe = os.path.join(str(tmp), "wspr_host")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "wspr_host_driver.cpp"), "-lm"], check=True)
    return exe


def load():
    return np.load(os.path.join(GOLD, "wspr_ref.npz"))
