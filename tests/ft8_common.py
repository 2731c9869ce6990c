"""What the FT8 / FT4 tests and tools/make_ref_ft8_golden.py share: the seeded scenes (waterfalls of the load path, sample streams of the
monitor and end-to-end scenes), the writer of a scene file and the reader of the records of tools/ref/ft8_harness.h, the build of the
host twin, and the golden's conditions.  Test infrastructure; never imported by the product package.

Inputs are rebuilt from seeds -- np.random.default_rng(BASE + seed) drawing integers -- and kept in the golden by digest."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BASE = 0x46543800
FT8, FT4 = 0, 1
RATE, NS = 12000, 512
MAX_CAND, MIN_SCORE, LDPC_N = 140, 10, 174
# the derived sizes at 12000 Hz; the golden's maker asserts each on the reference, the CPU test against the golden
SIZES = {FT8: dict(block=1920, nfft=3840, num_bins=481, min_bin=16, max_blocks=93, num_samples=175200, slot_blocks=92, period=15.0, symbol=0.160),
         FT4: dict(block=576, nfft=1152, num_bins=145, min_bin=4, max_blocks=156, num_samples=85200, slot_blocks=148, period=7.5, symbol=0.048)}
COSTAS8 = (3, 1, 4, 0, 6, 5, 2)
COSTAS4 = ((0, 1, 3, 2), (1, 0, 2, 3), (2, 3, 1, 0), (3, 2, 0, 1))
GRAY8, GRAY4 = (0, 1, 3, 2, 5, 6, 4, 7), (0, 1, 3, 2)
LOAD, STREAM = 0, 1
T_SIZES, T_EVENT, T_SLOT, T_END = 1, 2, 3, 4
KEEP = 20                                           # log174 of the first KEEP candidates of a scene, except in FULL_LOG
FULL_LOG = "load_a_ft8"

cand_dtype = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1"),
                       ("freq_hz", "<f4"), ("time_sec", "<f4"), ("snr", "<f4")])
CAND_KEY = ("score", "time_offset", "freq_offset", "time_sub", "freq_sub")


def digest(b):
    return hashlib.sha256(b).digest()


def rng(seed):
    return np.random.default_rng(BASE + seed)


def pname(p):
    return "ft4" if p == FT4 else "ft8"


def sync_blocks(p):
    """(block relative to the candidate, expected tone) of every Costas symbol (decode.c:72-95, :138-153)"""
    if p == FT4:
        return [(1 + 33 * m + k, COSTAS4[m][k]) for m in range(4) for k in range(4)]
    return [(36 * m + k, COSTAS8[k]) for m in range(3) for k in range(7)]


def data_blocks(p):
    """the block of every data symbol (decode.c:265, :291)"""
    if p == FT4:
        return [k + (5 if k < 29 else 9 if k < 58 else 13) for k in range(87)]
    return [k + (7 if k < 29 else 14) for k in range(58)]


# ---- the load path: waterfalls [num_blocks, 2, 2, num_bins]
def plants(p):
    """(time_offset, freq_offset, time_sub, freq_sub): the four time offsets of the search's edges, both frequency edges, all four cells"""
    nb, tones = SIZES[p]["num_bins"], 4 if p == FT4 else 8
    return [(-10, 0, 0, 0), (-1, nb - tones, 0, 1), (0, nb // 2, 1, 0), (19, nb // 3, 1, 1)]


def waterfall(p, seed, num_blocks=20, planted=True, constant=None):
    nb = SIZES[p]["num_bins"]
    if constant is not None:
        return np.full((num_blocks, 2, 2, nb), constant, np.uint8)
    mag = rng(seed).integers(80, 120, (num_blocks, 2, 2, nb)).astype(np.uint8)
    if planted:
        tones = 4 if p == FT4 else 8
        for to, fo, ts, fs in plants(p):
            for blk, tone in sync_blocks(p):
                b = to + blk
                if 0 <= b < num_blocks:
                    mag[b, ts, fs, fo:fo + tones] = 40
                    mag[b, ts, fs, fo + tone] = 200
    return mag


# name -> (protocol, waterfall arguments, num_candidates, min_score); 20 blocks unless stated: the `break` at num_blocks and the zeroed bits
LOADS = {}
for _p in (FT8, FT4):
    _n = pname(_p)
    LOADS["load_a_" + _n] = (_p, dict(seed=1 + _p, num_blocks=50), 140, 10)  # 50 blocks: a group planted at -10 shows its second Costas group
    LOADS["load_b_" + _n] = (_p, dict(seed=1 + _p), 4, 3)                   # far more pass than 4: eviction, ties at the heap's minimum
    LOADS["load_c_" + _n] = (_p, dict(seed=1 + _p), 140, 2)                 # more pass than 140
    LOADS["load_none_" + _n] = (_p, dict(seed=1 + _p), 140, 300)            # nothing passes
    LOADS["load_const_" + _n] = (_p, dict(seed=0, constant=100), 140, 0)    # every score 0: all tie, variance 0, log174 NaN


# ---- the streams: int16 [callbacks, NS] and the clock reading of every callback, a multiple of 1 / 64 s (so that tv_sec + tv_nsec / 1e9
# of decode_ft8.c:513 is the reading itself)
def clock(t0, ncb, ns=NS):
    return np.floor((t0 + np.arange(ncb) * (ns / float(RATE))) * 64.0) / 64.0


def tones_and_noise(n, seed, amp=100, tones=((431.0, 2000.0), (1502.5, 600.0))):
    r = rng(seed)
    x = r.integers(-amp, amp + 1, n).astype(np.float64)
    t = np.arange(n) / float(RATE)
    for f, a in tones:
        x += a * np.sin(2 * np.pi * f * t)
    return np.round(x).astype(np.int16)


def frame_samples(p, to, ts, fo, fs, seed, amp):
    """(first sample relative to the slot's first, float64 samples) of a synthetic frame whose symbol 0 is centred on the analysis
    frame of (block `to`, time_sub `ts`) and whose tone 0 lies on bin fo of freq_sub fs: Costas groups plus seeded data symbols"""
    sz = SIZES[p]
    block, sub = sz["block"], sz["block"] // 2
    nsym = 105 if p == FT4 else 79
    tone = np.full(nsym, -1)
    for blk, tn in sync_blocks(p):
        tone[blk] = tn
    data = rng(seed).integers(0, 4 if p == FT4 else 8, len(data_blocks(p)))
    gray = GRAY4 if p == FT4 else GRAY8
    for k, blk in enumerate(data_blocks(p)):
        tone[blk] = gray[int(data[k])]
    f0 = (sz["min_bin"] + fo + fs / 2.0) / sz["symbol"]
    f = np.repeat(f0 + np.maximum(tone, 0) / sz["symbol"], block)
    a = np.repeat(np.where(tone >= 0, float(amp), 0.0), block)          # FT4's ramp symbols are silent
    ph = 2 * np.pi * np.cumsum(f) / RATE
    return to * block + (ts - 2) * sub, a * np.sin(ph)


E2E_FRAMES = {FT8: [(3, 0, 100, 0), (-3, 1, 250, 1), (7, 1, 400, 0)], FT4: [(3, 0, 20, 0), (-3, 1, 60, 1), (9, 1, 110, 0)]}      # (to, ts, fo, fs); one starts before the slot


def slot_stream(p, seed, frames=(), ncb_after=0, t0=None, amp=100, pre=2):
    """`pre` callbacks before the slot (dropped: the clock says three quarters of a slot), one full slot, the callbacks to the next
    sync and ncb_after behind it -> (samples [ncb, NS], times [ncb])"""
    sz = SIZES[p]
    t0 = 1000 * sz["period"] + 0.8125 if t0 is None else t0              # (t0 - 0.8) mod period = 1 / 80 s
    slot_cb = -(-sz["slot_blocks"] * sz["block"] // NS)
    gap_cb = int(np.ceil(sz["period"] * RATE / NS)) - slot_cb + 1        # to the first callback whose clock lies in the next slot's first quarter
    n = (slot_cb + gap_cb + ncb_after) * NS
    x = rng(seed).integers(-amp, amp + 1, n).astype(np.float64)
    for m, (to, ts, fo, fs) in enumerate(frames):
        s0, s = frame_samples(p, to, ts, fo, fs, seed + 100 + m, 3000.0)
        lo, hi = max(s0, 0), min(s0 + s.size, n)
        x[lo:hi] += s[lo - s0:hi - s0]
    body = np.round(x).astype(np.int16).reshape(-1, NS)
    head = rng(seed + 7).integers(-amp, amp + 1, (pre, NS)).astype(np.int16)
    times = np.concatenate([clock(t0 - sz["period"] / 4.0 - 1.0, pre), clock(t0, body.shape[0])])
    return np.concatenate([head, body]), times


def short_stream(p, kind, seed):
    """6 blocks from a sync, behind two dropped callbacks"""
    sz = SIZES[p]
    ncb = -(-6 * sz["block"] // NS)
    n = ncb * NS
    if kind == "tones":
        x = tones_and_noise(n, seed)
    elif kind == "silence":
        x = np.zeros(n, np.int16)
    else:
        x = (rng(seed).integers(0, 2, n) * 2 - 1).astype(np.int16) * 32767
    t0 = 2000 * sz["period"] + 0.8125
    head = rng(seed + 7).integers(-100, 101, (2, NS)).astype(np.int16)
    return np.concatenate([head, x.reshape(-1, NS)]), np.concatenate([clock(t0 - sz["period"] / 4.0 - 1.0, 2), clock(t0, ncb)])


# name -> (protocol, maker of (samples, times))
STREAMS = {}
for _p in (FT8, FT4):
    _n = pname(_p)
    STREAMS["mon6_" + _n] = (_p, lambda p=_p: short_stream(p, "tones", 11 + p))
    STREAMS["silence_" + _n] = (_p, lambda p=_p: short_stream(p, "silence", 0))
    STREAMS["boundary_" + _n] = (_p, lambda p=_p: slot_stream(p, 21 + p, ncb_after=-(-3 * SIZES[p]["block"] // NS)))
    STREAMS["e2e_" + _n] = (_p, lambda p=_p: slot_stream(p, 31 + p, frames=E2E_FRAMES[p]))
STREAMS["fullscale_ft8"] = (FT8, lambda: short_stream(FT8, "full", 41))
MONITOR = [n for n in STREAMS if not n.startswith("e2e_")]               # the scenes whose bytes of build A the golden keeps
TAIL_BLOCKS = 2                                                          # of a full slot's waterfall the golden keeps the last two blocks


def scene_bytes(name):
    """the scene file of tools/ref/ft8_harness.h"""
    if name in LOADS:
        p, kw, ncand, min_score = LOADS[name]
        mag = waterfall(p, **kw)
        return np.array([LOAD, p, mag.shape[0], ncand, min_score, 0, 0, 0], np.int32).tobytes() + mag.tobytes()
    p, make = STREAMS[name]
    x, t = make()
    return stream_bytes(p, x, t)


def stream_bytes(p, x, t, reinit_at=-1, reinit_protocol=0):
    x = np.ascontiguousarray(x, np.int16)
    return (np.array([STREAM, p, x.shape[1], x.shape[0], reinit_at, reinit_protocol, 0, 0], np.int32).tobytes() + np.ascontiguousarray(t, np.float64).tobytes()
            + x.tobytes())


def load_bytes(p, mag, ncand=MAX_CAND, min_score=MIN_SCORE):
    mag = np.ascontiguousarray(mag, np.uint8)
    return np.array([LOAD, p, mag.shape[0], ncand, min_score, 0, 0, 0], np.int32).tobytes() + mag.tobytes()


def parse(raw):
    """the records of a harness run -> dict(sizes, window, events [n, 4] + times, slots [dict], end dict)"""
    out = dict(events=[], slots=[], end=None)
    at = 0
    while at < len(raw):
        tag, n = np.frombuffer(raw, np.int32, 2, at)
        b = raw[at + 8:at + 8 + n]
        at += 8 + int(n)
        if tag == T_SIZES:
            v = np.frombuffer(b, np.int32, 8)
            out["sizes"] = dict(zip(("block", "nfft", "num_bins", "min_bin", "max_blocks", "num_samples", "block_stride", "subblock"), (int(x) for x in v)))
            out["window"] = np.frombuffer(b, np.float32, int(v[1]), 32).copy()
        elif tag == T_EVENT:
            v = np.frombuffer(b, np.int32, 4)
            out["events"].append((int(v[0]), int(v[1]), int(v[2]), int(v[3]), int(np.frombuffer(b, np.int64, 1, 16)[0])))
        elif tag == T_SLOT:
            v = np.frombuffer(b, np.int32, 4)
            nc = int(v[2])
            o = 20
            cand = np.frombuffer(b, cand_dtype, nc, o).copy()
            o += 20 * nc
            log174 = np.frombuffer(b, np.float32, nc * LDPC_N, o).reshape(nc, LDPC_N).copy()
            o += 4 * nc * LDPC_N
            out["slots"].append(dict(cb=int(v[0]), num_blocks=int(v[1]), ncand=nc, max_mag=np.frombuffer(b, np.float32, 1, 16)[0], cand=cand, log174=log174,
                                     mag=np.frombuffer(b, np.uint8, len(b) - o, o).copy()))
        elif tag == T_END:
            v = np.frombuffer(b, np.int32, 8)
            nfft = int(v[6])
            out["end"] = dict(state=v[:6].copy(), nfft=nfft, max_mag=np.frombuffer(b, np.float32, 1, 32)[0], last_frame=np.frombuffer(b, np.float32, nfft, 36).copy(),
                              mag=np.frombuffer(b, np.uint8, len(b) - 36 - 4 * nfft, 36 + 4 * nfft).copy())
    return out


def run_exe(exe, scene, tmp, expect=0):
    """scene: the bytes of a scene file"""
    tmp = str(tmp)
    sp, op = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
    with open(sp, "wb") as f:
        f.write(scene)
    r = subprocess.run([exe, sp, op])
    assert r.returncode == expect, (r.returncode, expect)
    if expect:
        return None
    with open(op, "rb") as f:
        return parse(f.read())


def build_driver(tmp, defines=()):
    exe = os.path.join(str(tmp), "ft8_host_driver" + "".join("_" + d.split("=")[0] for d in defines))
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe] + ["-D" + d for d in defines] + [os.path.join(ROOT, "tools", "ft8_host_driver.cpp"), "-lm"], check=True)
    return exe


def load():
    return np.load(os.path.join(GOLD, "ft8_ref.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def slot_golden(sl, keep):
    """what the golden keeps of a slot record: every candidate, log174 of the first `keep`, a digest of all of it"""
    return dict(cand=sl["cand"], log174=sl["log174"][:keep], log_sha=np.frombuffer(digest(sl["log174"].tobytes()), np.uint8),
                head=np.array([sl["cb"], sl["num_blocks"], sl["ncand"]], np.int32), max_mag=np.array([sl["max_mag"]], np.float32))


def same_slot(got, g, k, keep, what, max_mag=True):
    """a parsed slot record against the golden's entries under the prefix k: every field, floats by their bits (NaN included)"""
    assert [got["cb"], got["num_blocks"], got["ncand"]] == [int(v) for v in g[k + "head"]], (what, "head")
    assert got["cand"].tobytes() == np.ascontiguousarray(g[k + "cand"]).tobytes(), (what, "candidates")
    assert bits(got["log174"][:keep]).tobytes() == bits(g[k + "log174"]).tobytes(), (what, "log174")
    assert digest(got["log174"].tobytes()) == bytes(g[k + "log_sha"]), (what, "log174 of every candidate")
    if max_mag:
        assert bits(got["max_mag"]).tobytes() == bits(g[k + "max_mag"]).tobytes(), (what, "max_mag")


def golden_conditions(g, size):
    """what the tests rely on, stated once: checked when the golden is made and by the CPU suite"""
    assert size < 400 * 1024, size
    assert sorted(str(n) for n in g["load_names"]) == sorted(LOADS) and sorted(str(n) for n in g["stream_names"]) == sorted(STREAMS)
    for p in (FT8, FT4):
        v = g["sizes_" + pname(p)]
        sz = SIZES[p]
        assert [int(x) for x in v] == [sz["block"], sz["nfft"], sz["num_bins"], sz["min_bin"], sz["max_blocks"], sz["num_samples"], 4 * sz["num_bins"], sz["block"] // 2,
                                       sz["slot_blocks"]], pname(p)
        assert g["window_" + pname(p)].size == sz["nfft"]
    for name, (p, kw, ncand, min_score) in LOADS.items():
        k = "l_%s_" % name
        npass, nc = int(g[k + "npass"][0]), int(g[k + "head"][2])
        sc = g[k + "cand"]["score"]
        assert nc == min(npass, ncand) and (np.diff(sc.astype(np.int32)) <= 0).all(), name
        if "_b_" in name or "_c_" in name:
            assert npass > ncand, (name, "eviction")
        if "_c_" in name:                                   # equal scores at the lowest kept score and further up the list
            assert int(g[k + "ntie_min"][0]) >= 2 and (np.diff(sc[sc > sc[-1]].astype(np.int32)) == 0).any(), (name, "ties")
        if "_none_" in name:
            assert npass == 0 and nc == 0
        if "_const_" in name:
            assert nc == ncand and (sc == 0).all() and np.isnan(g[k + "log174"]).all()
        if "_a_" in name:
            got = {tuple(int(c[f]) for f in CAND_KEY[1:]) for c in g[k + "cand"]}
            assert all(pl in {(a, b, c, d) for a, b, c, d in got} for pl in plants(p)), (name, "a planted group is not a candidate")
    for name in STREAMS:
        k = "s_%s_" % name
        n_ab, nbytes, dmax = int(g[k + "n_ab"][0]), int(g[k + "nbytes"][0]), int(g[k + "ab_max"][0])
        assert dmax <= 1 and n_ab <= 0.001 * nbytes, (name, n_ab, nbytes, dmax)
        if name.startswith("silence"):
            assert n_ab == 0 and not g[k + "end_mag"].any() and float(g[k + "max_mag_ab"][0]) == 0.0
