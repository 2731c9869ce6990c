"""What the stage-2 WSPR tests and tools/make_ref_wspr_dec_golden.py share: a WSPR encoder, the seeded scenes (samples, the candidates a
caller hands in, the passes), the fano-only symbol sets, the runner of the harness binaries and the reader of their records.  Test
infrastructure; never imported by the product package.

Inputs are rebuilt from seeds with np.random.default_rng(BASE + seed) drawing INTEGERS, and kept in the golden by digest.  The noise of a
scene is the sum of four uniform integers in -259 .. 259 per component: sigma 299.6."""
import hashlib
import os
import subprocess

import numpy as np

from .wspr_common import PR3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BASE = 0x57534400
TPOINTS, NSYM, SPS, MAX_NPK, MAX_IDT = 45000, 162, 256, 12, 129
DF2 = 0.732421875
POLY1, POLY2 = 0xf2d05351, 0xe4613c47
SKIPPED, MINSYNC1, NO_CHANGE, TIME_UP, DECODED, QUICK_MISS = 0, 1, 2, 3, 4, 5

rec_dtype = np.dtype([("result", "<i4"), ("ignore", "<i4"), ("f1", "<f4"), ("shift1", "<i4"), ("drift1", "<f4"), ("sync1", "<f4"),
                      ("tr_f", "<f4", (6,)), ("tr_shift", "<i4", (6,)), ("tr_sync", "<f4", (6,)),
                      ("idt", "<i4"), ("ii", "<i4"), ("jig_shift", "<i4"), ("gates", "<i4"), ("rms", "<f4"),
                      ("metric", "<u4"), ("cycles", "<u4"), ("maxnp", "<u4"), ("decdata", "u1", (11,)), ("symbols", "u1", (NSYM,)), ("pad", "u1", (3,))])
fano_dtype = np.dtype([("ok", "<i4"), ("metric", "<u4"), ("cycles", "<u4"), ("maxnp", "<u4"), ("data", "u1", (10,)), ("pad", "u1", (2,))])
cand_in_dtype = np.dtype([("freq0", "<f4"), ("shift0", "<i4"), ("drift0", "<f4"), ("sync0", "<f4")])
assert rec_dtype.itemsize == 304 and fano_dtype.itemsize == 28


def digest(b):
    return hashlib.sha256(b).digest()


def rng(seed):
    return np.random.default_rng(BASE + seed)


# ---- the encoder: 50 bits, 31 zeros behind them, the K = 32 rate 1/2 code, the bit-reversal interleaver, 2 * bit + sync
def parity(v):
    return bin(v).count("1") & 1


def bitrev8(i):
    return int("{:08b}".format(i)[::-1], 2)


PERM = [j for j in (bitrev8(i) for i in range(256)) if j < NSYM]          # deinterleave: place p holds symbol PERM[p]


def message_bits(seed):
    return rng(seed).integers(0, 2, 50).astype(np.int64)


def encode(bits50):
    """-> (the 162 code bits in transmission order, the 10 bytes fano hands out for them: 80 of the 81 bits, high bit first)"""
    bits = list(int(b) for b in bits50) + [0] * 31
    state, code = 0, []
    for b in bits:
        state = ((state << 1) | b) & 0xffffffff
        code += [parity(state & POLY1), parity(state & POLY2)]
    sent = [0] * NSYM
    for p, j in enumerate(PERM):
        sent[j] = code[p]
    data = bytes(int("".join(str(b) for b in bits[8 * k:8 * k + 8]), 2) for k in range(10))
    return np.array(sent, np.int64), data, np.array(code, np.int64)


def channel_symbols(seed):
    sent, data, _ = encode(message_bits(seed))
    return 2 * sent + PR3, data


# ---- the scenes
def noise(seed):
    r = rng(seed)
    return (r.integers(-259, 260, (4, TPOINTS)).sum(axis=0) + 1j * r.integers(-259, 260, (4, TPOINTS)).sum(axis=0)).astype(np.complex128)


def samples(seed, signals, silent=False):
    """complex64 [45000], integer valued: the noise and per signal (amplitude, f0 Hz, start sample, drift Hz, message seed) the message as
    the decoder models it: symbol i at f0 + drift / 2 * (i - 81) / 81 + (tone - 1.5) * 375 / 256 for 256 samples from start + 256 i on"""
    x = np.zeros(TPOINTS, np.complex128) if silent else noise(seed)
    for amp, f0, start, drift, mseed in signals:
        sym, _ = channel_symbols(mseed)
        i = np.repeat(np.arange(NSYM), SPS)
        f = f0 + drift / 2.0 * (i - 81.0) / 81.0 + (np.repeat(sym, SPS) - 1.5) * (375.0 / 256)
        s = amp * np.exp(1j * 2 * np.pi * np.cumsum(f) / 375.0)
        lo, hi = max(start, 0), min(start + s.size, TPOINTS)
        x[lo:hi] += s[lo - start:hi - start]
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


def near(f):
    return float(np.float32(round(f / DF2) * DF2))


P0, P1 = (200, 2, 0), (1000, 1, 0)
# name -> seed, signals, candidates (freq0, shift0, drift0, sync0), passes (maxcycles, iifac, quickmode)
SCENES = {
    "strong": dict(seed=1, signals=[(80, 20.3, 750, 0.0, 101)], cands=[(near(20.3), 768, 0.0, 0.5)], passes=[P0, P1]),
    "driftp": dict(seed=2, signals=[(80, -47.1, 1100, 2.5, 102)], cands=[(near(-47.1), 1152, 2.0, 0.5)], passes=[P0]),
    "driftm": dict(seed=3, signals=[(80, 63.9, 400, -1.5, 103)], cands=[(near(63.9), 384, -1.0, 0.5)], passes=[P0]),
    "early": dict(seed=4, signals=[(80, 5.2, -300, 1.0, 104)], cands=[(near(5.2), -256, 1.0, 0.5)], passes=[P0]),
    "late": dict(seed=5, signals=[(80, -88.8, 3890, 0.0, 105)], cands=[(near(-88.8), 3900, 0.0, 0.5)], passes=[P0]),
    "jig_a": dict(seed=35, signals=[(37.0, 45.0, 765, 0.0, 135)], cands=[(near(45.0), 768, 0.0, 0.3)], passes=[P0, P1]),          # decodes at ii +2
    "jig_b": dict(seed=35, signals=[(36.0, 45.0, 765, 0.0, 135)], cands=[(near(45.0), 768, 0.0, 0.3)], passes=[P0]),              # at ii +12
    "jig_c": dict(seed=41, signals=[(36.0, 51.0, 771, 0.0, 141)], cands=[(near(51.0), 768, 0.0, 0.3)], passes=[P0, P1]),          # at ii -4
    "jig_d": dict(seed=41, signals=[(37.0, 51.0, 771, 0.0, 141)], cands=[(near(51.0), 768, 0.0, 0.3)], passes=[P0]),              # at ii -10
    "timeup_a": dict(seed=10, signals=[(33, 12.0, 750, 0.0, 110)], cands=[(near(12.0), 768, 0.0, 0.2)], passes=[P0, P1]),         # 129 jiggles on the second pass
    "timeup_b": dict(seed=11, signals=[(35, -33.0, 900, 1.0, 111)], cands=[(near(-33.0), 896, 1.0, 0.2)], passes=[P0, P1]),       # time up, then decoded at iifac 1
    "timeup_c": dict(seed=12, signals=[(27.5, 40.0, 750, 0.0, 112)], cands=[(near(40.0), 768, 0.0, 0.2)], passes=[P0]),
    "nochange_a": dict(seed=35, signals=[(25.0, 45.0, 765, 0.0, 135)], cands=[(near(45.0), 768, 0.0, 0.2)], passes=[P0, P1]),     # no jiggle passes the gate
    "nochange_b": dict(seed=37, signals=[(24.0, 47.0, 767, 0.0, 137)], cands=[(near(47.0), 768, 0.0, 0.2)], passes=[P0]),
    "minsync_a": dict(seed=14, signals=[(18, 25.0, 750, 0.0, 114)], cands=[(near(25.0), 768, 0.0, 0.1)], passes=[P0, P1]),
    "minsync_b": dict(seed=15, signals=[], cands=[(near(-5.0), 512, 3.0, 0.1)], passes=[P0]),
    "silence": dict(seed=16, signals=[], silent=True, cands=[(near(10.0), 768, 0.0, 0.0)], passes=[P0]),
    "quick_hit": dict(seed=17, signals=[(80, 50.5, 770, 0.0, 117)], cands=[(near(50.5), 768, 0.0, 0.5)], passes=[(200, 2, 1)]),
    "quick_miss": dict(seed=18, signals=[(33, -20.5, 770, 0.0, 118)], cands=[(near(-20.5), 768, 0.0, 0.5)], passes=[(200, 2, 1), P0]),
    # two signals, each with the images a peak list puts beside it, and noise-only bins: twelve candidates in SNR order, two passes
    "twelve": dict(seed=19, signals=[(80, 30.2, 750, 0.0, 119), (45, -60.4, 1290, 1.0, 120)],
                   cands=[(near(30.2), 768, 0.0, 0.6), (near(30.2) + DF2, 768, 0.0, 0.5), (near(30.2) - DF2, 768, 0.0, 0.5), (near(-60.4), 1280, 1.0, 0.4),
                          (near(30.2) + 2 * DF2, 768, 0.0, 0.3), (near(-60.4) + DF2, 1280, 1.0, 0.3), (near(-60.4) - DF2, 1280, 1.0, 0.3), (near(30.2) - 2 * DF2, 768, 0.0, 0.3),
                          (near(90.0), 256, -2.0, 0.2), (near(-100.0), 2048, 4.0, 0.2), (near(0.0), 0, 0.0, 0.2), (near(-60.4) + 2 * DF2, 1280, 1.0, 0.2)],
                   passes=[P0, P1]),
}
# the scenes in which the two builds of the reference are compared byte for byte: few jiggles, so that no soft value comes within 1e-4 of
# an integer (with 65 or 129 jiggles of 162 values one always does); the others are held to the cap of 1 % and one count
AB_BYTEWISE = ("strong", "driftp", "driftm", "early", "late", "jig_a", "jig_c", "quick_hit", "twelve", "minsync_a", "minsync_b", "silence")


def scene_inputs(name):
    s = SCENES[name]
    x = samples(s["seed"], s["signals"], s.get("silent", False))
    cands = np.zeros(len(s["cands"]), cand_in_dtype)
    for k, c in enumerate(s["cands"]):
        cands[k] = (np.float32(c[0]), c[1], c[2], c[3])
    return x, cands, np.array(s["passes"], np.int32).reshape(-1, 3)


def scene_file(name, path):
    x, cands, passes = scene_inputs(name)
    with open(path, "wb") as f:
        f.write(np.array([cands.size, passes.shape[0]], np.int32).tobytes())
        f.write(np.ascontiguousarray(x.real, np.float32).tobytes())
        f.write(np.ascontiguousarray(x.imag, np.float32).tobytes())
        f.write(cands.tobytes())
        f.write(passes.tobytes())
    return x, cands, passes


def scene_sha(name):
    x, cands, passes = scene_inputs(name)
    return np.frombuffer(digest(x.tobytes() + cands.tobytes() + passes.tobytes()), np.uint8)


# ---- fano alone: deinterleaved symbol sets
def soft_set(mseed, seed, sigma):
    """the code bits of a message as soft symbols around 128 -+ 60 with integer noise of about sigma"""
    _, _, code = encode(message_bits(mseed))
    r = rng(seed)
    n = r.integers(-sigma, sigma + 1, (3, NSYM)).sum(axis=0) if sigma else 0
    return np.clip(128 + 60 * (2 * code - 1) + n, 0, 255).astype(np.uint8)


def fano_sets():
    """name -> (symbols uint8 [162], maxcycles)"""
    _, _, code = encode(message_bits(201))
    sat = (255 * code).astype(np.uint8)
    out = {
        "all128": (np.full(NSYM, 128, np.uint8), 200),
        "saturated": (sat, 200),
        "last_cycle": (sat, 1),                     # 81 cycles are what a clean set takes: finished within the last allowed cycle, and yet a timeout
        "random": (rng(202).integers(0, 256, NSYM).astype(np.uint8), 200),
        "random_1": (rng(203).integers(0, 256, NSYM).astype(np.uint8), 1),
        "clean": (soft_set(204, 205, 0), 200),
        "noisy": (soft_set(204, 207, 50), 1000),             # decodes after turning back
        "noisier": (soft_set(204, 209, 60), 1000),           # 11589 cycles
        "too_noisy": (soft_set(204, 205, 70), 200),           # times out
    }
    return out


# ---- running the harness binaries
def build_driver(tmp, defines=()):
    exe = os.path.join(str(tmp), "wspr_dec_host" + "".join("_" + d for d in defines))
    subprocess.run(["g++", "-O2", "-ffp-contract=off"] + ["-D" + d for d in defines] + ["-o", exe, os.path.join(ROOT, "tools", "wspr_dec_host_driver.cpp"), "-lm"], check=True)
    return exe


def table_file(mettab, tmp):
    path = os.path.join(str(tmp), "mettab.bin")
    np.ascontiguousarray(mettab, np.int32).tofile(path)
    return path


def run_scene(exe, name, tmp, mettab=None, expect=0, scene_path=None):
    """the twin (mettab given) or the reference harness (it writes its table) on a scene -> dict(recs [npass, ncand], jig [n, 162], mettab, watch)"""
    tmp = str(tmp)
    p = lambda n: os.path.join(tmp, n)
    if scene_path is None:
        scene_path = p("scene_%s.bin" % name)
        _, cands, passes = scene_file(name, scene_path)
        ncand, npass = cands.size, passes.shape[0]
    else:
        ncand, npass = (int(v) for v in np.fromfile(scene_path, np.int32, 2))
    args = [exe, scene_path, p("out.bin"), p("jig.bin"), table_file(mettab, tmp) if mettab is not None else p("mettab_ref.bin")]
    if mettab is not None:
        args.append(p("watch.bin"))
    r = subprocess.run(args)
    assert r.returncode == expect, (r.returncode, expect)
    if expect:
        return None
    got = dict(recs=np.fromfile(p("out.bin"), rec_dtype).reshape(npass, ncand), jig=np.fromfile(p("jig.bin"), np.uint8).reshape(-1, NSYM))
    if mettab is None:
        got["mettab"] = np.fromfile(p("mettab_ref.bin"), np.int32).reshape(2, 256)
    else:
        got["watch"] = np.fromfile(p("watch.bin"), np.dtype([("least", "<f4"), ("strict", "<i4"), ("int_dist", "<f4")]))
    return got


def run_fano(exe, sets, maxcycles, mettab, tmp, expect=0):
    tmp = str(tmp)
    np.ascontiguousarray(sets, np.uint8).reshape(-1, NSYM).tofile(os.path.join(tmp, "syms.bin"))
    n = np.asarray(sets).reshape(-1, NSYM).shape[0]
    r = subprocess.run([exe, "-f", os.path.join(tmp, "syms.bin"), str(n), str(int(maxcycles)), table_file(mettab, tmp), os.path.join(tmp, "fano.bin")])
    assert r.returncode == expect, (r.returncode, expect)
    return None if expect else np.fromfile(os.path.join(tmp, "fano.bin"), fano_dtype)


def load():
    return np.load(os.path.join(GOLD, "wspr_dec_ref.npz"))


def recs_of(g, name):
    return np.ascontiguousarray(g["s_%s_recs" % name]).view(rec_dtype)[..., 0]


def golden_conditions(g, size):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    R = lambda name: recs_of(g, name)
    reached = {}
    for name in SCENES:
        r = R(name)
        assert r.shape == (len(SCENES[name]["passes"]), len(SCENES[name]["cands"])), name
        for v in r["result"].ravel().tolist():
            reached.setdefault(v, set()).add(name)
        w = g["s_%s_watch" % name]
        assert (w["strict"] == 1).all(), name                                   # every winning ss strictly above its runner-up
        ab = g["s_%s_ab" % name]
        assert ab[0] <= 0.01 * max(ab[1], 1) and ab[2] <= 1, name                # the two builds' jiggle bytes
        if name in AB_BYTEWISE:
            assert ab[0] == 0 and (w["int_dist"] >= 1e-4).all(), name
        for ps, rows in enumerate(r):                                           # a decoded record holds what was sent
            for c in rows:
                if c["result"] == DECODED:
                    assert bytes(c["decdata"][:10]) in [channel_symbols(s[4])[1] for s in SCENES[name]["signals"]] and c["decdata"][10] == 0, name
                    assert c["ignore"] == 1
    for cls in (SKIPPED, MINSYNC1, NO_CHANGE, TIME_UP, DECODED):
        assert len(reached.get(cls, ())) >= 2, cls
    assert QUICK_MISS in reached
    # the scenes reach what they are named for
    one = lambda name, ps=0: R(name)[ps][0]
    assert one("strong")["drift1"] == 0.0 and one("strong")["idt"] == 1 and one("strong", 1)["result"] == SKIPPED                   # neither drift wins; a second pass skips
    assert one("driftp")["drift1"] == 2.5 and one("driftm")["drift1"] == -1.5
    assert one("early")["shift1"] < 0 and one("early")["result"] == DECODED                                                     # symbols at k <= 0, and k == 0 inside a sum
    assert one("late")["shift1"] + 162 * 256 > TPOINTS and one("late")["result"] == DECODED                                   # the last symbols at k >= np
    assert one("jig_a")["result"] == one("jig_b")["result"] == DECODED and one("jig_a")["ii"] > 0 and one("jig_b")["ii"] > 0 and one("jig_b")["idt"] > 8
    assert one("jig_c")["result"] == one("jig_d")["result"] == DECODED and one("jig_c")["ii"] < 0 and one("jig_d")["ii"] < 0
    assert one("timeup_a")["result"] == TIME_UP and one("timeup_a")["idt"] == 65 and 0 < one("timeup_a")["gates"] < 65 and one("timeup_a")["ignore"] == 0
    assert one("timeup_a", 1)["idt"] == 129 and one("timeup_a", 1)["result"] == TIME_UP                                          # 129 jiggles
    assert one("timeup_b")["result"] == TIME_UP and one("timeup_b", 1)["result"] == DECODED and one("timeup_b", 1)["ii"] % 2 == 1  # found only at iifac 1
    assert one("nochange_a")["result"] == NO_CHANGE and one("nochange_a")["gates"] == 0 and one("nochange_a")["idt"] == 65 and one("nochange_a", 1)["result"] == SKIPPED
    assert one("minsync_a")["result"] == MINSYNC1 and one("minsync_a")["idt"] == 0 and (one("minsync_a")["tr_sync"][4:] == 0).all()
    s = one("silence")
    assert s["result"] == MINSYNC1 and s["f1"] == 0.0 and s["shift1"] == 0 and s["sync1"] == np.float32(-1e30)                  # to the letter
    assert one("quick_hit")["result"] == DECODED and one("quick_miss")["result"] == QUICK_MISS and one("quick_miss")["idt"] == 1 and one("quick_miss")["ignore"] == 0
    t = R("twelve")
    assert (t[0]["result"] == DECODED).sum() >= 4 and (t[0]["result"] == MINSYNC1).sum() >= 4 and (t[1]["result"] == SKIPPED).all()
    f = lambda n: g["f_%s" % n].view(fano_dtype)[0]
    assert f("last_cycle")["ok"] == 0 and f("last_cycle")["cycles"] == 82 and bytes(f("last_cycle")["data"]) == bytes(f("saturated")["data"])    # finished, and yet a timeout
    assert f("random")["ok"] == 0 and f("random")["cycles"] == 200 * 81 + 2 and f("random_1")["cycles"] == 83 and f("all128")["ok"] in (0, 1)
    assert f("noisy")["ok"] == 1 and f("noisy")["cycles"] > 82                                                                     # it had to turn back
    assert g["mettab"].shape == (2, 256) and (g["mettab"][0] == g["mettab"][1][::-1]).all() and g["ab_total"][3] == 0 and g["ab_total"][2] > 100000
    assert size <= 400 * 1024
