"""What the audio-spectrum tests share (tests/test_spec_cpu.py, test_spec_gpu.py, test_spec_bank_gpu.py,
tools/make_ref_spec_golden.py): the seeded pool of 1024-point spectra that tests/golden/spec_ref.npz was made from (the file holds
the pool's digest, not the spectra), the limiter's clock scripts, the emission scripts, and the host driver
tools/spec_host_driver.cpp (csrc/kg_spec.h compiled for the host with the reference's flags).

No spectrum of the pool holds a NaN: (int) NaN is undefined in the reference, so NaN input is outside the row's contract."""
import os
import subprocess

import numpy as np

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W = 1024
SEED = 0x53504543
PASSBAND, CHAN_NULL = 0, 1
# rx_sound.cpp:201-202 in float, left to right (the golden decides; these only place the edge set)
_S0 = np.float32(20.0) / (np.float32(32767.0) * np.float32(32767.0) * np.float32(1024.0) * np.float32(1024.0))
SCALE = (np.float32(_S0 * np.float32(1e6)), np.float32(_S0 * np.float32(0.0004)))
# the reference's mode_e numbers (rx/mode.h:69-70), by name, for the emission scripts
MODES = ["AM", "AMN", "USB", "LSB", "CW", "CWN", "NBFM", "IQ", "DRM", "USN", "LSN", "SAM", "SAU", "SAL", "SAS", "QAM", "NNFM"]
NULL_LSB, NULL_USB = 1, 2                       # CHAN_NULL_LSB, CHAN_NULL_USB (rx/wdsp/wdsp.h:7-8)


EDGE_STEPS = (-64, -16, -3, -1, 0, 1, 3, 16, 64)


def _edge(inst):
    """re with pwr * scale within a few ulps of 10^(k/10) for every integer k in -200..0: where the (int) truncation decides.
    Nine values per k, EDGE_STEPS ulps of re from the nearest float to the root.  One ulp of re moves the dB value by 1e-6, less
    than the float spacing of dB beyond -16 (1.5e-5 from -128 on), so the near neighbours round to the same dB as the centre; the
    +-64 ulp ones (6.6e-5 dB) are on either side of k for certain."""
    out = []
    for k in range(-200, 1):
        re0 = np.float32(np.sqrt(10.0 ** (k / 10.0) / float(SCALE[inst])))
        bits = int(re0.view(np.uint32))
        out += [np.uint32(bits + d).view(np.float32) for d in EDGE_STEPS]
    out = np.array(out, np.float32)                 # 201 * 9 = 1809 values: two rows
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
    add("zeros_signs_denormals", re, rng.standard_normal(W))
    # |re| log-uniform over 1e-12 .. 1e12: floor and ceiling both reached
    for r in range(8):
        re = rng.choice([-1.0, 1.0], W) * 10.0 ** rng.uniform(-12, 12, W)
        add("loguniform_%d" % r, re, rng.choice([-1.0, 1.0], W) * 10.0 ** rng.uniform(-12, 12, W))
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
    for inst in (PASSBAND, CHAN_NULL):
        e = _edge(inst)
        for r in range(2):
            add("edge_%s_%d" % ("null" if inst else "pb", r), e[r] * rng.choice([-1.0, 1.0], W).astype(np.float32), rng.standard_normal(W))
    spec = np.stack(rows)
    assert not np.isnan(spec.real).any() and not np.isnan(spec.imag).any()
    return names, spec


def load():
    return np.load(os.path.join(GOLD, "spec_ref.npz"))


# ---- Pin 2: the limiter's clocks (ms), one connection each
def limiter_scripts():
    blk12k, blk20k = 512 / 12000.0 * 1e3, 512 / 20250.0 * 1e3      # 42.67 and 25.28 ms a sound block
    return {
        "first_at_125": [125, 126, 200, 251, 252, 376, 377],
        "first_below": [0, 1, 60, 124, 125, 130, 254, 255, 256],
        "first_above": [126, 127, 251, 252, 300, 377],
        "cadence_42_67": [int(1000 + k * blk12k) for k in range(60)],
        "cadence_25_28": [int(777 + k * blk20k) for k in range(100)],
        "long_gap": [int(500 + k * blk12k) for k in range(12)] + [int(5000 + k * blk12k) for k in range(40)],
        "wraps": [4294967000, 4294967100, 4294967200, 4294967290, 5, 100, 200],
    }


# ---- Pin 3: emission scripts.  P n: `SET spc_=n`; M mode mparam n5: the mode command; B: a sound block
def _M(mode, mparam=0, n5=0):
    return "M %d %d %d" % (MODES.index(mode), mparam, n5)


def emit_scripts():
    B = lambda k: ["B"] * k
    walk = ([_M("USB")] + B(3) + [_M("SAM", 0, 1)] + B(3) + [_M("SAM", NULL_LSB, 1)] + B(4) + [_M("SAM", 0, 1)] + B(3) +
            [_M("SAM", NULL_USB, 1)] + B(4) + [_M("AM")] + B(3) + [_M("SAM", NULL_LSB, 1)] + B(4))
    return {
        "walk_spec_on": ["P 2"] + walk,
        "walk_spec_off": ["P 0"] + walk,
        "on_off_on": ["P 2", _M("USB")] + B(3) + ["P 0"] + B(3) + ["P 2"] + B(3) + ["P 1"] + B(2) + ["P 7"] + B(2) + ["P -1"] + B(2) + ["P 2"] + B(2),
        "null_on_off_on": ["P 0", _M("SAM", NULL_USB, 1)] + B(3) + ["P 2"] + B(3) + ["P 0"] + B(2) + ["P 2"] + B(3),
        "same_mode_without_n5": ["P 2", _M("SAM", NULL_LSB, 1)] + B(3) + [_M("SAM", 0, 0)] + B(3) + [_M("SAM", 0, 1)] + B(3),
        "other_sam_modes": ["P 2", _M("SAL", NULL_LSB, 1)] + B(2) + [_M("SAS", NULL_USB, 1)] + B(2) + [_M("QAM", NULL_LSB, 1)] + B(2) + [_M("SAM", NULL_LSB, 1)] + B(3),
    }


def emit_blocks(n):
    """the seeded blocks the stand-in CFastFIR objects hand over at their fills"""
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    c = np.empty((n, W), np.complex64)
    c.real = rng.choice([-1.0, 1.0], (n, W)) * 10.0 ** rng.uniform(-3, 7, (n, W))
    c.imag = rng.standard_normal((n, W))
    return c


def parse_emit(raw):
    """out.bin of the reference harness or the host driver -> per block a list of (instance, isChanNull, block index, row uint8[1024])"""
    out, at = [], 0
    while at < len(raw):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        at += 4
        rows = []
        for _ in range(n):
            iv = np.frombuffer(raw[at:at + 12], np.int32)
            rows.append((int(iv[0]), int(iv[1]), int(iv[2]), np.frombuffer(raw[at + 12:at + 12 + W], np.uint8).copy()))
            at += 12 + W
        out.append(rows)
    return out


def emit_golden(g, name):
    """-> per block a list of (instance, isChanNull, block index, row digest) from the golden file"""
    cnt, info, sha = g["emit_%s_count" % name], g["emit_%s_info" % name], g["emit_%s_sha" % name]
    out, at = [], 0
    for c in cnt:
        out.append([(int(info[at + i][0]), int(info[at + i][1]), int(info[at + i][2]), bytes(sha[at + i])) for i in range(int(c))])
        at += int(c)
    return out


# ---- the host driver
def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "spec_host_driver")


def host_rows(exe, spec, tmpdir):
    """-> uint8 [rows, 2, 1024]: every spectrum with the passband scale, then the channel-null one (kg_spec::row)"""
    P = lambda f: os.path.join(str(tmpdir), f)
    np.ascontiguousarray(spec, np.complex64).tofile(P("in.bin"))
    subprocess.run([exe, "rows", P("in.bin"), P("out.bin")], check=True)
    return np.fromfile(P("out.bin"), np.uint8).reshape(-1, 2, W)


def host_limiter(exe, clocks, tmpdir):
    """-> (fired int32[n], last_ms uint32[n])"""
    P = lambda f: os.path.join(str(tmpdir), f)
    np.array(clocks, np.uint32).tofile(P("clk.bin"))
    subprocess.run([exe, "limiter", P("clk.bin"), P("out.bin")], check=True)
    a = np.fromfile(P("out.bin"), np.uint32).reshape(-1, 2)
    return a[:, 0].astype(np.int32), a[:, 1].copy()


def host_emit(exe, lines, blocks, tmpdir):
    P = lambda f: os.path.join(str(tmpdir), f)
    open(P("s.txt"), "w").write("\n".join(lines) + "\n")
    np.ascontiguousarray(blocks, np.complex64).tofile(P("blk.bin"))
    subprocess.run([exe, "emit", P("s.txt"), P("blk.bin"), P("out.bin")], check=True)
    return parse_emit(open(P("out.bin"), "rb").read())

