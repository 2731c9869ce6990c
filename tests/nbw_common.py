"""What the Wild noise-blanker tests share (tests/test_nbw_cpu.py, test_nbw_gpu.py, test_nbw_bank_gpu.py, tools/fuzz_parity.py,
tools/make_ref_nbw_golden.py): the seeded pool of int16 streams, the scenarios of tests/golden/nbw_ref.npz and their inputs rebuilt
from the pool, the digests, and the host driver tools/nbw_host_driver.cpp (csrc/kg_nbw.h compiled for the host with the reference's
flags)."""
import os
import subprocess

import numpy as np

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 512
HIST = 120
REC = 4 * 4 + 4 + HIST * 4          # one S record: int32 taps, impulse_samples, nb_algo, nb_enable[NB_BLANKER]; float thresh; hist[120]
RATE = 12000.0
SEED = 0x4E425701
POOL_BLOCKS = {"speech": 48, "clicks": 56, "quiet": 32, "loud": 24}


def i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _tones(n, t, amps):
    return sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in amps)


def pool():
    """name -> int16 stream.  One generator, drawn in a fixed order; the golden file holds each stream's digest."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    out = {}
    # noisy speech-like: a gated harmonic series on a strong noise floor (the detector fires all the time at the default threshold)
    n = POOL_BLOCKS["speech"] * BLK
    t = np.arange(n) / RATE
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    gate = 0.5 * (1 + np.sin(2 * np.pi * 3.1 * t)) ** 2
    out["speech"] = i16(gate * (3000 * np.sin(ph) + 1800 * np.sin(3 * ph + 0.4) + 900 * np.sin(5 * ph + 1.1)) + 900 * rng.standard_normal(n))
    # tones on a low noise floor with sparse clicks of one to three samples
    n = POOL_BLOCKS["clicks"] * BLK
    t = np.arange(n) / RATE
    x = _tones(n, t, [(2500, 500, 0.0), (2000, 1000, 0.3), (1000, 1800, 1.0)]) + 60 * rng.standard_normal(n)
    for b in range(POOL_BLOCKS["clicks"]):
        if rng.random() < 0.4:
            for _ in range(int(rng.integers(1, 4))):
                p = b * BLK + int(rng.integers(0, BLK - 3))
                w = int(rng.integers(1, 4))
                x[p:p + w] += rng.choice([-1.0, 1.0]) * rng.uniform(9000, 16000)
    out["clicks"] = i16(x)
    # the same kind of signal without a click: the base of the scenarios that place their own
    n = POOL_BLOCKS["quiet"] * BLK
    t = np.arange(n) / RATE
    out["quiet"] = i16(_tones(n, t, [(3000, 450, 0.2), (1500, 1250, 0.0), (800, 2100, 2.0)]) + 40 * rng.standard_normal(n))
    # close to full scale, with clicks: do the repairs leave int16?
    n = POOL_BLOCKS["loud"] * BLK
    t = np.arange(n) / RATE
    x = _tones(n, t, [(26000, 450, 0.0), (5000, 2900, 0.5)]) + 300 * rng.standard_normal(n)
    for b in range(POOL_BLOCKS["loud"]):
        p = b * BLK + int(rng.integers(40, BLK - 40))
        x[p:p + 2] -= np.sign(x[p]) * 30000
    out["loud"] = i16(x)
    return out


def load():
    return np.load(os.path.join(GOLD, "nbw_ref.npz"))


def names(g):
    return [str(n) for n in g["names"]]


def script(g, name):
    return [str(l) for l in g[name + "_script"]]


def make_input(streams, src, off, nb, zero, clicks):
    """blocks off .. off + nb of a pool stream, the listed blocks zeroed, then the scenario's own clicks (sample, width, amplitude)
    added (saturating)"""
    x = streams[src][off * BLK:(off + nb) * BLK].astype(np.int32)
    assert x.size == nb * BLK, "the pool stream is too short"
    for z in zero:
        x[int(z) * BLK:(int(z) + 1) * BLK] = 0
    for p, w, a in clicks:
        x[int(p):int(p) + int(w)] += int(a)
    return np.clip(x, -32768, 32767).astype(np.int16)


def scenario_input(g, name, streams):
    nb = sum(1 for l in script(g, name) if l[0] == "B")
    return make_input(streams, str(g[name + "_src"]), int(g[name + "_off"]), nb, g[name + "_zero"], g[name + "_clicks"].reshape(-1, 3))


def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "nbw_host_driver")


def split_states(raw):
    assert len(raw) % REC == 0
    out = []
    for i in range(len(raw) // REC):
        r = raw[i * REC:(i + 1) * REC]
        out.append((np.frombuffer(r[:16], np.int32), np.frombuffer(r[16:20], np.float32), np.frombuffer(r[20:], np.float32)))
    return out


def split_trace(raw):
    """-> (hits int32[blocks], largest |float| handed to the int16 conversion float32[blocks])"""
    a = np.frombuffer(raw, np.int32).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy().view(np.float32)


def run_driver(exe, lines, x, tmpdir):
    """-> (int16 output, state records (ints[4], thresh[1], hist[120]), hits per stage block, max |float| per stage block, exit status)"""
    P = lambda f: os.path.join(str(tmpdir), f)
    open(P("s.txt"), "w").write("\n".join(lines) + "\n")
    np.ascontiguousarray(x, np.int16).tofile(P("in.bin"))
    r = subprocess.run([exe, P("s.txt"), P("in.bin"), P("out.bin"), P("st.bin"), P("tr.bin")])
    if r.returncode:
        return None, None, None, None, r.returncode
    hits, mx = split_trace(open(P("tr.bin"), "rb").read())
    return np.fromfile(P("out.bin"), np.int16), split_states(open(P("st.bin"), "rb").read()), hits, mx, 0


def check_blocks(name, y, g, what):
    """every 512-sample block of y against the scenario's per-block digests (and the full output where the file holds it)"""
    want = g[name + "_out_sha"]
    assert y.size == want.shape[0] * BLK, (name, what, y.size)
    if name + "_out" in g.files:
        bad = np.flatnonzero(y != g[name + "_out"])
        assert bad.size == 0, (name, what, "first differing sample", int(bad[0]), int(y[bad[0]]), int(g[name + "_out"][bad[0]]))
    for b in range(want.shape[0]):
        assert digest(y[b * BLK:(b + 1) * BLK].tobytes()) == bytes(want[b]), (name, what, "block", b)


def check_state(name, k, ints, thresh, hist, g, what):
    """the k-th S record of the scenario: taps, impulse_samples, thresh bit for bit, the carried history bit for bit"""
    wi, wt, wh = g[name + "_state_i"][k], g[name + "_state_t"][k], g[name + "_state_h"][k]
    assert [int(v) for v in ints[:2]] == [int(v) for v in wi[:2]], (name, what, k, ints, wi)
    assert np.float32(thresh).view(np.uint32) == np.float32(wt).view(np.uint32), (name, what, k, thresh, wt)
    assert np.array_equal(np.ascontiguousarray(hist, np.float32).view(np.uint32), wh.view(np.uint32)), (name, what, k)


def random_script(rng):
    """A random script the library accepts (tools/fuzz_parity.py, tests/test_nbw_cpu.py): the three parameter messages, single
    re-inits in mid-stream over the whole range of taps and impulse_samples, the enable off and on, another algo and back, a new
    connection, stereo blocks.  A new connection zeroes the stored vector and keeps the stage's own (memset(s); nb_Wild[ch] stays):
    the stage comes back on over the kept vector, and the first parameter change after that is the whole three-message sequence
    with the stage off, as a client sends it -- a single message would init from a vector of zeros, which the library refuses
    while the stage is on."""
    def value(k):
        return ["%.9g" % 10 ** rng.uniform(-0.3, 0.8), "%d" % rng.integers(1, 41), "%d" % rng.integers(2, 42)][k]
    three = lambda: ["P 0 %d %s" % (k, value(k)) for k in range(3)]
    lines = ["A 2"] + three() + ["E 0 1"]
    zeroed = False
    for b in range(int(rng.integers(6, 40))):
        r = rng.random()
        if r < 0.10:
            if zeroed:
                lines += ["E 0 0"] + three() + ["E 0 1"]
                zeroed = False
            else:
                k = int(rng.integers(0, 3))
                lines.append("P 0 %d %s" % (k, value(k)))
        elif r < 0.14:
            lines += ["E 0 0", "B 512 0", "E 0 1"]
        elif r < 0.17:
            lines += ["A %d" % rng.integers(0, 2), "B 512 0", "A 2", "E 0 1"]
        elif r < 0.19:
            lines += ["C", "B 512 0", "A 2", "E 0 1"]
            zeroed = True
        elif r < 0.21:
            lines.append("P %d %d %s" % (rng.integers(1, 4), rng.integers(0, 8), value(0)))      # another type: stored, no init
        lines.append("B 512 %d" % (rng.random() < 0.05))
    lines.append("S")
    return lines


# ---- replaying a scenario's script on a kg_post channel (GPU tests, tools/fuzz_parity.py) ----
class Replay:
    """One scenario's script on channel ch of P, a command at a time, with the command state of snd_t kept here as kg_rxbank keeps it
    (kg_post holds the stage's vector and switch only): step() runs commands up to the next block and returns it (or None at the
    end); the caller runs the stage and hands the output to done()."""

    def __init__(self, P, ch, lines, x):
        self.P, self.ch, self.lines, self.x = P, ch, list(lines), x
        self.ip, self.pos, self.algo, self.on, self.out, self.states = 0, 0, 0, 0, [], []
        self.en = [0] * 4
        self.param = np.zeros((4, 8), np.float32)

    def step(self):
        """-> (int16[512], runs the stage?) of the next block, or None"""
        P, ch = self.P, self.ch
        while self.ip < len(self.lines):
            f = self.lines[self.ip].split()
            self.ip += 1
            if f[0] == "A":
                self.algo, self.en, self.on = int(f[1]), [0] * 4, 0
                P.set_nbw(ch, 0)
            elif f[0] == "E":
                t, e = int(f[1]), int(f[2])
                if t == 0 and self.algo == 2:
                    P.set_nbw(ch, e)
                    self.on = int(bool(e))
                self.en[t] = e
            elif f[0] == "P":
                t, p = int(f[1]), int(f[2])
                v = self.param[t].copy()
                v[p] = np.float32(f[3])
                if t == 0 and self.algo == 2:
                    P.nbw_init(ch, v)
                self.param[t] = v
            elif f[0] == "C":
                self.algo, self.en, self.on = 0, [0] * 4, 0
                self.param[:] = 0
                P.reset(ch)
            elif f[0] == "S":
                self.states.append(P.nbw_state([ch]))
            elif f[0] == "B":
                assert int(f[1]) == BLK
                blk = self.x[self.pos:self.pos + BLK]
                self.pos += BLK
                return blk, (not int(f[2])) and bool(self.on)
        return None

    def peek_is_block(self):
        """the next script line is a block that runs the stage (so it can share a multi-block call with the previous one)"""
        if self.ip >= len(self.lines):
            return False
        f = self.lines[self.ip].split()
        return f[0] == "B" and not int(f[2]) and bool(self.on)

    def done(self, y):
        self.out.append(np.asarray(y, np.int16).reshape(-1))

    def output(self):
        return np.concatenate(self.out)


def check_states(name, states, g, what):
    """the S snapshots of a replay (Post.nbw_state dicts) against the scenario's"""
    assert len(states) == len(g[name + "_state_i"]), (what, name)
    for k, st in enumerate(states):
        check_state(name, k, st["ints"][0], st["thresh"][0], st["hist"][0], g, what)
        assert int(st["ints"][0, 2]) == int(g[name + "_state_i"][k][3] and g[name + "_state_i"][k][2] == 2), (what, name, k, "the switch")
