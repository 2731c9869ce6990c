"""What the spectral noise-reduction tests share (tests/test_nrs_cpu.py, test_nrs_gpu.py, test_nrs_bank_gpu.py, tools/fuzz_parity.py):
the scenarios of tests/golden/nrs_ref.npz (tools/make_ref_nrs_golden.py), their inputs rebuilt from the pool, the digests, and the
host driver tools/nrs_host_driver.cpp (csrc/kg_nrs.h compiled for the host with the reference's flags)."""
import os
import subprocess

import numpy as np

from . import script_common
from .script_common import digest  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 512
ARRAYS = ("last_sample_buffer", "last_iFFT_result", "NR_Nest", "xt", "pslp", "NR_SNR_post", "NR_SNR_prio", "NR_Hk_old", "NR_G")
REC = 2 * 4 + 12 * 4 + 9 * 256 * 4


def load():
    return np.load(os.path.join(GOLD, "nrs_ref.npz"))


def names(g):
    return [str(n) for n in g["names"]]


def fdigest(a):
    """SHA-256 prefix of a float32 vector with every NaN as 0x7FC00000 (x86's default NaN is the negative quiet one, the GPU's the
    positive one; a NaN is compared as a NaN)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return digest(u.tobytes())


def script(g, name):
    return [str(l) for l in g[name + "_script"]]


def scenario_input(g, name):
    nb = sum(1 for l in script(g, name) if l[0] == "B")
    off = int(g[name + "_off"])
    x = g["pool_" + str(g[name + "_src"])][off * BLK:(off + nb) * BLK].copy()
    for z in g[name + "_zero"]:
        x[int(z) * BLK:(int(z) + 1) * BLK] = 0
    assert x.size == nb * BLK
    return x


def build_driver(tmpdir):
    return script_common.build_driver(tmpdir, "nrs_host_driver")


def run_driver(exe, rate, lines, x, tmpdir):
    """-> (int16 output, list of state records (ints[2], floats[12], arrays[9][256]), trace[blocks][5], exit status)"""
    P = lambda f: os.path.join(str(tmpdir), f)
    open(P("s.txt"), "w").write("\n".join(lines) + "\n")
    np.ascontiguousarray(x, np.int16).tofile(P("in.bin"))
    r = subprocess.run([exe, str(int(rate)), P("s.txt"), P("in.bin"), P("out.bin"), P("st.bin"), P("tr.bin")])
    if r.returncode:
        return None, None, None, r.returncode
    y = np.fromfile(P("out.bin"), np.int16)
    raw = open(P("st.bin"), "rb").read()
    assert len(raw) % REC == 0
    states = []
    for i in range(len(raw) // REC):
        rec = raw[i * REC:(i + 1) * REC]
        states.append((np.frombuffer(rec[:8], np.int32), np.frombuffer(rec[8:56], np.float32), np.frombuffer(rec[56:], np.float32).reshape(9, 256)))
    return y, states, np.fromfile(P("tr.bin"), np.int32).reshape(-1, 5), 0


def check_blocks(name, y, g, what):
    """every 512-sample block of y against the scenario's per-block digests (and the full output where the file holds it)"""
    want = g[name + "_out_sha"]
    assert y.size == len(want) * BLK, (what, name, y.size)
    bad = [b for b in range(len(want)) if digest(y[b * BLK:(b + 1) * BLK].tobytes()) != bytes(want[b])]
    assert not bad, (what, name, "blocks that differ from the reference", bad)
    if name + "_out" in g.files:
        assert np.array_equal(y, g[name + "_out"]), (what, name)


# ---- replaying a scenario's script on a kg_post channel (GPU tests, tools/fuzz_parity.py) ----
class Replay:
    """One scenario's script on channel ch of P, a command at a time: step() runs commands up to the next block and returns it
    (or None at the end); the caller runs the stage and hands the output to done()."""

    def __init__(self, P, ch, lines, x):
        from flydog_sdr_gps_amd import post
        self.post, self.P, self.ch, self.lines, self.x = post, P, ch, list(lines), x
        self.ip, self.pos, self.algo, self.out, self.states = 0, 0, 0, [], []

    def step(self):
        """-> (int16[512], runs the stage?) of the next block, or None"""
        P, ch, post = self.P, self.ch, self.post
        while self.ip < len(self.lines):
            f = self.lines[self.ip].split()
            self.ip += 1
            if f[0] == "A":
                self.algo = int(f[1])
                if self.algo == post.NR_SPECTRAL:
                    P.nrs_select(ch)
                else:
                    P.set_nr_algo(ch, self.algo)
            elif f[0] == "E":
                P.set_nr_enable(ch, int(f[1]), int(f[2]))
            elif f[0] == "P":
                P.set_nr_param(ch, int(f[1]), int(f[2]), np.float32(f[3]))
            elif f[0] == "M":
                P.nrs_passband(ch, float(f[1]), float(f[2]))
            elif f[0] == "C":
                self.algo = 0
                P.reset(ch)
            elif f[0] == "S":
                self.states.append(P.nrs_state([ch]))
            elif f[0] == "B":
                assert int(f[1]) == BLK
                blk = self.x[self.pos:self.pos + BLK]
                self.pos += BLK
                return blk, (not int(f[2])) and self.algo == post.NR_SPECTRAL
        return None

    def peek_is_block(self):
        """the next script line is a block that runs the stage (so it can share a multi-block call with the previous one)"""
        if self.ip >= len(self.lines):
            return False
        f = self.lines[self.ip].split()
        return f[0] == "B" and not int(f[2]) and self.algo == self.post.NR_SPECTRAL

    def done(self, y):
        self.out.append(np.asarray(y, np.int16).reshape(-1))

    def output(self):
        return np.concatenate(self.out)


def check_states(name, states, g, what):
    """the S snapshots of a replay (Post.nrs_state dicts) against the scenario's: first_time, init_counter, the scalars bit for bit,
    the rate constants once the state was initialised (the reference computes them at the first init), the nine arrays by digest"""
    si, sf, sha = g[name + "_state_i"], g[name + "_state_f"], g[name + "_state_sha"]
    assert len(states) == len(si), (what, name)
    for k, st in enumerate(states):
        assert list(st["ints"][0, :2]) == list(si[k]), (what, name, k, st["ints"][0], si[k])
        sc = st["scalars"][0]
        got = np.array([sc[0], sc[1], sc[2], sc[4], sc[5]], np.float32)
        assert np.array_equal(got.view(np.uint32), sf[k][:5].view(np.uint32)), (what, name, k, got, sf[k][:5])
        assert np.array_equal(sc[6:8].view(np.uint32), sf[k][10:12].view(np.uint32)), (what, name, k, "norm_locut / norm_hicut", sc[6:8], sf[k][10:12])
        if si[k][0] != 0:
            assert np.array_equal(st["rate"][:5].view(np.uint32), sf[k][5:10].view(np.uint32)), (what, name, k, "tinc .. ap", st["rate"], sf[k][5:10])
        for a in range(9):
            assert fdigest(st["arrays"][0, a]) == bytes(sha[k][a]), (what, name, k, ARRAYS[a])
