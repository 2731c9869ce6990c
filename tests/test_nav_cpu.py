"""Nav frame sync without a GPU: the model (tests/nav_model.py) against the reference's own records (tests/golden/nav_ref.npz, made by
tools/make_ref_nav_golden.py), the encoders of flydog_sdr_gps_amd/nav.py through the model, kg_nav.h's host build
(tools/nav_host_driver.cpp, plain and under the address / undefined-behaviour sanitizers, a stand-alone program) against both, the
exported symbols, and the derived bound on the records of a push."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import nav
from . import nav_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = {nav.L1: ((16,), (17,), (299,), (301,)), nav.E1B: ((16,), (17,), (499,), (501,))}
NAV_SYMBOLS = {"kg_nav_create": 3, "kg_nav_destroy": 1, "kg_nav_set_mode": 3, "kg_nav_push_bits_dev": 8, "kg_nav_push_bits": 8,
               "kg_nav_push_epochs_dev": 9, "kg_nav_get_state": 7}


def load_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "nav_ref.npz"))
    out = {}
    for name in g["names"]:
        name = str(name)
        n = int(g[name + "_nbits"][0])
        out[name] = dict(mode=int(g[name + "_mode"][0]), bits=np.unpackbits(g[name + "_bits"])[:n].copy(),
                         frames=g[name + "_frames"].copy().view(nm.frame_dtype).reshape(-1), hold=tuple(int(v) for v in g[name + "_hold"]))
    return out


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def model_runs(golden):
    """the model on every golden stream, in one push: computed once"""
    return {name: nm.run(s["mode"], s["bits"]) for name, s in golden.items()}


def same_frames(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (what, "record %d" % k, a, b)


def test_golden_holds_what_the_generator_promised(golden):
    fr = {m: np.concatenate([s["frames"] for s in golden.values() if s["mode"] == m]) for m in (nav.L1, nav.E1B)}
    ca, e1 = fr[nav.L1], fr[nav.E1B]
    assert (ca["err"] == 0).sum() >= 20 and ((ca["err"] == nav.ERR_PARITY) & (ca["id"] > 0)).sum() >= 5
    assert (e1["err"] == 0).sum() >= 20 and (e1["err"] == nav.ERR_SLIP).sum() >= 3 and (e1["err"] == nav.ERR_CRC).sum() >= 5
    assert (e1["err"] == nav.ERR_ALERT).sum() >= 1 and (e1["err"] == nav.ERR_OOS).sum() >= 2
    assert set(ca["inverted"]) == {0, 1} and set(e1["inverted"]) == {0, 1}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "nav_ref.npz")) < 1 << 20


def test_model_equals_the_reference(golden, model_runs):
    for name, s in golden.items():
        fr, c = model_runs[name]
        same_frames(fr, s["frames"], name)
        assert (len(c.buf), c.base) == s["hold"], name


def test_model_does_not_depend_on_the_cuts(golden):
    for name in ("ca_bit_error_w3", "ca_random_2", "ca_back_to_back_preambles", "e1b_odd_start_inverted", "e1b_chance_pair_in_page"):
        s = golden[name]
        for cuts in CUTS[s["mode"]] + ((1,),):
            fr, c = nm.run(s["mode"], s["bits"], cuts)
            same_frames(fr, s["frames"], (name, cuts))
            assert (len(c.buf), c.base, c.pushed) == s["hold"] + (s["bits"].size,), (name, cuts)


def test_encoders_round_trip_through_the_model():
    rng = np.random.default_rng(11)
    d29 = d30 = 0
    stream, words = [], []
    for k in range(3):
        w = [int(v) for v in rng.integers(0, 1 << 24, 10)]
        w[0] = (0x8B << 16) | (w[0] & 0xFFFF)
        f = nav.l1_subframe(w, d29, d30)
        while f[-2] != f[-1]:                           # ParityCheck starts a subframe from D29 = D30 (the system sends 0 0)
            w[9] = int(rng.integers(0, 1 << 24))
            f = nav.l1_subframe(w, d29, d30)
        d29, d30 = int(f[-2]), int(f[-1])
        stream.append(f)
        words.append(w)
    fr, _ = nm.run(nav.L1, np.concatenate(stream))
    assert len(fr) == 3 and (fr["err"] == 0).all() and fr["bit"].tolist() == [0, 300, 600]
    for r, w in zip(fr, words):
        got = np.unpackbits(r["data"])[:300].reshape(10, 30)[:, :24]
        assert [int("".join(str(b) for b in row), 2) for row in got] == w
        assert r["id"] == (w[1] >> 2) & 7
    for inverted in (0, 1):
        w = rng.integers(0, 2, 128).astype(np.uint8)
        res = rng.integers(0, 2, 64).astype(np.uint8)
        page = nav.e1b_page(w, inverted=inverted, reserved=res)
        fr, _ = nm.run(nav.E1B, np.concatenate([page, page]))
        assert len(fr) == 2 and (fr["err"] == 0).all() and (fr["inverted"] == inverted).all() and (fr["consumed"] == 500).all()
        bits = np.unpackbits(fr[0]["data"][:30])
        assert np.array_equal(bits[2:114], w[:112]) and np.array_equal(bits[122:138], w[112:]) and np.array_equal(bits[138:202], res)
        assert fr[0]["id"] == int("".join(str(b) for b in w[:6]), 2) and not bits[114:120].any()


# ---- kg_nav.h on the host
def build_driver(tmpdir, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/nav_host_driver.cpp"
    exe = os.path.join(str(tmpdir), name)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tools", "nav_host_driver.cpp")], check=True)
    return exe


def run_driver(exe, script):
    """-> [(frames, state dict, bound) per push]"""
    p = subprocess.run([exe], input=script.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    out, recs = [], []
    for line in p.stdout.decode().splitlines():
        f = line.split(" ")
        if f[0] == "F":
            r = np.zeros((), nm.frame_dtype)
            r["bit"], r["err"], r["consumed"], r["inverted"], r["id"] = (int(v) for v in f[1:6])
            r["data"] = np.frombuffer(bytes.fromhex(f[6]), np.uint8)
            recs.append(r)
        elif f[0] == "H":
            st = dict(holding=int(f[1]), bit0=int(f[2]), pushed=int(f[3]), nav_ms=int(f[4]), nav_prev=int(f[5]), nav_glitch=int(f[6]),
                      held=np.array([int(ch) for ch in f[7]], np.uint8))
            out.append((nm.frames(recs), st, int(f[8])))
            recs = []
    return out


def bitstr(bits):
    return "".join("01"[int(b) & 1] for b in bits)


def same_state(got, want, what):
    for k in ("holding", "bit0", "pushed", "nav_ms", "nav_prev", "nav_glitch"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["held"], want["held"]), what


def epoch_flags(rng, n, mode):
    """Inav per epoch: runs of 20 with a few glitches (C/A), random (E1B)"""
    if mode == nav.E1B:
        return rng.integers(0, 2, n).astype(np.uint8)
    f = np.repeat(rng.integers(0, 2, n // 20 + 2), 20)[7:7 + n].astype(np.uint8)
    f[rng.choice(n, max(n // 90, 1), replace=False)] ^= 1
    return f


def driver_script(golden):
    """every golden stream in one push and in its cuts, then the nav-bit machine; -> (script, [(what, model frames, model state) per push])"""
    script, want = [], []
    rng = np.random.default_rng(5)
    for name, s in golden.items():
        for cuts in (None,) + CUTS[s["mode"]]:
            script.append("T %d" % s["mode"])
            c = nm.Channel(s["mode"])
            at, k = 0, 0
            while at < s["bits"].size:
                n = s["bits"].size if cuts is None else cuts[k % len(cuts)]
                script.append("P " + bitstr(s["bits"][at:at + n]))
                want.append(((name, cuts, at), nm.frames(c.push(s["bits"][at:at + n])), c.state()))
                at += n
                k += 1
    for mode, bits in ((nav.L1, golden["ca_upright"]["bits"]), (nav.E1B, golden["e1b_upright"]["bits"])):
        per = 20 if mode == nav.L1 else 1
        flags = np.repeat(bits[:40 if mode == nav.L1 else 700], per)
        flags = np.concatenate([flags, epoch_flags(rng, 333, mode)])
        script.append("T %d" % mode)
        c = nm.Channel(mode)
        for a in range(0, flags.size, 211):
            script.append("E " + bitstr(flags[a:a + 211]))
            want.append((("epochs", mode, a), nm.frames(c.push(c.nav_bits(flags[a:a + 211]))), c.state()))
    return "\n".join(script) + "\n", want


@pytest.fixture(scope="module")
def driver_case(golden):
    return driver_script(golden)


def check_driver(exe, golden, case):
    script, want = case
    got = run_driver(exe, script)
    assert len(got) == len(want)
    nrec = 0
    for (fr, st, bound), (what, wfr, wst) in zip(got, want):
        same_frames(fr, wfr, what)
        same_state(st, wst, what)
        assert len(fr) <= bound, what
        nrec += len(fr)
    assert nrec > 4 * sum(len(s["frames"]) for s in golden.values())


def test_host_build_equals_the_model(tmp_path, golden, driver_case):
    check_driver(build_driver(tmp_path, "nav_host", []), golden, driver_case)


def test_host_build_under_sanitizers(tmp_path, golden, driver_case):
    exe = build_driver(tmp_path, "nav_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_driver(exe, golden, driver_case)


def test_library_exports_the_nav_symbols():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, nargs in NAV_SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m and len(m.group(1).split(",")) == nargs, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert getattr(lib, s) is not None
    assert not re.search(r"\bvoid\s*\*\s*d_\w+", "".join(re.findall(r"kg_nav_\w+\s*\([^;]*\)\s*;", header))), "every device pointer of kg_nav is typed"


# ---- the bound on the records of one push
def test_cap_bound_against_the_model():
    """cap >= ceil(nbits / 30) (C/A), ceil(nbits / 250) (E1B): never exceeded, and reached, on streams of back-to-back preambles whose
    heads each drop the least a record can drop -- a parity failure in word 0, a slip -- pushed behind a tail of 299 / 499 held bits"""
    rng = np.random.default_rng(3)
    ca = np.concatenate([np.concatenate([nav.L1_PREAMBLE, rng.integers(0, 2, 22).astype(np.uint8)]) for _ in range(40)])
    odd = nav.e1b_page(rng.integers(0, 2, 128).astype(np.uint8))[250:]
    e1 = np.tile(odd, 8)
    reached = {nav.L1: 0, nav.E1B: 0}
    for mode, stream, sizes in ((nav.L1, ca, (1, 29, 30, 31, 60, 61, 299, 300, 301, 700)), (nav.E1B, e1, (1, 249, 250, 251, 500, 501, 1100))):
        sub = nav.SUBFRAME_BITS[mode]
        for n in sizes:
            c = nm.Channel(mode)
            assert c.push(stream[:sub - 1]) == [] and len(c.buf) == sub - 1
            recs = c.push(stream[sub - 1:sub - 1 + n])
            bound = nav.cap_for([mode], [n])
            assert len(recs) <= bound, (mode, n, len(recs), bound)
            reached[mode] += len(recs) == bound
            c = nm.Channel(mode)                        # and from an empty channel
            assert len(c.push(stream[:n])) <= bound
    assert reached[nav.L1] >= 8 and reached[nav.E1B] == 7, reached
    assert nav.cap_for([nav.L1, nav.E1B], [0, 0]) == 0 and nav.cap_for([nav.L1, nav.E1B], [31, 251]) == 2
    assert nav.cap_for_epochs([nav.L1, nav.E1B], 600) == max(-(-30 // 30), -(-600 // 250))
