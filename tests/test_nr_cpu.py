"""kg_nr.h, the per-sample arithmetic of c2s_sound()'s noise-reduction switch (rx/rx_sound.cpp:933-949: wdsp_ANR_filter and
CLMS::ProcessFilter) that kg_post's kernel runs, compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the
driver tools/nr_host_driver.cpp, against every unit scenario of tests/golden/nr_ref.npz (made by tools/make_ref_nr_golden.py from
the reference's own statements) -- BIT-EXACT: every output sample, the end states, the weight vectors through their digests.
Then the C ABI: the header's NR constants equal the reference's enum values and parameter indices, and the new entry points are
declared, bound and exported."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import script_common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NR_SYMBOLS = ("kg_post_set_nr_algo", "kg_post_set_nr_enable", "kg_post_set_nr_param", "kg_post_nr_process_dev", "kg_post_nr_state")
REC = 6 * 4 + 2 * 4 + 512 * 4 + 121 * 4


def digest(b):
    """SHA-256 prefix of a float32 vector's bytes with every NaN as 0x7FC00000 (tools/make_ref_nr_golden.py: a diverged filter's
    weights are NaN on either machine, with the sign bit of each machine's default NaN)"""
    u = np.frombuffer(bytes(b), np.uint32).copy()
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return script_common.digest(u.tobytes())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "nr_ref.npz"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host driver"
    exe = str(tmp_path_factory.mktemp("nr") / "nr_host_driver")
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "nr_host_driver.cpp")],
                   check=True)
    return exe


def test_unit_scenarios_bit_exact(golden, driver, tmp_path):
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 16
    for name in names:
        x = golden[name + "_in"]
        (tmp_path / "s.txt").write_text("\n".join(str(l) for l in golden[name + "_script"]) + "\n")
        x.tofile(str(tmp_path / "in.bin"))
        subprocess.run([driver, str(tmp_path / "s.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
        raw = (tmp_path / "out.bin").read_bytes()
        y = np.frombuffer(raw[:2 * x.size], np.int16)
        want = golden[name + "_out"]
        bad = np.flatnonzero(y != want)
        assert bad.size == 0, (name, bad.size, bad[:5], y[bad[:5]], want[bad[:5]])
        st = raw[2 * x.size:]
        assert len(st) == 2 * REC, name
        for t in range(2):
            r = st[t * REC:(t + 1) * REC]
            assert np.array_equal(np.frombuffer(r[:24], np.int32), golden[name + "_state_i"][t]), (name, t)
            assert np.array_equal(np.frombuffer(r[24:32], np.uint32), golden[name + "_state_f"][t].view(np.uint32)), (name, t)
            assert digest(r[32:32 + 2048]) == bytes(golden[name + "_w_sha"][t]), (name, t, "wdsp w[]")
            assert digest(r[32 + 2048:]) == bytes(golden[name + "_coef_sha"][t]), (name, t, "CLMS m_lmscoef[]")


def test_scenarios_cover_the_corners(golden):
    """the golden file exercises the corners: lidx held at lidx_min, the int16 wrap, the delay-line lengths.  (lidx_max is out of
    reach as written: with nev < nel, lidx rises by lincr and, unless that passes lidx_max, falls by ldecr at once -- from 120 it
    never gets above 121.)"""
    lidx = np.concatenate([golden[str(n) + "_state_f"][:, 0] for n in golden["names"]])
    assert (lidx == 120.0).any() and (lidx < 200.0).all()
    loud = golden["wdsp_loud_wrap_out"].astype(np.int32)
    assert np.abs(np.diff(loud)).max() > 32768                      # the (s2_t) cast wrapped
    dlens = {int(golden[str(n) + "_state_i"][t, 4]) for n in golden["names"] for t in range(2)}
    assert {0, 1, 17, 48, 300} <= dlens, dlens


def _header_enums():
    text = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    return {k: int(v) for k, v in re.findall(r"\bKG_(NR_[A-Z_]+)\s*=\s*(\d+)", text)}


def test_header_constants_equal_the_reference(golden):
    h = _header_enums()
    ref = dict(zip((str(n) for n in golden["const_names"]), (int(v) for v in golden["const_values"])))
    assert ref["NOISE_PARAMS"] == h["NR_PARAMS"]
    for k in ("NR_OFF", "NR_WDSP", "NR_ORIG", "NR_SPECTRAL", "NR_DENOISE", "NR_AUTONOTCH", "NR_DELAY", "NR_BETA", "NR_DECAY", "NR_TAPS",
              "NR_DLY", "NR_GAIN", "NR_LEAKAGE"):
        assert h[k] == ref[k], k
    from flydog_sdr_gps_amd import post
    for k in ("NR_OFF", "NR_WDSP", "NR_ORIG", "NR_SPECTRAL", "NR_DENOISE", "NR_AUTONOTCH", "NR_TAPS", "NR_DLY", "NR_GAIN", "NR_LEAKAGE",
              "NR_DELAY", "NR_BETA", "NR_DECAY", "NR_PARAMS"):
        assert getattr(post, k) == h[k], k


def test_nr_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s in NR_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
