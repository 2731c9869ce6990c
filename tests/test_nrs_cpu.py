"""kg_nrs.h, the arithmetic of NR_SPECTRAL (rx/Teensy/NR_spectral.cpp and the CMSIS 512-point transform it calls) that kg_post's
kernel runs, compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/nrs_host_driver.cpp,
against every scenario of tests/golden/nrs_ref.npz (made by tools/make_ref_nrs_golden.py from the reference's own statements) --
BIT-EXACT: every output block, every end state (the arrays through their NaN-canonical digests), the NN of every phase-3 frame.
Then the tables (the library's twiddles and window equal the ones the pin ran with), the conditions the golden file must meet so
that the parity tests cannot pass vacuously, the header's constants, the Python mirror of the passband, and the C ABI."""
import math
import os
import re

import numpy as np
import pytest

from . import nrs_common as nc

ROOT = nc.ROOT
NRS_SYMBOLS = ("kg_post_nrs_select", "kg_post_nrs_setup", "kg_post_nrs_passband", "kg_post_nrs_process_dev", "kg_post_nrs_state")


@pytest.fixture(scope="module")
def golden():
    return nc.load()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return nc.build_driver(tmp_path_factory.mktemp("nrs"))


@pytest.fixture(scope="module")
def runs(golden, driver, tmp_path_factory):
    """every scenario through the host driver: name -> (output, states, trace)"""
    tmp = tmp_path_factory.mktemp("nrs_runs")
    out = {}
    for name in nc.names(golden):
        y, st, tr, rc = nc.run_driver(driver, int(golden[name + "_rate"]), nc.script(golden, name), nc.scenario_input(golden, name), tmp)
        assert rc == 0, (name, rc)
        out[name] = (y, st, tr)
    return out


def test_scenarios_bit_exact(golden, runs):
    assert len(runs) >= 20
    for name, (y, states, tr) in runs.items():
        nc.check_blocks(name, y, golden, "host driver")
        si, sf, sha = golden[name + "_state_i"], golden[name + "_state_f"], golden[name + "_state_sha"]
        assert len(states) == len(si), name
        for k, (iv, fv, arr) in enumerate(states):
            assert np.array_equal(iv, si[k]), (name, k, iv, si[k])
            assert np.array_equal(fv.view(np.uint32), sf[k].view(np.uint32)), (name, k, fv, sf[k])
            for a in range(9):
                assert nc.fdigest(arr[a]) == bytes(sha[k][a]), (name, k, nc.ARRAYS[a])
        assert np.array_equal(tr[:, :4], golden[name + "_trace"]), (name, "NN / pslp / first_time per block")


def test_tables_equal_the_pins(golden):
    """kg_tables.h's twiddles and window (tools/gen_tables.py) are the arrays the reference binary ran with"""
    text = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_tables.h")).read()

    def floats(name):
        body = text[text.index(name + " = {{"):]
        body = body[:body.index("}};")]
        return np.array([float.fromhex(h) for h in re.findall(r"-?0x[0-9a-f.]+p[-+]?\d+", body)], np.float64).astype(np.float32)
    tw, win = floats("KG_NRS_TW"), floats("KG_NRS_WIN")
    assert tw.size == 1024 and win.size == 256
    assert np.array_equal(tw.view(np.uint32), golden["twiddle"].view(np.uint32))
    assert np.array_equal(win.view(np.uint32), golden["window"].view(np.uint32))
    # and the twiddles are what the builder says they are: cos / sin in double, rounded once
    want = np.array([f(2.0 * math.pi * k / 512) for k in range(512) for f in (math.cos, math.sin)], np.float64).astype(np.float32)
    assert np.array_equal(tw.view(np.uint32), want.view(np.uint32))


def test_transform_is_a_dft(golden):
    """the stored twiddles against a double-precision DFT's: the table is right to float precision"""
    k = np.arange(512)
    tw = golden["twiddle"].astype(np.float64)
    assert np.abs(tw[0::2] - np.cos(2 * np.pi * k / 512)).max() < 6e-8
    assert np.abs(tw[1::2] - np.sin(2 * np.pi * k / 512)).max() < 6e-8


def test_golden_file_meets_its_conditions(golden, runs):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    nn, over_taken, over_not, nan_frames = set(), False, False, 0
    for name in nc.names(golden):
        tr = golden[name + "_trace"]
        degenerate = bool(golden[name + "_degenerate"])
        nn |= {int(v) for v in tr[:, :2].ravel() if v}
        p3 = tr[tr[:, 3] == 3]
        over_taken |= bool((p3[:, 2] > 0).any())
        over_not |= bool((p3[:, 2] == 0).any())
        nan_frames += int(runs[name][2][:, 4].sum())
        x, y = nc.scenario_input(golden, name), runs[name][0]
        if not degenerate:
            same = [b for b in range(x.size // nc.BLK) if np.array_equal(x[b * nc.BLK:(b + 1) * nc.BLK], y[b * nc.BLK:(b + 1) * nc.BLK])]
            assert not same, (name, "blocks the stage left unchanged", same)
        if name != "never_initialised":
            assert golden[name + "_state_i"][-1][0] == 3, (name, "phase 3 not reached")
    assert nn == {1, 3, 5, 7, 9}, nn
    assert over_taken and over_not, "pslp > psthr must be both taken and not taken"
    assert nan_frames >= 1, "no frame with a NaN power_ratio"
    assert golden["never_initialised_state_i"][-1][0] == 0 and not golden["never_initialised_out"].any()
    loud = golden["loud_wrap_out"].astype(np.int32)
    assert np.abs(np.diff(loud)).max() > 32768                          # the TYPEMONO16 conversion wrapped
    rates = {int(golden[n + "_rate"]) for n in nc.names(golden)}
    assert rates == {12000, 20250}
    size = os.path.getsize(os.path.join(nc.GOLD, "nrs_ref.npz"))
    assert size < 1 << 20


def test_passband_rule(golden, driver, tmp_path):
    """the narrowest legal passbands are in the file; one bin narrower is refused by the driver (exit 6), at the command"""
    from flydog_sdr_gps_amd import post
    assert post.nrs_vad_bins(*post.nrs_norm_passband(0, 390), 12000) == (1, 17)
    assert post.nrs_vad_bins(*post.nrs_norm_passband(5720, 5999), 12000) == (244, 256)
    assert post.nrs_passband_ok(0, 390, 12000) and not post.nrs_passband_ok(0, 370, 12000)
    assert post.nrs_passband_ok(5720, 5999, 12000) and not post.nrs_passband_ok(5750, 5999, 12000)
    assert post.nrs_passband_ok(470, 530, 12000)                        # CW: narrower than NN, legal (stale NR_G reads)
    x = np.zeros(512, np.int16)
    for lines in (["M 0 370", "A 3"], ["M 300 2700", "A 3", "M 5750 5999"], ["A 3"]):
        assert nc.run_driver(driver, 12000, lines + ["B 512 0"], x, tmp_path)[3] == 6, lines
    assert nc.run_driver(driver, 12000, ["M 0 370", "A 1", "B 512 0"], x, tmp_path)[3] == 0          # other algos: any passband
    # the Python mirror of rx_sound_cmd.cpp:252-266 against the reference's norm_locut / norm_hicut of every scenario's last passband
    for name in nc.names(golden):
        cuts = [l.split() for l in nc.script(golden, name) if l[0] in "MC"]
        if cuts and cuts[-1][0] == "M":
            lo, hi = post.nrs_norm_passband(float(cuts[-1][1]), float(cuts[-1][2]))
            assert (lo, hi) == tuple(golden[name + "_state_f"][-1][10:12]), name


def test_header_constants_equal_the_reference(golden):
    text = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    h = {k: int(v) for k, v in re.findall(r"\bKG_(NRS?_[A-Z_]+)\s*=\s*(\d+)", text)}
    ref = dict(zip((str(n) for n in golden["const_names"]), (float(v) for v in golden["const_values"])))
    assert h["NR_SPECTRAL"] == ref["NR_SPECTRAL"] and h["NR_PARAMS"] == ref["NOISE_PARAMS"]
    assert (h["NRS_GAIN"], h["NRS_ALPHA"], h["NRS_ASNR"]) == (ref["NR_S_GAIN"], ref["NR_ALPHA"], ref["NR_ASNR"])
    from flydog_sdr_gps_amd import post
    assert (post.NR_S_GAIN, post.NR_ALPHA, post.NR_ASNR, post.NRS_BLOCK) == (ref["NR_S_GAIN"], ref["NR_ALPHA"], ref["NR_ASNR"], ref["FFT_FULL"])
    assert post.NRS_ARRAYS == nc.ARRAYS
    # kg_nrs.h's literals are the reference's
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_nrs.h")).read()
    assert "FFT_FULL = %d" % ref["FFT_FULL"] in src and "NR_WIDTH = %d" % ref["NR_width"] in src
    for name, pat in (("psthr", r"psthr = ([\d.]+)"), ("pnsaf", r"pnsaf = ([\d.]+)"), ("psini", r"psini = ([\d.]+)"), ("pspri", r"pspri = ([\d.]+)"),
                      ("power_threshold", r"power_threshold = ([\d.]+)"), ("snr_prio_min_dB", r"snr_prio_min_dB = (-?[\d.]+)")):
        vals = {float(v) for v in re.findall(pat, src)}
        assert vals == {ref[name]}, (name, vals, ref[name])


def test_nrs_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s in NRS_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
    declared = set(re.findall(r"^(?:int|void|const char \*|size_t|double)\s*\*?\s*(kg_\w+)\(", header, re.M))
    assert set(NRS_SYMBOLS) <= declared
