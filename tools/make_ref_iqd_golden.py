"""Generates tests/golden/iqd_ref.npz from the REFERENCE ITSELF: the IQ display extension -- class iq_display
(extensions/IQ_display/iq_display.cpp:29-242) over class pll (rx/kiwi/pll.h).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_fftext_golden.py: the line ranges are cut (each checked against its text) into
a temporary directory (deleted on exit), tools/ref/ref_iqd_main.cpp -- stubs of ours, none of the reference's headers -- is compiled
around them with g++ -O2 -ffp-contract=off -std=gnu++11; only data is kept.

Per script of tests/iqd_common.py (the inputs are the seeded pool, rebuilt by the tests and kept here by digest): the rows of every block
(count, cmd, length; the bytes by one digest over the stream, in full for the scripts of iqd_common.FULL), which blocks sent the text
message and its four numbers, and the end state: every scalar bit for bit, _iq / _plot / _map by digest.  The conditions of
tests/test_iqd_cpu.py::test_golden_file_meets_its_conditions are checked here on the reference's output before the file is written.

    python tools/make_ref_iqd_golden.py
    python tools/make_ref_iqd_golden.py --random     tests/golden/iqd_rand_ref.npz: the seeded random scripts of tests/ext_random.py, by
                                                     digest and integers alone
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import iqd_common as C  # noqa: E402

F, P = "extensions/IQ_display/iq_display.cpp", "rx/kiwi/pll.h"

CUTS = [
    (P, "IQD_CUT_PLL", 8, 54, "class pll {", "} ;"),
    (F, "IQD_CUT_CLASS", 29, 242, "class iq_display {", "} ;"),
]
PINS = [(F, 21, "#define IQ_POINTS       0"),
        (F, 22, "#define IQ_DENSITY      1"),
        (F, 25, "#define N_IQ_RING (16*1024)"),
        (F, 26, "#define N_CH        2"),
        (F, 27, "#define N_HISTORY   2"),
        (F, 16, "#define IQ_DISPLAY_DEBUG_MSG    false"),
        (F, 38, "const float scale_factor = 255*(_gain ? _gain * (ch ? 20 : 1) / CUTESDR_MAX_VAL : 1.0f/(4.0*_ama));"),
        (F, 40, "return std::complex<u1_t>(u1_t(std::max(0.0f, std::min(255.0f, 127+sample.real()))),"),
        (F, 52, "const std::complex<float> exp_sample = (std::complex<float>)(std::pow(sample, _exponent));"),
        (F, 65, "_cma    = (float(_maN)*_cma +          sample )/float(_maN+1);"),
        (F, 67, "_maN   += (_maN < int(0.5*_fs));"),
        (F, 82, "ext_send_msg_data(_rx_chan, IQ_DISPLAY_DEBUG_MSG, cmd, (u1_t*)(&(_plot[ch][0][0])), _points*N_CH*NIQ);"),
        (F, 93, "ext_send_msg_data(_rx_chan, IQ_DISPLAY_DEBUG_MSG, cmd, (u1_t*)(&(_map[0])), _points*NIQ);"),
        (F, 99, "if (_nsamp > _maNsend) {"),
        (F, 108, 'ext_send_msg(_rx_chan, IQ_DISPLAY_DEBUG_MSG, "EXT cmaI=%e cmaQ=%e df=%e phase=%f adc_clock=%.0f",'),
        (F, 129, "set_gain(gain? std::pow(10.0, ((float) gain - 50) / 10.0) : 0);"),
        (F, 259, "iqs[rx_chan] = iq_display::make(rx_chan);"),
        (F, 267, "iqs[rx_chan]->set_sample_rate(ext_update_get_sample_rateHz(rx_chan));"),
        (F, 268, "ext_register_receive_iq_samps(iq_display_data, rx_chan);"),
        (P, 39, "_phase = std::fmod(_phase+float(2*M_PI*_fc+_df)/_fs, float(8*2*M_PI));"),
        (P, 41, "_ud  = std::arg(sample * std::exp(std::complex<float>(0.0f, -_phase)));"),
        ("kiwi.h", 33, "#define	NIQ	2"),
        ("kiwi.h", 43, "#define CUTESDR_MAX_VAL ((float) ((1 << CUTESDR_SCALE) - 1))"),
        ("types.h", 10, "typedef unsigned char       u1_t;"),
        ("rx/CuteSDR/datatypes.h", 47, "#define TYPECPX	tSComplex"),
        ("rx/rx_sound.cpp", 669, "receive_iq_pre_agc")]


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    exe = os.path.join(tmp, "iqd_ref")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=gnu++11", "-w", "-I" + tmp, "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_iqd_main.cpp"), "-lm"],
                   check=True)
    return exe


def final_df(got, lines):
    """the df of the last sent text message, in Hz"""
    return float(got["status"]["df"][-1])


def random_main():
    from tests import ext_random
    with tempfile.TemporaryDirectory() as tmp:
        ext_random.write_fixture("iqd", build(tmp), C.pool(), tmp)


def main():
    out = {}
    samples = C.pool()
    out["pool_sha"] = np.frombuffer(C.digest(samples.tobytes()), np.uint8)
    sc = C.scripts()
    out["script_names"] = np.array(sorted(sc))
    varied = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name in sorted(sc):
            got = C.run_script_exe(exe, sc[name], samples, tmp)
            k = "s_%s_" % name
            out[k + "script"] = np.array(sc[name])
            for key, v in C.golden_of(got, name in C.FULL).items():
                out[k + key] = v
            edge, total = (int(v) for v in out[k + "edge_bytes"])
            df = final_df(got, sc[name]) if got["status"].size else float("nan")
            print("   %-22s %3d blocks %5d rows %8d bytes (%4.1f%% at 0 / 255), %2d sent, df %9.4f Hz" % (
                name, got["nrows"].size, int(got["nrows"].sum()), total, 100.0 * edge / max(total, 1), int(got["sent"].sum()), df))
            assert got["nrows"].sum() >= 1 and got["sent"].sum() >= 1, (name, "every script emits a row and a sent status")
            offset = C.pll_offset(got["ints"])
            if offset is not None:
                assert abs(df - offset) < 1.0, (name, "the reference's final df is within 1 Hz of the offset", df)
            if name == "msk":
                assert (np.abs(got["status"]["df"][-C.MSK_SETTLED:] - offset) < 1.0).all(), (name, "settled", got["status"]["df"])
            varied += 2 * edge < total
    assert 2 * varied >= len(sc), ("in at least half of the scripts fewer than half of the row bytes are 0 or 255", varied, len(sc))
    path = os.path.join(C.GOLD, "iqd_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    random_main() if sys.argv[1:] == ["--random"] else main()
