"""Generates tests/golden/cw_ref.npz from the REFERENCE ITSELF: the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp,
the defines and the struct through CW_Decode).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_fax_golden.py: the line range is cut (checked against its first and last
line) into a temporary directory (deleted on exit), tools/ref/ref_cw_main.cpp -- stubs of ours, none of the reference's headers, the
commands of cw_decoder.cpp restated from the lines pinned below -- is compiled around it with g++ -O2 -ffp-contract=off; only data is
kept.

Per script of tests/cw_common.py (the inputs are the seeded pool, rebuilt by the tests and kept here by digest): the events of every
sound block and the end state, every scalar, the ring and data[] bit for bit, and the harness's count of the corrective branches.
The conditions of tests/test_cw_cpu.py::test_golden_file_meets_its_conditions are checked here, by that very function, before the
file is kept.

    python tools/make_ref_cw_golden.py [--show]
    python tools/make_ref_cw_golden.py --random     tests/golden/cw_rand_ref.npz: the seeded random scripts and the shape scripts of
                                                    tests/ext_random.py, by digest and integers alone
"""
import os
import subprocess
import sys
import tempfile

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import cw_common as C  # noqa: E402

U, X, HH = "extensions/CW_decoder/uhsdr_cw_decoder.cpp", "extensions/CW_decoder/cw_decoder.cpp", "extensions/CW_decoder/uhsdr_cw_decoder.h"

# file, name, first line, last line, text of the first, text of the last
CUTS = [
    (U, "CW_CUT_ALL", 50, 1296, "//#define SIGNAL_TAU			0.01", "}"),
]
PINS = [(U, 51, "#define SIGNAL_TAU 0.1"),
        (U, 59, "#define ONE_SECOND (snd_rate / cw->blocksize)"),
        (U, 176, "static cw_decoder_t cw_decoder[MAX_RX_CHANS];"),
        (U, 296, "static void AudioFilter_CalcGoertzel(Goertzel* g, float32_t freq, const uint32_t size, const float goertzel_coeff, float32_t samplerate)"),
        (U, 299, "g->a = (0.5 + (freq * goertzel_coeff) * size/samplerate);"),
        (U, 309, "g->b0 = g->r * g->b1 - g->b2 + in;"),
        (U, 345, "void CwDecode_Init(int rx_chan, int wpm, int training_interval)"),
        (U, 351, "memset(cw, 0, sizeof(cw_decoder_t));"),
        (U, 356, "cw->sampling_freq = ext_update_get_sample_rateHz(rx_chan);"),
        (U, 385, 'ext_send_msg(cw->rx_chan, false, "EXT cw_train=0");'),
        (U, 483, "newstate = (siglevel >= cw->threshold_linear)? true:false;"),
        (U, 519, "static int slowdown;"),
        (U, 520, "if (slowdown++ == 2) {"),
        (U, 525, 'ext_send_msg(cw->rx_chan, false, "EXT cw_plot=%.2f,%d,%.2f", dB, siglevel >= 0, threshold_log);'),
        (U, 563, "if (cw->sig_timer > ONE_SECOND * CW_TIMEOUT)"),
        (U, 606, "cw->speed = cw->speed_wpm_avg;"),
        (U, 617, "cw->raw_signal_buffer[cw->sample_counter] = (float32_t) samps[idx] / 4;"),
        (U, 672, 'ext_send_msg(cw->rx_chan, false, "EXT cw_train=%d", processed >= cw->training_interval? 0 : processed);'),
        (U, 862, "- ((uint32_t) cw->data[cw->data_len - 1].time"),
        (U, 874, "- ((uint32_t) cw->data[cw->data_len - 1].time"),
        (U, 961, 'ext_send_msg_encoded(cw->rx_chan, false, "EXT", "cw_chars", (char *) s);'),
        (U, 983, "u4_t now = timer_sec() / 4;"),
        (U, 985, 'ext_send_msg(cw->rx_chan, false, "EXT cw_wpm=%d", cw->speed);'),
        (U, 1007, "int16_t x = (cw->times.cwspace_avg + cw->times.pulse_avg) - cw->times.w_space;"),
        (U, 1149, "cw->sig_outcount = ring_idx_change(cw->last_outcount, +2,CW_SIG_BUFSIZE);"),
        (U, 1159, 'NextTask("cw-loop");'),
        (U, 1184, "cw->sig_outcount = cw->last_outcount;"),
        (U, 1277, "cw->err_timeout = timer_sec() + ERROR_TIMEOUT;"),
        (U, 1278, 'ext_send_msg(cw->rx_chan, false, "EXT cw_train=%d", -(cw->err_cnt));'),
        (U, 1292, 'ext_send_msg(cw->rx_chan, false, "EXT cw_train=0");'),
        (HH, 17, "typedef float float32_t;"),
        (HH, 20, "#define CW_DECODER_BLOCKSIZE_MAX 128"),
        (HH, 23, "#define CW_DECODER_BLOCKSIZE_DEFAULT 88"),
        (X, 101, "CwDecode_RxProcessor(rx_chan, 0, FASTFIR_OUTBUF_SIZE, &rx->real_samples_s2[e->rd_pos][0]);"),
        (X, 111, "ext_unregister_receive_real_samps_task(rx_chan);"),
        (X, 137, "CwDecode_Init(rx_chan, 0, training_interval);"),
        (X, 149, "ext_register_receive_real_samps_task(e->tid, rx_chan);"),
        (X, 164, "CwDecode_Init(rx_chan, 0, training_interval);"),
        (X, 181, "CwDecode_pboff(rx_chan, pboff);"),
        (X, 188, "CwDecode_wpm(rx_chan, wpm, training_interval);"),
        (X, 195, "CwDecode_wsc(rx_chan, wsc);"),
        (X, 202, "CwDecode_threshold(rx_chan, 0, isAutoThreshold);"),
        (X, 209, "CwDecode_threshold(rx_chan, 1, threshold_lin);"),
        ("types.h", 115, "#define CLAMP(a,min,max) ( ((a) < (min))? (min) : ( ((a) > (max))? (max) : (a) ) )"),
        ("rx/CuteSDR/datatypes.h", 104, "#define K_PI (3.14159265358979323846)")]


def build(tmp):
    ref_cut.cut(tmp, CUTS, whole=True)
    ref_cut.pin(PINS, white_space_aside=True)
    exe = os.path.join(tmp, "cw_ref")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I" + tmp, "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_cw_main.cpp"), "-lm"], check=True)
    return exe


def report(name, got, out, k):
    e = got["evs"]
    tr = e[e["kind"] == C.TRAIN]["a"]
    print("   %-20s %4d blocks %5d events, stats %s, train<0 %s, wpm %s\n        %r" % (
        name, got["nev"].size, e.size, got["stats"][:5].tolist(), tr[tr < 0].tolist(), sorted(set(e[e["kind"] == C.WPM]["a"].tolist())), C.text_of(e)))
    if "--show" in sys.argv:
        print("        train:", tr.tolist()[:80])


def main():
    ref_cut.script_golden_main(C, build, "cw_ref.npz", ref_cut.script_by_digest, report, check="--nocheck" not in sys.argv)


def random_main():
    from tests import ext_random
    with tempfile.TemporaryDirectory() as tmp:
        ext_random.write_fixture("cw", build(tmp), C.pool(), tmp)


if __name__ == "__main__":
    random_main() if sys.argv[1:] == ["--random"] else main()
