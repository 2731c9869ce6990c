"""Generates tests/golden/lorc_ref.npz from the REFERENCE ITSELF: the Loran-C extension (extensions/Loran_C/loran_c.cpp) -- its structs
(:29-52), loran_c_data (:65-196) and init_gri (:198-208).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_iqd_golden.py: the line ranges are cut (each checked against its first and
last line) into a temporary directory (deleted on exit), tools/ref/ref_lorc_main.cpp -- stubs of ours, none of the reference's headers,
the commands of loran_c_msgs restated from the lines pinned below -- is compiled around them with g++ -O2 -ffp-contract=off; only data
is kept.

Per script of tests/lorc_common.py (the inputs are the seeded pool, rebuilt by the tests and kept here by digest): every row (the block
and sample it went out at, channel, command, length, bytes) in send order and the end state, every scalar and avg[2][1199] bit for bit.
The conditions of tests/test_lorc_cpu.py::test_golden_file_meets_its_conditions are checked here, by that very function, before the
file is kept.

    python tools/make_ref_lorc_golden.py
    python tools/make_ref_lorc_golden.py --random     tests/golden/lorc_rand_ref.npz: the seeded random scripts of tests/ext_random.py, by
                                                      digest and integers alone
"""
import os
import subprocess
import sys
import tempfile

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import lorc_common as C  # noqa: E402

F = "extensions/Loran_C/loran_c.cpp"

# file, name, first line, last line, text of the first, text of the last, a line of ours ahead of the cut (the conditional the cut's
# first lines close was opened a line above it)
CUTS = [
    (F, "LORC_CUT_STRUCTS", 29, 52, "typedef struct {", "} loran_c_t;", ""),
    (F, "LORC_CUT_DATA", 65, 196, "static void loran_c_data(int rx_chan, int instance, int nsamps, TYPECPX *samps)", "}", "#ifdef USE_IQ"),
    (F, "LORC_CUT_GRI", 198, 208, "static void init_gri(loran_c_t *e, int ch, int gri)", "}", ""),
]
PINS = [(F, 17, "#define	SCOPE_DATA	0"),
        (F, 18, "#define	SCOPE_RESET	1"),
        (F, 20, "#define	GRI_2_SEC(gri)	((double) (gri) / 1e5)"),
        (F, 22, "#define SND_RATE_HALF_THRESHOLD 12000"),
        (F, 23, "#define MAX_GRI			        9999"),
        (F, 24, "#define	MAX_BUCKET		        (int) (SND_RATE_HALF_THRESHOLD * GRI_2_SEC(MAX_GRI))"),
        (F, 58, "#define AVG_CMA		0"),
        (F, 59, "#define AVG_EMA		1"),
        (F, 60, "#define AVG_IIR		2"),
        (F, 62, "#define USE_IQ"),
        (F, 64, "#ifdef USE_IQ"),
        (F, 85, "int bn = floor(fmod(c->samp - c->offset, c->samp_per_GRI));"),
        (F, 87, "if (bn == 0 && c->dsp_samps > e->i_srate) {"),
        (F, 111, "scope = c->max? (255 * (avg / c->max)) : 0;"),
        (F, 126, "if (bn == 0 && (c->restart || (c->avg_samps > (e->i_srate * c->avg_param_i)))) {"),
        (F, 148, "c->avg[bn] = (c->avg[bn] * c->navgs) + pwr;"),
        (F, 149, "c->avg[bn] /= c->navgs + 1;"),
        (F, 168, "c->avg[bn] += (pwr - c->avg[bn]) / DECAY;"),
        (F, 186, "float iir_gain = 1.0 - expf(-(c->avg_param_f) * pwr/CUTESDR_MAX_VAL);"),
        (F, 187, "c->avg[bn] += (pwr - c->avg[bn]) * iir_gain;"),
        (F, 219, "memset(e, 0, sizeof(loran_c_t));"),
        (F, 221, "e->srate = ext_update_get_sample_rateHz(rx_chan);"),
        (F, 222, "e->i_srate = snd_rate;"),
        (F, 223, "float ms_per_bin = 1.0/e->srate * 1e3;"),
        (F, 224, "if (snd_rate > SND_RATE_HALF_THRESHOLD) ms_per_bin *= 2;"),
        (F, 234, "init_gri(e, ch, i_gri);"),
        (F, 237, "e->redraw_legend = true;"),
        (F, 238, "c->restart = true;"),
        (F, 246, "c->offset = (c->offset + offset) % c->nbucket;"),
        (F, 257, "c->gain = gain? pow(10.0, ((float) -gain) / 10.0) : 0;"),
        (F, 266, "c->avg_algo = avg_algo;"),
        (F, 275, "c->avg_param_f = avg_param;"),
        (F, 276, "c->avg_param_i = lround(avg_param);"),
        (F, 284, "e->redraw_legend = true;"),
        (F, 285, "e->ch[0].restart = e->ch[1].restart = true;"),
        (F, 287, "ext_register_receive_iq_samps(loran_c_data, rx_chan);"),
        (F, 297, "ext_unregister_receive_iq_samps(e->rx_chan);"),
        ("kiwi.h", 42, "#define	CUTESDR_SCALE	15"),
        ("kiwi.h", 43, "#define CUTESDR_MAX_VAL ((float) ((1 << CUTESDR_SCALE) - 1))"),
        ("extensions/ext.h", 68, "void ext_register_receive_iq_samps(ext_receive_iq_samps_t func, int rx_chan, int flags = PRE_AGC);"),
        ("extensions/ext.h", 99, "int ext_send_msg_data(int rx_chan, bool debug, u1_t cmd, u1_t *bytes, int nbytes);"),
        ("types.h", 9, "typedef unsigned int        u4_t;"),
        ("types.h", 10, "typedef unsigned char       u1_t;"),
        ("rx/rx_sound.cpp", 669, "receive_iq_pre_agc")]


def build(tmp):
    ref_cut.cut(tmp, CUTS, whole=True)
    ref_cut.pin(PINS, white_space_aside=True)
    exe = os.path.join(tmp, "lorc_ref")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I" + tmp, "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_lorc_main.cpp"), "-lm"], check=True)
    return exe


def random_main():
    from tests import ext_random
    with tempfile.TemporaryDirectory() as tmp:
        ext_random.write_fixture("lorc", build(tmp), C.pool(), tmp)


def report(name, got, out, k):
    allb = out[k + "rows"]
    edge = int(((allb == 0) | (allb == 255)).sum())
    print("   %-20s %3d blocks %3d rows (%d reset) %7d bytes (%5.1f%% at 0 / 255), navgs %s" % (
        name, got["nrows"].size, int(got["nrows"].sum()), int((got["cmd"] == 1).sum()), allb.size, 100.0 * edge / max(allb.size, 1),
        got["scalars"]["ch"]["navgs"].tolist()))


def main():
    ref_cut.script_golden_main(C, build, "lorc_ref.npz", ref_cut.script_by_text, report)


if __name__ == "__main__":
    random_main() if sys.argv[1:] == ["--random"] else main()
