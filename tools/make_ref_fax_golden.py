"""Generates tests/golden/fax_ref.npz from the REFERENCE ITSELF: the FAX extension's decoder (extensions/FAX/FaxDecoder.h, the class,
and FaxDecoder.cpp, apply_firfilter through CleanUpBuffers).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_lorc_golden.py: the line ranges are cut (each checked against its first and
last line) into a temporary directory (deleted on exit), tools/ref/ref_fax_main.cpp -- stubs of ours, none of the reference's headers,
median_i and the commands of fax.cpp restated from the lines pinned below -- is compiled around them with g++ -O2 -ffp-contract=off;
only data is kept.

Per script of tests/fax_common.py (the inputs are the seeded pool, rebuilt by the tests and kept here by digest): the lines every block
completed, every line's record, every row and the end state, every scalar and array bit for bit.  The conditions of
tests/test_fax_cpu.py::test_golden_file_meets_its_conditions are checked here, by that very function, before the file is kept.

    python tools/make_ref_fax_golden.py
    python tools/make_ref_fax_golden.py --random     tests/golden/fax_rand_ref.npz: the seeded random scripts and the shape scripts of
                                                    tests/ext_random.py, by digest and integers alone
"""
import os
import subprocess
import sys
import tempfile

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import fax_common as C  # noqa: E402

H, F, X = "extensions/FAX/FaxDecoder.h", "extensions/FAX/FaxDecoder.cpp", "extensions/FAX/fax.cpp"

# file, name, first line, last line, text of the first, text of the last
CUTS = [
    (H, "FAX_CUT_CLASS", 33, 138, "#define FAX_MSG_CLEAR   255", "};"),
    (F, "FAX_CUT_METHODS", 56, 556, "static TYPEREAL apply_firfilter(FaxDecoder::firfilter *filter, TYPEREAL sample)", "}"),
]
PINS = [(H, 34, "#define FAX_MSG_DRAW 254"),
        (H, 37, "class FaxDecoder"),
        (H, 77, "private:"),
        (F, 51, "FaxDecoder m_FaxDecoder[MAX_RX_CHANS];"),
        (F, 94, "m_SamplesPerSec_frac = ext_update_get_sample_rateHz(m_rx_chan);"),
        (F, 95, "m_SamplesPerSec_nom = snd_rate;"),
        (F, 103, "TYPEREAL k = -2 * M_PI * freq * 60.0 / m_lpm / samps_per_line;"),
        (F, 155, 'NextTaskFast("FaxPhasingLinePosition");'),
        (F, 195, "if (typecount == m_StartStopLength*m_lpm/60.0 - leewaylines) {"),
        (F, 209, 'ext_send_msg(m_rx_chan, false, "EXT fax_autostopped=0");'),
        (F, 216, 'ext_send_msg(m_rx_chan, false, "EXT fax_autostopped=1");'),
        (F, 238, "phasingSkipData = median_i(phasingPos, m_phasingLines - phasingSkipLines, &ten_pct, &ninety_pct);"),
        (F, 239, 'rcprintf(m_rx_chan, "FAX L%d SET phasingSkipData=%d 10%%=%d 90%%=%d\\n", m_imageline, phasingSkipData, ten_pct, ninety_pct);'),
        (F, 240, "if ((ninety_pct - ten_pct) > m_SamplesPerLine/6) {"),
        (F, 274, 'ext_send_msg(m_rx_chan, false, "EXT fax_phased");'),
        (F, 294, 'ext_send_msg(m_rx_chan, false, "EXT fax_sps_changed");'),
        (F, 404, "ext_send_msg_data(m_rx_chan, false, FAX_MSG_DRAW, m_debug? image : m_outImage, m_imagewidth);"),
        (F, 405, "FileWrite(m_outImage, m_imagewidth);"),
        (F, 439, 'NextTaskFast("ProcessSamples 2");'),
        (F, 458, 'm_imgdata = (u1_t*) kiwi_imalloc("InitializeImage", m_imagewidth*height*m_imagecolors);'),
        (X, 85, "m_FaxDecoder[rx_chan].ProcessSamples(&rx->real_samples_s2[e->rd_pos][0], FASTFIR_OUTBUF_SIZE, e->shift);"),
        (X, 88, "e->shift = 0;"),
        (X, 105, "memset(e, 0, sizeof(*e));"),
        (X, 144, "true // bool reset"),
        (X, 162, "e->shift = shift;"),
        ("support/misc.cpp", 92, "qsort(i, len, sizeof *i, qsort_intcomp);"),
        ("support/misc.cpp", 93, "if (pct_1) *pct_1 = i[(int) (len * ((float) *pct_1 / 100.0))];"),
        ("support/misc.cpp", 94, "if (pct_2) *pct_2 = i[(int) (len * ((float) *pct_2 / 100.0))];"),
        ("support/misc.cpp", 95, "return i[len/2];"),
        ("support/misc.cpp", 79, "return i1 - i2;"),
        ("rx/CuteSDR/datatypes.h", 46, "#define TYPEREAL f32_t"),
        ("rx/CuteSDR/datatypes.h", 73, "#define MSIN(x) sinf(x)"),
        ("rx/CuteSDR/datatypes.h", 74, "#define MCOS(x) cosf(x)"),
        ("rx/CuteSDR/datatypes.h", 80, "#define MSQRT(x) sqrtf(x)"),
        ("rx/CuteSDR/datatypes.h", 103, "#define K_2PI (2.0 * 3.14159265358979323846)"),
        ("rx/rx_sound.cpp", 701, "out_samps_s2 = &rx->real_samples_s2[rx->real_wr_pos][0];"),
        ("rx/rx_sound.cpp", 1103, "rx->real_wr_pos = (rx->real_wr_pos+1) & (N_DPBUF-1);")]


def build(tmp):
    ref_cut.cut(tmp, CUTS, whole=True)
    ref_cut.pin(PINS, white_space_aside=True)
    exe = os.path.join(tmp, "fax_ref")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I" + tmp, "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_fax_main.cpp"), "-lm"], check=True)
    return exe


def report(name, got, out, k):
    r = got["recs"]
    print("   %-20s %4d blocks %3d lines (%d start %d stop) %3d rows, flags %s, skip %d, medians %s" % (
        name, got["nlines"].size, r.size, int((r["type"] == 1).sum()), int((r["type"] == 2).sum()), len(got["rows"]),
        sorted(set(int(f) for f in r["flags"])), int(got["info"]["skip"]),
        [(int(x["phasingSkipData"]), int(x["ten_pct"]), int(x["ninety_pct"])) for x in r if x["flags"] & C.F_MEDIAN]))


def main():
    ref_cut.script_golden_main(C, build, "fax_ref.npz", ref_cut.script_by_digest, report)


def random_main():
    from tests import ext_random
    with tempfile.TemporaryDirectory() as tmp:
        ext_random.write_fixture("fax", build(tmp), C.pool(), tmp)


if __name__ == "__main__":
    random_main() if sys.argv[1:] == ["--random"] else main()
