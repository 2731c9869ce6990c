"""Generates tests/golden/wspr_ref.npz from the REFERENCE ITSELF: stage 1 of the WSPR extension (extensions/wspr/wspr_main.cpp,
wspr.cpp, wspr_util.cpp, wspr.h).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_cw_golden.py: the line ranges are cut (each checked against its first and
last line) into a temporary directory (deleted on exit), tools/ref/ref_wspr_main.cpp -- stubs of ours, none of the reference's headers
-- is compiled around them with g++ -O2 -ffp-contract=off; only data is kept.  FFTW is not on this machine: the transform is
wspr_dft512 of tools/ref/wspr_harness.h, the 512-point DFT in double rounded to float; a SECOND build with -DWSPR_DFT_FP32, an
independent radix-2 transform in float, measures what two correct transforms differ by in the row bytes (rows32_diff, rows32_max).

Per script of tests/wspr_common.py (the inputs are rebuilt from seeds by the tests and kept here by digest): the status changes,
every row with its group, half and sync flag, the savg of a few rows, pwr_sampavg, every cycle end (peaks, candidates), the end state,
and digests of pwr_samp and of i_data / q_data.  The host model (tools/wspr_host_driver.cpp) is run on every script too: it must equal
the reference record by record, and it supplies each candidate's margin over its runner-up.

The conditions the tests rely on are CHECKED HERE and recorded (cond): no two kept peaks tie in snr0, nor at the MAX_NPK cut; every
10*log10 of a kept peak is at least 4 double ulps from a float rounding tie; every winning sync1 is strictly above its runner-up, by
1e-3 of its value in the end-to-end scenes; the two builds differ in under 2 % of the row bytes of every pushed scene.  A seed that
breaks one is replaced, not excused.

    python tools/make_ref_wspr_golden.py
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import wspr_common as W  # noqa: E402

M, D, U, H = "extensions/wspr/wspr_main.cpp", "extensions/wspr/wspr.cpp", "extensions/wspr/wspr_util.cpp", "extensions/wspr/wspr.h"

# file, name, first line, last line, text of the first, text of the last
CUTS = [
    (H, "WSPR_CUT_H", 110, 332, "#define WSPR_CHECKING", "} wspr_shmem_t;"),
    (M, "WSPR_CUT_STATUS", 94, 114, 'const char *status_str[] = { "none", "idle", "sync", "running", "decoding" };', "}"),
    (M, "WSPR_CUT_FFT", 140, 240, "int grp = w->FFTtask_group;", "}"),
    (M, "WSPR_CUT_DATA", 592, 788, "static double frate, fdecimate;", "}"),
    (M, "WSPR_CUT_RESET", 790, 800, "void wspr_reset(wspr_t *w)", "}"),
    (M, "WSPR_CUT_CONST", 1154, 1156, "nffts = FPG * floor(GROUPS-1) -1;", "hbins_205 = (nbins_411-1)/2;"),
    (M, "WSPR_CUT_WINDOW", 1186, 1188, "for (i=0; i < NFFT; i++) {", "}"),
    (D, "WSPR_CUT_PR3", 31, 40, "static const unsigned char pr3[NSYM_162]=", "0,0};"),
    (D, "WSPR_CUT_RENORM", 214, 253, "void renormalize(wspr_t *w, float psavg[], float smspec[], float tmpsort[])", "}"),
    (D, "WSPR_CUT_PASS0", 555, 714, "if (ipass == 0) {", "}"),
    (U, "WSPR_CUT_COMP", 394, 406, "int snr_comp(const void *elem1, const void *elem2)", "}"),
]
PINS = [(M, 49, "#define	NONE		0"), (M, 53, "#define	DECODING	4"),
        (M, 67, "int nffts, nbins_411, hbins_205;"), (M, 70, "static float window[NFFT];"),
        (M, 175, "w->fftin[j][0] = id[k] * window[j];"), (M, 182, "WSPR_FFTW_EXECUTE(w->fftplan);"), (M, 192, "k = j+SPS;"),
        (M, 197, "float pwr = ii*ii + qq*qq;"), (M, 204, "wb->pwr_samp[w->fft_ping_pong][j][i] = pwr;"),
        (M, 216, "wb->smspec[WSPR_RENORM_FFT][j] = dB = 10*log10(wb->smspec[WSPR_RENORM_FFT][j]) - w->snr_scaling_factor;"),
        (M, 234, "wb->ws[j+1] = (u1_t) y;"), (M, 236, "wb->ws[0] = ((grp == 0) && w->tsync)? 1:0;"),
        (M, 275, "if (last < nffts) continue;"), (M, 277, "w->decode_ping_pong = w->fft_ping_pong;"),
        (M, 281, "TaskWakeupFP(w->WSPR_DecodeTask_id, TWF_CHECK_WAKING, TO_VOID_PARAM(w->rx_chan));"),
        (M, 468, "w->abort_decode = false;"), (M, 472, "wspr_status(w, DECODING, NONE);"), (M, 568, "wspr_status(w, w->status_resume, NONE);"),
        (M, 638, "if (!(min&1) && (sec == 0)) {"), (M, 675, "#define FRACTIONAL_DECIMATION 0"), (M, 760, "if (w->decim++ < (int_decimate-1))"),
        (M, 764, "if (w->didx >= TPOINTS)"), (M, 767, "if (w->group == 3) w->tsync = FALSE;"),
        (M, 836, "wspr_status(w, IDLE, IDLE);"), (M, 880, 'n = sscanf(msg, "SET capture=%d", &w->capture);'), (M, 890, "w->reset = TRUE;"),
        (M, 894, "wspr_status(w, SYNC, RUNNING);"), (M, 896, "w->abort_decode = true;"), (M, 897, "wspr_close(w->rx_chan);"), (M, 822, "wspr_reset(w);"),
        (M, 1163, "memset(w, 0, sizeof(wspr_t));"), (M, 1170, "w->wspr_type = WSPR_TYPE_2MIN;"), (M, 1176, "wspr_reset(w);"),
        (M, 1187, "window[i] = sin(i * K_PI/(NFFT-1));"), (M, 1193, "int_decimate = snd_rate / FSRATE;"),
        (D, 246, "w->min_snr = pow(10.0,-7.0/10.0);"), (D, 247, "w->snr_scaling_factor = (w->wspr_type == WSPR_TYPE_2MIN)? 26.3 : 35.3;"),
        (D, 490, "float DF2 = FSRATE/FSPS/2;"), (D, 511, "int maxdrift=4;"), (D, 529, "#define MORE_EFFORT"),
        (D, 447, "#define send_peaks_all(w, npk) w->npk = npk; if (!w->autorun) wspr_send_peaks(w, 0, npk);"),
        (D, 665, "if0 = p->freq0/DF2+SPS;"), (D, 678, "ifd=ifr+((float)k-FHSYM_81)/FHSYM_81*( (float)idrift )/(2.0*DF2);"),
        (D, 700, "if( sync1 > smax ) {"), (D, 702, "p->shift0=HSPS*(k0+1);"),
        ("rx/CuteSDR/datatypes.h", 104, "#define K_PI (3.14159265358979323846)")]


def build(tmp, fp32=False):
    ref_cut.cut(tmp, CUTS, whole=True)
    ref_cut.pin(PINS, white_space_aside=True)
    pr3 = "".join(c for c in open(os.path.join(tmp, "WSPR_CUT_PR3.inc")).read().split("=")[1] if c in "01")
    assert pr3 == "".join(str(int(v)) for v in W.PR3), "tests/wspr_common.py PR3"
    exe = os.path.join(tmp, "wspr_ref32" if fp32 else "wspr_ref")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I" + tmp, "-I" + os.path.join(ROOT, "tools", "ref")] + (["-DWSPR_DFT_FP32"] if fp32 else []) +
                   ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_wspr_main.cpp"), "-lm"], check=True)
    return exe


def same(a, b, name):
    for f in ("ev", "rows", "meta", "info"):
        assert np.array_equal(a[f], b[f]), (name, f)
    assert np.array_equal(a["cyc"][:, :111], b["cyc"][:, :111]), (name, "cycle ends")
    for f in ("pwr_sampavg", "pwr_samp", "iq"):
        assert a[f].tobytes() == b[f].tobytes(), (name, f)
    assert sorted(a["savg"]) == sorted(b["savg"]) and all(a["savg"][r].tobytes() == b["savg"][r].tobytes() for r in a["savg"]), (name, "savg")


def main():
    out = {}
    samples = W.pool()
    out["pool_sha"] = np.frombuffer(W.digest(samples.tobytes()), np.uint8)
    sc = W.scripts()
    out["script_names"] = np.array(sorted(sc))
    with tempfile.TemporaryDirectory() as tmp:
        exe, exe32, twin = build(tmp), build(tmp, fp32=True), W.build_driver(tmp)
        for name in sorted(sc):
            got = W.run_script_exe(exe, sc[name], samples, tmp)
            mine = W.run_script_exe(twin, sc[name], samples, tmp)
            same(got, mine, name)                                       # the host model IS the reference, record by record
            got["cyc"][:, 113:] = mine["cyc"][:, 113:]                  # cond[2], cond[3]: the twin's margins
            k = "s_%s_" % name
            out[k + "script_sha"] = np.frombuffer(W.digest("\n".join(sc[name]).encode()), np.uint8)
            for key, v in W.golden_of(got).items():
                out[k + key] = v
            line = "   %-14s %4d rows %d cycle ends" % (name, got["rows"].shape[0], got["cyc"].shape[0])
            for c in got["cyc"]:
                cond = c[111:]
                margin = float(cond[3:4].view(np.float32)[0])
                assert cond[0] == 1, (name, "two kept peaks tie in snr0")
                assert cond[1] == 1, (name, "a 10*log10 within 4 double ulps of a float tie")
                assert cond[2] == 1, (name, "a winner not above its runner-up")
                assert name not in W.E2E or margin >= 1e-3, (name, "margin", margin)
                line += "  npk %d margin %.2e" % (c[2], margin)
            if not name.startswith("load_"):
                got32 = W.run_script_exe(exe32, sc[name], samples, tmp)
                assert np.array_equal(got32["meta"], got["meta"]) and np.array_equal(got32["ev"], got["ev"])
                d = np.abs(got32["rows"].astype(np.int32) - got["rows"].astype(np.int32))
                out[k + "rows32_diff"] = (d != 0).sum(axis=1).astype(np.int32)
                out[k + "rows32_max"] = d.max(axis=1).astype(np.int32) if d.size else np.zeros(0, np.int32)
                frac = float((d != 0).mean()) if d.size else 0.0
                assert frac < 0.02, (name, "the two builds differ in %.2f %% of the row bytes" % (100 * frac))
                line += "  fp32 build: %d of %d bytes differ, at most by %d" % ((d != 0).sum(), d.size, d.max() if d.size else 0)
            print(line)
        path = os.path.join(tmp, "wspr_ref.npz")
        np.savez_compressed(path, **out)
        test = __import__("tests.test_wspr_cpu", fromlist=["golden_conditions"])
        test.golden_conditions(np.load(path), os.path.getsize(path))
        final = os.path.join(W.GOLD, "wspr_ref.npz")
        shutil.copyfile(path, final)
    print("wrote %s, %d bytes" % (final, os.path.getsize(final)))


if __name__ == "__main__":
    main()
