"""Generates tests/golden/fftext_ref.npz from the REFERENCE ITSELF: the FFT extension, extensions/FFT/FFT.cpp -- fft_data (:69-191) and
fft_msgs (:193-261) with the declarations they need (:17-67).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_spec_golden.py: the line ranges are cut (each checked against its text) into
a temporary directory (deleted on exit), tools/ref/ref_fftext_main.cpp is compiled around them with -O2 -ffp-contract=off; only data is
kept.  No FFT runs.  Needs oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both).

Two pins (tests/fftext_common.py holds the inputs):
  1. scripts   commands and blocks of the seeded pool: per block whether a message was sent, its bin and row (in full for the scripts
               of fftext_common.FULL, by digest for all), and the final state: run, instance, bins, the latch, both scales, fi, fft_sec,
               time, ncma, the digest of all 200 x 1024 sums and the leading bins' sums in full where few are used
  2. limiter   fft_data under FUNC_SPEC and scripted clocks: sent / last_ms per call

    python tools/make_ref_fftext_golden.py
    python tools/make_ref_fftext_golden.py --random     tests/golden/fftext_rand_ref.npz: the seeded random scripts of tests/ext_random.py, by
                                                        digest and integers alone
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT  # ref_cut puts the repository root on sys.path
from tests import fftext_common as C  # noqa: E402

F = "extensions/FFT/FFT.cpp"

CUTS = [
    (F, "FFTEXT_CUT_DECLS", 17, 67, "//#define DEBUG_MSG	true", 'static const char* func_s[] = { "off", "wf", "spec", "integ" };'),
    (F, "FFTEXT_CUT_DATA", 69, 191, "bool fft_data(int rx_chan, int instance, int flags, int ratio, int nsamps, TYPECPX *samps)", "}"),
    (F, "FFTEXT_CUT_MSGS", 193, 261, "bool fft_msgs(char *msg, int rx_chan)", "}"),
]
PINS = [(F, 33, "#define INTEG_WIDTH CONV_FFT_SIZE"),
        (F, 38, "#define MAX_BINS	200"),
        (F, 66, "enum data_e { FUNC_OFF=-1, FUNC_WF=0, FUNC_SPEC=1, FUNC_INTEG=2 };"),
        (F, 72, "if (instance != e->instance) return false;"),
        (F, 79, "e->fft_sec = 1.0 / (ext_update_get_sample_rateHz(rx_chan) * ratio / INTEG_WIDTH);"),
        (F, 80, "e->bins = trunc(e->time / e->fft_sec);"),
        (F, 93, "double fr = fmod(e->fi, e->time);"),
        (F, 98, "if (bin >= MAX_BINS) return false;"),
        (F, 116, "e->pwr[bin][i] = samps[i].re * samps[i].re;"),
        (F, 128, "pwr = re*re + im*im;"),
        (F, 139, "e->pwr[bin][i] += pwr;"),
        (F, 159, "dB = 10.0 * log10f(pwr * scale + (float) 1e-30);"),
        (F, 166, "e->dsp.fft[i+unwrap] = (u1_t) (int) dB;"),
        (F, 177, "#define UPDATE_MS 100"),
        (F, 188, "ext_send_msg_data(rx_chan, DEBUG_MSG, FFT, (u1_t *) &e->dsp, sizeof(e->dsp));"),
        (F, 211, "float scale = 10.0 * 2.0 / (CUTESDR_MAX_VAL * CUTESDR_MAX_VAL * INTEG_WIDTH * INTEG_WIDTH);"),
        (F, 222, "e->instance = snd->isSAM? SND_INSTANCE_FFT_CHAN_NULL : SND_INSTANCE_FFT_PASSBAND;"),
        (F, 237, "ext_register_receive_FFT_samps(fft_data, rx_chan, POST_FILTERED);"),
        ("rx/CuteSDR/fastfir.cpp", 302, "specAF_FFT(rx_chan, receive_FFT_instance, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, m_pFFTBuf);"),
        ("rx/mode.h", 70, "MODE_USN, MODE_LSN, MODE_SAM, MODE_SAU, MODE_SAL, MODE_SAS, MODE_QAM, MODE_NNFM"),
        ("rx/rx_sound.h", 34, "#define SND_INSTANCE_FFT_PASSBAND   0"),
        ("rx/rx_sound.h", 35, "#define SND_INSTANCE_FFT_CHAN_NULL  1"),
        ("kiwi.h", 43, "#define CUTESDR_MAX_VAL ((float) ((1 << CUTESDR_SCALE) - 1))")]


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    gen, fftw = os.path.join(REF, "gen"), os.path.join(REF, "fftw3_api")
    if not os.path.isfile(os.path.join(gen, "kiwi.gen.h")) or not os.path.isdir(fftw):
        sys.exit("oracle/_ref/gen/kiwi.gen.h or oracle/_ref/fftw3_api missing: run oracle/build_ref.sh first")
    inc = [R] + [os.path.join(R, d) for d in ("gps", "rx", "rx/CuteSDR", "rx/csdr", "rx/kiwi", "rx/wdsp", "rx/Teensy", "rx/CMSIS", "support",
                                               "platform/common", "platform/beaglebone", "arch/sitara", "init", "net", "web", "dev", "ui",
                                               "extensions", "pkgs", "pkgs/mongoose", "pkgs/jsmn", "pkgs/sha256")]
    for top in ("rx", "extensions", "pkgs"):
        for d, subs, _ in os.walk(os.path.join(R, top)):
            if d.count(os.sep) - os.path.join(R, top).count(os.sep) <= 2:
                inc.append(d)
    dfn = ["-std=gnu++11", "-DKIWI", "-DKIWISDR", "-DHOST", "-DDEBIAN_VERSION=11", "-DVERSION_MAJ=1", "-DVERSION_MIN=663", "-DARCH_CPU=x86",
           "-DCPU_AM3359", "-DPLATFORM_beaglebone_black"]
    exe = os.path.join(tmp, "fftext_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"] + ["-I" + d for d in inc]
           + ["-I" + gen, "-I" + tmp, "-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_fftext_main.cpp"), "-lm",
              "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


def random_main():
    from tests import ext_random
    with tempfile.TemporaryDirectory() as tmp:
        ext_random.write_fixture("fftext", build(tmp), C.pool()[1], tmp)


def main():
    out = {}
    names, spec = C.pool()
    assert len(names) == C.NPOOL
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        out["pool_names"] = np.array(names)
        out["pool_sha"] = np.frombuffer(C.digest(spec.tobytes()), np.uint8)
        sc = C.scripts()
        out["script_names"] = np.array(sorted(sc))
        for name in sorted(sc):
            got = C.run_script_exe(exe, sc[name], spec, tmp)
            k = "s_%s_" % name
            out[k + "script"] = np.array(sc[name])
            out[k + "sent"], out[k + "bins"] = got["sent"], got["bins"]
            if name in C.FULL:
                out[k + "rows"] = got["rows"]
            out[k + "row_sha"] = C.row_digests(got["rows"])
            out[k + "state"] = np.array([got["run"], got["instance"], got["nbins"], got["reset"]], np.int32)
            out[k + "scales"] = np.array([got["fft_scale"], got["spectrum_scale"]], np.float32)
            out[k + "times"] = np.array([got["fi"], got["fft_sec"], got["time"]], np.float64)
            out[k + "ncma"] = got["ncma"]
            out[k + "pwr_sha"] = np.frombuffer(C.digest(got["pwr"].tobytes()), np.uint8)
            used = int(np.flatnonzero(got["pwr"].any(axis=1)).max(initial=-1)) + 1
            if 0 < used <= 3:
                out[k + "pwr_head"] = got["pwr"][:used]
            rows = got["rows"]
            print("   %-18s %3d blocks %3d rows, bins %s, nbins %d, ncma sum %d, bytes %s, fi %.6f" % (
                name, got["sent"].size, rows.shape[0], sorted(set(got["bins"].tolist()))[:6], got["nbins"], int(got["ncma"].sum()),
                ("%d .. %d" % (rows.min(), rows.max())) if rows.size else "-", got["fi"]))
        lim = C.limiter_scripts()
        out["limiter_names"] = np.array(sorted(lim))
        for k in sorted(lim):
            sent, last = C.run_limiter_exe(exe, lim[k], tmp)
            out["limiter_%s_clock" % k] = np.array(lim[k], np.uint32)
            out["limiter_%s_sent" % k] = sent
            out["limiter_%s_last" % k] = last
            print("   limiter %-16s %3d calls, %3d sent" % (k, len(lim[k]), int(sent.sum())))
    path = os.path.join(C.GOLD, "fftext_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= 300000


if __name__ == "__main__":
    random_main() if sys.argv[1:] == ["--random"] else main()
