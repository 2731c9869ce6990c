"""Generates tests/golden/spec_ref.npz from the REFERENCE ITSELF: the audio spectrum display of c2s_sound() -- specAF_FFT
(rx/rx_sound.cpp:175-220), its call from inside CFastFIR::ProcessData (rx/CuteSDR/fastfir.cpp), `SET spc_=`
(rx/rx_sound_cmd.cpp:333-337), the mode command's reset (:227-228) and the channel-null call site (rx/rx_sound.cpp:802-804).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_nbw_golden.py: the line ranges are cut (each checked against its text) into
a temporary directory (deleted on exit), tools/ref/ref_spec_main.cpp is compiled around them with -O2 -ffp-contract=off; only data is
kept.  No FFT runs: the two CFastFIR objects are built from the cut statements with their transforms left out.  Needs
oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both).

Three pins (tests/spec_common.py holds the inputs):
  1. rows      every spectrum of the seeded pool through specAF_FFT with isChanNull false and true: the rows in full, the pool's digest
  2. limiter   the same function under scripted clocks: fired / specAF_last_ms per call
  3. emission  scripts of commands and 512-sample blocks: per block the rows handed over (instance, isChanNull, which fill, digest)

    python tools/make_ref_spec_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT  # ref_cut puts the repository root on sys.path
from tests import spec_common as C  # noqa: E402


CUTS = [
    ("rx/rx_sound.cpp", "SPEC_CUT_ROW", 175, 220, "bool specAF_FFT(int rx_chan, int instance, int flags, int ratio, int ns_out, TYPECPX *samps)", "}"),
    ("rx/rx_sound.cpp", "SPEC_CUT_SAM", 802, 804, "s->isChanNull = wdsp_SAM_demod(rx_chan, s->mode, s->SAM_mparam, ns_out, agc_samps_c, out_samps_s2);",
     "if (s->isChanNull) m_chan_null_FIR[rx_chan].ProcessData(rx_chan, ns_out, agc_samps_c, NULL);"),
    ("rx/rx_sound_cmd.cpp", "SPEC_CUT_CLEAR", 227, 228, "s->isChanNull = false;", "s->specAF_instance = SND_INSTANCE_FFT_PASSBAND;"),
    ("rx/rx_sound_cmd.cpp", "SPEC_CUT_CMD", 333, 337, 'if (sscanf(cmd, "SET spc_=%d", &n) == 1) {', "did_cmd = true;"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_POS0", 64, 64, "m_InBufInPos = (CONV_FIR_SIZE - 1);", "m_InBufInPos = (CONV_FIR_SIZE - 1);"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_SETUP", 175, 175, "m_instance = instance;", "m_instance = instance;"),
    ("rx/rx_sound_cmd.cpp", "SPEC_CUT_DESIGN", 274, 275, "m_PassbandFIR[rx_chan].SetupParameters(SND_INSTANCE_FFT_PASSBAND, s->locut, s->hicut, CW_OFFSET, frate);",
     "m_chan_null_FIR[rx_chan].SetupParameters(SND_INSTANCE_FFT_CHAN_NULL, s->locut, s->hicut, CW_OFFSET, frate);"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_INST", 247, 247, "int receive_FFT_instance = m_instance;", "int receive_FFT_instance = m_instance;"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_POST", 251, 253, "snd_t *snd = &snd_inst[rx_chan];",
     "bool specAF_FFT_post = (specAF_FFT != NULL && snd->specAF_instance == m_instance);"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_LOOP", 255, 272, "int i = 0;", "if (m_InBufInPos >= CONV_FFT_SIZE) {"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_CALL", 301, 302, "if (specAF_FFT_post)",
     "specAF_FFT(rx_chan, receive_FFT_instance, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, m_pFFTBuf);"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_OUT", 306, 311, "if (OutBuf != NULL) {", "}"),
    ("rx/CuteSDR/fastfir.cpp", "SPEC_CUT_TAIL", 319, 323, "m_InBufInPos = CONV_FIR_SIZE - 1;", "return outpos;"),
]
PINS = [("rx/rx_sound.cpp", 198, "pwr[i] = samps[i].re * samps[i].re;"),
        ("rx/rx_sound.cpp", 201, "float scale = 10.0f * 2.0f / (CUTESDR_MAX_VAL * CUTESDR_MAX_VAL * FFT_WIDTH * FFT_WIDTH);"),
        ("rx/rx_sound.cpp", 202, "scale *= s->isChanNull? 0.0004f : 1e6f;"),
        ("rx/rx_sound.cpp", 209, "float dB = 10.0 * log10f(pwr[i] * scale + (float) 1e-30);"),
        ("rx/rx_sound.cpp", 215, "fft[i+unwrap] = (u1_t) (int) dB;"),
        ("rx/rx_sound.cpp", 236, "memset(s, 0, sizeof(snd_t));"),
        ("rx/rx_sound.cpp", 803, "s->specAF_instance = s->isChanNull? SND_INSTANCE_FFT_CHAN_NULL : SND_INSTANCE_FFT_PASSBAND;"),
        ("rx/rx_sound_cmd.cpp", 202, "if (s->mode != _mode || n == 5) {"),
        ("rx/rx_sound_cmd.cpp", 214, "s->isSAM = mode_flags[_mode] & IS_SAM;"),
        ("rx/rx_sound_cmd.cpp", 215, "if (s->isSAM && n == 5) {"),
        ("rx/rx_sound_cmd.cpp", 216, "s->SAM_mparam = s->mparam & MODE_FLAGS_SAM;"),
        ("rx/rx_sound_cmd.cpp", 230, "s->mode = _mode;"),
        ("rx/rx_sound_cmd.cpp", 273, "#define CW_OFFSET 0"),
        ("rx/rx_sound_cmd.cpp", 336, "s->specAF_FFT = (n == SPEC_SND_AF)? specAF_FFT : NULL;"),
        ("rx/wdsp/SAM_demod.cpp", 176, "bool isChanNull = (mode == MODE_SAM && chan_null_which != CHAN_NULL_NONE);"),
        ("rx/wdsp/SAM_demod.cpp", 355, "return isChanNull;"),
        ("rx/CuteSDR/fastfir.cpp", 304, "MFFTW_EXECUTE(m_FFT_RevPlan);"),
        ("rx/mode.h", 69, "MODE_AM, MODE_AMN, MODE_USB, MODE_LSB, MODE_CW, MODE_CWN, MODE_NBFM, MODE_IQ, MODE_DRM,"),
        ("rx/mode.h", 70, "MODE_USN, MODE_LSN, MODE_SAM, MODE_SAU, MODE_SAL, MODE_SAS, MODE_QAM, MODE_NNFM"),
        ("rx/rx_sound.h", 34, "#define SND_INSTANCE_FFT_PASSBAND   0"),
        ("rx/rx_sound.h", 35, "#define SND_INSTANCE_FFT_CHAN_NULL  1"),
        ("rx/rx_sound.h", 81, "#define SPEC_SND_AF     2"),
        ("rx/rx_sound.h", 82, "#define N_SND_SPEC      3"),
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
    exe = os.path.join(tmp, "spec_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"] + ["-I" + d for d in inc]
           + ["-I" + gen, "-I" + tmp, "-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_spec_main.cpp"), "-lm",
              "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


def main():
    out = {}
    names, spec = C.pool()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        P = lambda f: os.path.join(tmp, f)
        # 1. rows
        spec.tofile(P("in.bin"))
        subprocess.run([exe, "rows", P("in.bin"), P("out.bin")], check=True)
        rows = np.fromfile(P("out.bin"), np.uint8).reshape(len(names), 2, C.W)
        out["pool_names"] = np.array(names)
        out["pool_sha"] = np.frombuffer(C.digest(spec.tobytes()), np.uint8)
        out["rows"] = rows
        print("spec_ref.npz: %d spectra x 2 instances, bytes %d .. %d" % (len(names), rows.min(), rows.max()))
        for i, n in enumerate(names):
            print("   %-24s passband %3d .. %3d   channel null %3d .. %3d" % (n, rows[i, 0].min(), rows[i, 0].max(), rows[i, 1].min(), rows[i, 1].max()))
        # 2. limiter
        lim = C.limiter_scripts()
        out["limiter_names"] = np.array(sorted(lim))
        for k in sorted(lim):
            np.array(lim[k], np.uint32).tofile(P("clk.bin"))
            subprocess.run([exe, "limiter", P("clk.bin"), P("out.bin")], check=True)
            a = np.fromfile(P("out.bin"), np.uint32).reshape(-1, 2)
            out["limiter_%s_clock" % k] = np.array(lim[k], np.uint32)
            out["limiter_%s_fired" % k] = a[:, 0].astype(np.int32)
            out["limiter_%s_last" % k] = a[:, 1].copy()
            print("   limiter %-16s %3d calls, %3d fired" % (k, len(lim[k]), int(a[:, 0].sum())))
        # 3. emission
        em = C.emit_scripts()
        nblk = 2 * max(sum(1 for l in s if l == "B") for s in em.values())
        blocks = C.emit_blocks(nblk)
        blocks.tofile(P("blk.bin"))
        out["emit_names"] = np.array(sorted(em))
        out["emit_blocks_sha"] = np.frombuffer(C.digest(blocks.tobytes()), np.uint8)
        out["emit_nblocks"] = np.int32(nblk)
        for k in sorted(em):
            open(P("s.txt"), "w").write("\n".join(em[k]) + "\n")
            subprocess.run([exe, "emit", P("s.txt"), P("blk.bin"), P("out.bin")], check=True)
            per = C.parse_emit(open(P("out.bin"), "rb").read())
            assert len(per) == sum(1 for l in em[k] if l == "B"), k
            flat = [r for b in per for r in b]
            out["emit_%s_script" % k] = np.array(em[k])
            out["emit_%s_count" % k] = np.array([len(b) for b in per], np.int32)
            out["emit_%s_info" % k] = np.array([r[:3] for r in flat], np.int32).reshape(-1, 3)
            out["emit_%s_sha" % k] = np.array([np.frombuffer(C.digest(r[3].tobytes()), np.uint8) for r in flat], np.uint8).reshape(-1, 16)
            print("   emit %-22s %s" % (k, " ".join("".join("PN"[r[0]] for r in b) or "-" for b in per)))
    path = os.path.join(C.GOLD, "spec_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= 300000


if __name__ == "__main__":
    main()
