"""Generates tests/golden/nr_ref.npz from the REFERENCE ITSELF: c2s_sound()'s noise-reduction switch (rx/rx_sound.cpp:933-949 ->
rx/wdsp/ANR.cpp, rx/kiwi/lms.cpp) driven by the two `SET nr` commands of rx/rx_sound_cmd.cpp (:464-471, :473-475, :505-523).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Like tools/make_ref_sam_golden.py, it cuts those line ranges (each checked against its text) into a temporary
directory (deleted on exit), compiles tools/ref/ref_nr_main.cpp around them with -O2 -ffp-contract=off (oracle/build_ref.sh's flags),
with rx/kiwi/lms.cpp linked and rx/wdsp/ANR.cpp included where they lie, runs it on scripted scenarios and keeps only the data: the
scripts, the int16 inputs made here from a fixed seed, the int16 outputs and the end states the reference's code produced (the
weight vectors as SHA-256 digests, NaN canonical).  Nothing of the reference's text enters the repository.  Needs oracle/_ref/gen/kiwi.gen.h
and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both; run first if absent).

    python tools/make_ref_nr_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT, read  # ref_cut puts the repository root on sys.path
from tests.script_common import digest_u8 as digest  # noqa: E402
GOLD = os.path.join(ROOT, "tests", "golden")

# (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    ("rx/rx_sound_cmd.cpp", "NR_CUT_ALGO", 464, 471, "case CMD_NR_ALGO:", "break;"),
    ("rx/rx_sound_cmd.cpp", "NR_CUT_DECLS", 473, 475, "int n_type, n_en;", "float n_pval;"),
    ("rx/rx_sound_cmd.cpp", "NR_CUT_TYPE", 505, 523, "case CMD_NR_TYPE:", ""),
    ("rx/rx_sound.cpp", "NR_CUT_STAGE", 933, 949, "// ordered so denoiser can cleanup residual noise from autonotch", "}"),
]
# the statements inside the cuts that the scenarios rely on
PINS = [("rx/rx_sound_cmd.cpp", 469, "memset(s->nr_enable, 0, sizeof(s->nr_enable));"),
        ("rx/rx_sound_cmd.cpp", 518, "case NR_WDSP: wdsp_ANR_init(rx_chan, (nr_type_e) n_type, s->nr_param[n_type]); break;"),
        ("rx/rx_sound_cmd.cpp", 519, "case NR_ORIG: m_LMS[rx_chan][n_type].Initialize((nr_type_e) n_type, s->nr_param[n_type]); break;"),
        ("rx/rx_sound_cmd.cpp", 524, "break;"),
        ("rx/rx_sound.cpp", 923, "if (!IQ_or_DRM_or_stereo) {"),
        ("rx/rx_sound.cpp", 936, "if (s->nr_enable[NR_AUTONOTCH]) wdsp_ANR_filter(rx_chan, NR_AUTONOTCH, ns_out, out_samps_s2, out_samps_s2);"),
        ("rx/rx_sound.cpp", 942, "if (s->nr_enable[NR_DENOISE]) m_LMS[rx_chan][NR_DENOISE].ProcessFilter(ns_out, out_samps_s2, out_samps_s2);")]
# the reference's enum values and parameter indices (rx/rx_noise.h:9-10, extensions/noise_filter/noise_filter.h), pinned by text
ENUMS = [("rx/rx_noise.h", "typedef enum { NR_OFF_ = 0, NR_WDSP = 1, NR_ORIG = 2, NR_SPECTRAL = 3 } nr_algo_e;"),
         ("rx/rx_noise.h", "typedef enum { NR_DENOISE = 0, NR_AUTONOTCH = 1 } nr_type_e;"),
         ("rx/rx_noise.h", "#define NOISE_PARAMS 8")]
PARAMS = ["NR_DELAY", "NR_BETA", "NR_DECAY", "NR_TAPS", "NR_DLY", "NR_GAIN", "NR_LEAKAGE"]


def consts():
    """name -> value of the reference's NR constants, read from its text"""
    out = {}
    for rel, t in ENUMS:
        assert any(t in l for l in read(rel)), ("reference enum moved", rel, t)
    out.update(NR_OFF=0, NR_WDSP=1, NR_ORIG=2, NR_SPECTRAL=3, NR_DENOISE=0, NR_AUTONOTCH=1, NOISE_PARAMS=8)
    nf = read("extensions/noise_filter/noise_filter.h")
    for p in PARAMS:
        v = [l.split() for l in nf if l.startswith("#define") and l.split()[1] == p]
        assert len(v) == 1, p
        out[p] = int(v[0][2])
    return out


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    gen, fftw = os.path.join(REF, "gen"), os.path.join(REF, "fftw3_api")
    if not os.path.isfile(os.path.join(gen, "kiwi.gen.h")) or not os.path.isdir(fftw):
        sys.exit("oracle/_ref/gen/kiwi.gen.h or oracle/_ref/fftw3_api missing: run oracle/build_ref.sh first")
    inc = [R] + [os.path.join(R, d) for d in ("gps", "rx", "rx/CuteSDR", "rx/csdr", "rx/kiwi", "rx/wdsp", "rx/Teensy", "support",
                                               "platform/common", "platform/beaglebone", "arch/sitara", "init", "net", "web", "dev", "ui",
                                               "extensions", "pkgs", "pkgs/mongoose", "pkgs/jsmn", "pkgs/sha256")]
    for top in ("rx", "extensions", "pkgs"):
        for d, subs, _ in os.walk(os.path.join(R, top)):
            if d.count(os.sep) - os.path.join(R, top).count(os.sep) <= 2:
                inc.append(d)
    dfn = ["-std=gnu++11", "-DKIWI", "-DKIWISDR", "-DHOST", "-DDEBIAN_VERSION=11", "-DVERSION_MAJ=1", "-DVERSION_MIN=663", "-DARCH_CPU=x86",
           "-DCPU_AM3359", "-DPLATFORM_beaglebone_black"]
    exe = os.path.join(tmp, "nr_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"] + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp]
           + ['-DNR_ANR_CPP="%s"' % os.path.join(R, "rx/wdsp/ANR.cpp"), "-no-pie", "-o", exe,
              os.path.join(ROOT, "tools", "ref", "ref_nr_main.cpp"), os.path.join(R, "rx/kiwi/lms.cpp")]
           + ["-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


rng = np.random.Generator(np.random.PCG64(0x4E520001))
RATE = 12000.0


def tones_noise(n, t0, tones, noise, amp=1.0):
    t = (np.arange(n) + t0) / RATE
    x = sum(a * np.sin(2 * np.pi * f * t + ph) for f, a, ph in tones) + noise * rng.standard_normal(n)
    return x * amp


def speech(n, t0, noise):
    """speech-like: syllable-gated harmonic tones with a moving pitch, plus noise"""
    t = (np.arange(n) + t0) / RATE
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    gate = 0.5 * (1 + np.sin(2 * np.pi * 3.1 * t)) ** 2
    v = gate * (3000 * np.sin(ph) + 1800 * np.sin(3 * ph + 0.4) + 900 * np.sin(5 * ph + 1.1))
    return v + noise * rng.standard_normal(n)


def i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


WDSP, ORIG = 1, 2
DN, AN = 0, 1


def wdsp_params(t, taps, dly, gain, leak):
    # the client's order: one parameter at a time (rx_sound_cmd.cpp:511-521 inits type t after every one)
    return ["P %d 0 %.9g" % (t, taps), "P %d 1 %.9g" % (t, dly), "P %d 2 %.9g" % (t, gain), "P %d 3 %.9g" % (t, leak)]


def orig_params(t, dlen, beta, decay):
    return ["P %d 0 %.9g" % (t, dlen), "P %d 1 %.9g" % (t, beta), "P %d 2 %.9g" % (t, decay)]


def blocks(k, n=512, stereo=0):
    return ["B %d %d" % (n, stereo)] * k


# name, script lines, signal (a function of n, t0)
sc = [
    ("wdsp_an_tone", ["A 1"] + wdsp_params(AN, 64, 16, 1e-4, 0.1) + ["E 1 1"] + blocks(8) + ["S"],
     lambda n, t0: tones_noise(n, t0, [(1000.0, 6000, 0.3)], 900)),
    ("wdsp_dn_speech", ["A 1"] + wdsp_params(DN, 64, 16, 1e-4, 0.1) + ["E 0 1"] + blocks(8) + ["S"], lambda n, t0: speech(n, t0, 1500)),
    ("wdsp_both_128", ["A 1"] + wdsp_params(AN, 128, 128, 2.048e-4, 0.2) + wdsp_params(DN, 128, 2, 1.28e-5, 8.0) + ["E 0 1", "E 1 1"]
     + blocks(6) + ["S"], lambda n, t0: speech(n, t0, 900) + tones_noise(n, t0, [(1375.0, 4000, 0.0)], 0)),
    ("wdsp_taps16_dly1", ["A 1"] + wdsp_params(AN, 16, 1, 8.192e-2, 1e-3) + wdsp_params(DN, 16, 1, 8.192e-2, 1e-3) + ["E 1 1", "E 0 1"]
     + blocks(4) + ["S"], lambda n, t0: tones_noise(n, t0, [(700.0, 5000, 0.0), (2100.0, 3000, 1.0)], 1200)),
    ("wdsp_loud_wrap", ["A 1"] + wdsp_params(DN, 64, 16, 1e-3, 1e-3) + ["E 0 1"] + blocks(4) + ["S"],
     lambda n, t0: tones_noise(n, t0, [(450.0, 30000, 0.0)], 2000)),
    ("wdsp_lidx_walk", ["A 1"] + wdsp_params(AN, 64, 2, 4.096e-2, 8192.0) + wdsp_params(DN, 64, 2, 1e-7, 1e-3) + ["E 1 1", "E 0 1"]
     + blocks(6) + ["S"], lambda n, t0: tones_noise(n, t0, [(300.0, 2000, 0.0)], 6000)),
    ("wdsp_midstream_params", ["A 1"] + wdsp_params(AN, 64, 16, 1e-4, 0.1) + ["E 1 1"] + blocks(2) + ["P 1 0 128"] + blocks(1) + ["P 1 1 64"]
     + blocks(1) + ["P 1 2 0.00128"] + blocks(1) + ["P 1 3 0.4"] + blocks(2) + ["S"],
     lambda n, t0: tones_noise(n, t0, [(1000.0, 6000, 0.3), (1800.0, 2000, 0.0)], 900)),
    ("wdsp_never_init_and_odd", ["A 1", "E 0 1", "E 1 1", "B 301 0", "B 7 0"] + wdsp_params(AN, 32, 3, 1e-4, 0.1)
     + ["B 511 0", "B 1 0", "B 1024 0", "S"], lambda n, t0: speech(n, t0, 2000)),
    ("orig_an_tone", ["A 2"] + orig_params(AN, 0, 0, 0) + ["E 1 1"] + blocks(8) + ["S"],
     lambda n, t0: tones_noise(n, t0, [(1000.0, 6000, 0.3)], 900)),
    ("orig_dn_speech", ["A 2"] + orig_params(DN, 0, 0, 0) + ["E 0 1"] + blocks(8) + ["S"], lambda n, t0: speech(n, t0, 1500)),
    ("orig_both_dlen", ["A 2"] + orig_params(AN, 300, 0.1, 0.999) + orig_params(DN, 1, 0.01, 0.97) + ["E 1 1", "E 0 1"] + blocks(4)
     + ["P 1 0 1000", "P 0 0 0.5"] + blocks(3) + ["S"], lambda n, t0: speech(n, t0, 900) + tones_noise(n, t0, [(1500.0, 3000, 0.0)], 0)),
    ("orig_loud_wrap", ["A 2"] + orig_params(DN, 0, 0.05, 0.999) + ["E 0 1"] + blocks(4) + ["S"],
     lambda n, t0: tones_noise(n, t0, [(450.0, 32000, 0.0)], 500)),
    ("orig_never_init_and_odd", ["A 2", "E 1 1", "E 0 1", "B 333 0", "B 5 0"] + orig_params(DN, 17, 0, 0) + ["B 1023 0", "B 2 0", "S"],
     lambda n, t0: speech(n, t0, 2000)),
    ("algo_switch_keeps_state", ["A 1"] + wdsp_params(AN, 64, 16, 1e-4, 0.1) + ["E 1 1"] + blocks(2) + ["A 2"] + orig_params(AN, 0, 0, 0)
     + ["E 1 1"] + blocks(2) + ["A 1", "B 512 0", "E 1 1"] + blocks(2) + ["A 0", "E 1 1", "E 0 1", "B 512 0", "C", "A 1", "E 1 1"]
     + blocks(2) + ["S"], lambda n, t0: tones_noise(n, t0, [(1000.0, 6000, 0.3)], 900)),
    ("stereo_skips", ["A 1"] + wdsp_params(AN, 64, 16, 1e-4, 0.1) + wdsp_params(DN, 64, 16, 1e-4, 0.1) + ["E 1 1", "E 0 1"]
     + ["B 512 0", "B 512 1", "B 512 0", "A 2", "E 1 1"] + orig_params(AN, 0, 0, 0) + ["B 512 1", "B 512 0", "S"],
     lambda n, t0: speech(n, t0, 1000)),
    ("enable_values", ["A 1"] + wdsp_params(DN, 64, 16, 1e-4, 0.1) + ["E 0 7", "B 512 0", "E 0 -1", "B 512 0", "E 0 0", "B 512 0", "S"],
     lambda n, t0: speech(n, t0, 1000)),
]


def fdigest(b):
    """digest of a float32 vector with every NaN as 0x7FC00000: a diverged filter's NaN weights are NaN on either machine, but x86's
    default NaN is the negative quiet one and the GPU's the positive one"""
    u = np.frombuffer(b, np.uint32).copy()
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return digest(u.tobytes())


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, script, sig in sc:
            n = sum(int(l.split()[1]) for l in script if l[0] == "B")
            x = i16(sig(n, 0))
            x.tofile(os.path.join(tmp, "in.bin"))
            open(os.path.join(tmp, "s.txt"), "w").write("\n".join(script) + "\n")
            subprocess.run([exe, os.path.join(tmp, "s.txt"), os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
            raw = open(os.path.join(tmp, "out.bin"), "rb").read()
            y = np.frombuffer(raw[:2 * n], np.int16)
            st = raw[2 * n:]
            rec = 6 * 4 + 2 * 4 + 512 * 4 + 121 * 4
            assert len(st) == 2 * rec * script.count("S")
            ints, flts, wsha, csha = [], [], [], []
            for t in range(2):
                r = st[t * rec:(t + 1) * rec]
                ints.append(np.frombuffer(r[:24], np.int32)); flts.append(np.frombuffer(r[24:32], np.float32))
                wsha.append(fdigest(r[32:32 + 2048])); csha.append(fdigest(r[32 + 2048:]))
            out[name + "_script"] = np.array(script)
            out[name + "_in"] = x
            out[name + "_out"] = y.copy()
            out[name + "_state_i"] = np.array(ints, np.int32)           # per type: in_idx, taps, delay, dlp, dlen, nr_type
            out[name + "_state_f"] = np.array(flts, np.float32)         # per type: lidx, ngamma
            out[name + "_w_sha"] = np.array(wsha, np.uint8)             # per type: SHA-256 prefix of ANR w[512]
            out[name + "_coef_sha"] = np.array(csha, np.uint8)          # per type: SHA-256 prefix of CLMS m_lmscoef[121]
            changed = int(np.count_nonzero(y != x))
            print("nr_ref.npz: %-26s %6d samples, %6d changed by NR" % (name, n, changed))
    out["names"] = np.array([s[0] for s in sc])
    c = consts()
    out["const_names"] = np.array(sorted(c))
    out["const_values"] = np.array([c[k] for k in sorted(c)], np.int32)
    np.savez_compressed(os.path.join(GOLD, "nr_ref.npz"), **out)


if __name__ == "__main__":
    main()
