"""Generates tests/golden/nb_ref.npz from the REFERENCE ITSELF: CuteSDR's CNoiseProc (rx/CuteSDR/noiseproc.cpp) as its two call sites
drive it -- the audio blanker of rx/rx_sound.cpp:597 (ProcessBlanker in place on the unpacked block) and the waterfall blanker of
rx/rx_waterfall.cpp:1092 / :1098 (SetupBlanker("WF", WF_C_NSAMPS, ...), ProcessBlankerOneShot on the windowed frame).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Like tools/make_ref_nr_golden.py, it cuts those statements (each checked against its text) into a temporary
directory (deleted on exit), compiles tools/ref/ref_nb_main.cpp around them with -O2 -ffp-contract=off (oracle/build_ref.sh's flags),
with rx/CuteSDR/noiseproc.cpp linked where it lies, runs it on scripted scenarios and keeps only the data: the scripts, the seeds
of the inputs (tests/nb_signals.py regenerates them), the outputs (audio: SHA-256 prefixes per block and the mask of blanked
samples; waterfall: SHA-256 prefixes per frame plus a few whole frames) and the end states.  Nothing of the reference's text enters
the repository.  Needs oracle/_ref/gen/kiwi.gen.h (oracle/build_ref.sh makes it; run first if absent).

    python tools/make_ref_nb_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT, read  # ref_cut puts the repository root on sys.path
from tests.script_common import digest_u8 as digest  # noqa: E402
from tests import nb_signals  # noqa: E402
from flydog_sdr_gps_amd import wf as wf_mod  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

# (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    ("rx/rx_sound.cpp", "NB_CUT_SND", 597, 597, "m_NoiseProc_snd[rx_chan].ProcessBlanker(ns_in, in_samps_c, in_samps_c);", ""),
    ("rx/rx_waterfall.cpp", "NB_CUT_WF_SETUP", 1092, 1092, 'm_NoiseProc_wf[rx_chan].SetupBlanker("WF", srate, wf->nb_param[NB_BLANKER]);', ""),
    ("rx/rx_waterfall.cpp", "NB_CUT_WF_ONESHOT", 1098, 1098,
     "m_NoiseProc_wf[rx_chan].ProcessBlankerOneShot(WF_C_NSAMPS, (TYPECPX*) fft->hw_c_samps, (TYPECPX*) fft->hw_c_samps);", ""),
]
# the statements around the cuts that the harness relies on
PINS = [("rx/rx_sound.cpp", 596, "if (s->nb_enable[NB_BLANKER] && s->nb_algo == NB_STD)"),
        ("rx/rx_sound.cpp", 593, "//#define NB_STD_POST_FILTER"),
        ("rx/rx_waterfall.cpp", 1087, "if (wf->nb_enable[NB_BLANKER] && wf->nb_enable[NB_WF]) {"),
        ("rx/rx_waterfall.cpp", 1090, "u4_t srate = WF_C_NSAMPS;"),
        ("rx/rx_waterfall.cpp", 1097, "if (wf->nb_setup)"),
        ("rx/rx_waterfall.cpp", 460, "if (wf->nb_enable[NB_BLANKER] && wf->nb_enable[NB_WF]) wf->nb_param_change[NB_BLANKER] = true;"),
        ("rx/CuteSDR/noiseproc.cpp", 48, "#define MAX_GATE 4096"),
        ("rx/CuteSDR/noiseproc.cpp", 52, "#define MAGAVE_TIME 0.005")]
# the reference's enum values and parameter indices (rx/rx_noise.h:3-7, extensions/noise_blank/noise_blank.h), pinned by text
ENUMS = [("rx/rx_noise.h", "typedef enum { NB_OFF = 0, NB_STD = 1, NB_WILD = 2 } nb_algo_e;"),
         ("rx/rx_noise.h", "typedef enum { NB_BLANKER = 0, NB_WF = 1, NB_CLICK = 2 } nb_type_e;"),
         ("rx/rx_noise.h", "#define NOISE_PARAMS 8"),
         ("rx/rx_noise.h", "#define NOISE_TYPES 4")]
PARAMS = ["NB_GATE", "NB_THRESHOLD"]


def consts():
    """name -> value of the reference's NB constants, read from its text"""
    for rel, t in ENUMS:
        assert any(t in l for l in read(rel)), ("reference enum moved", rel, t)
    out = dict(NB_OFF=0, NB_STD=1, NB_WILD=2, NB_BLANKER=0, NB_WF=1, NB_CLICK=2, NOISE_PARAMS=8, NOISE_TYPES=4)
    nb = read("extensions/noise_blank/noise_blank.h")
    for p in PARAMS:
        v = [l.split() for l in nb if l.startswith("#define") and l.split()[1] == p]
        assert len(v) == 1, p
        out[p] = int(v[0][2])
    return out


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    gen = os.path.join(REF, "gen")
    if not os.path.isfile(os.path.join(gen, "kiwi.gen.h")):
        sys.exit("oracle/_ref/gen/kiwi.gen.h missing: run oracle/build_ref.sh first")
    inc = [R] + [os.path.join(R, d) for d in ("gps", "rx", "rx/CuteSDR", "rx/csdr", "rx/kiwi", "rx/wdsp", "rx/Teensy", "support",
                                               "platform/common", "platform/beaglebone", "arch/sitara", "init", "net", "web", "dev", "ui",
                                               "extensions", "pkgs", "pkgs/mongoose", "pkgs/jsmn", "pkgs/sha256")]
    for top in ("rx", "extensions", "pkgs"):
        for d, subs, _ in os.walk(os.path.join(R, top)):
            if d.count(os.sep) - os.path.join(R, top).count(os.sep) <= 2:
                inc.append(d)
    dfn = ["-std=gnu++11", "-DKIWI", "-DKIWISDR", "-DHOST", "-DDEBIAN_VERSION=11", "-DVERSION_MAJ=1", "-DVERSION_MIN=663", "-DARCH_CPU=x86",
           "-DCPU_AM3359", "-DPLATFORM_beaglebone_black"]
    exe = os.path.join(tmp, "nb_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp]
           + ["-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_nb_main.cpp"), os.path.join(R, "rx/CuteSDR/noiseproc.cpp")]
           + ["-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


def blocks(sizes):
    return ["B %d" % n for n in sizes]


# audio scenarios: name, script, signal kind, seed
AUDIO = [
    ("snd12k_mid", ["U 12000 100 50"] + blocks([512] * 8) + ["S"], "noise_pulses", 1),
    ("snd20250", ["U 20250 200 30"] + blocks([512] * 8) + ["S"], "carrier_pulses", 2),
    ("snd_corrected", ["U 12000.37 150 40"] + blocks([512] * 8) + ["S"], "noise_pulses", 3),
    ("snd_gate_below3", ["U 12000 50 50"] + blocks([512] * 6) + ["S"], "noise_pulses", 4),
    ("snd_gate_clamped", ["U 12000 1000000 20"] + blocks([4096, 4096, 1000]) + ["S"], "quiet_then_loud", 5),
    ("snd_th0", ["U 12000 100 0"] + blocks([512] * 6) + ["S"], "quiet_then_loud", 6),
    ("snd_th100", ["U 12000 100 100"] + blocks([512] * 6) + ["S"], "noise_pulses", 7),
    ("snd_th_above", ["U 12000 300 250"] + blocks([512] * 6) + ["S"], "carrier_pulses", 8),
    ("snd_th_nan", ["U 12000 100 nan"] + blocks([512] * 4) + ["S"], "noise_pulses", 9),
    ("snd_chunked", ["U 12000 100 50"] + blocks([7, 300, 1, 1024, 0, 205, 512, 2047, 1]) + ["S"], "noise_pulses", 1),
    ("snd_setup_between", ["U 12000 100 50"] + blocks([512] * 3) + ["S", "U 20250 400 20"] + blocks([512] * 3) + ["S", "U 0 5 5"]
     + blocks([512] * 2) + ["S"], "carrier_pulses", 10),
    ("snd_long_block", ["U 12000 2000 60"] + blocks([10000]) + ["S"], "noise_pulses", 11),
]
# waterfall scenarios: name, script, frame kind, seed, number of frames, window function
WF = [
    ("wf_seq", ["W 100 50"] + ["F"] * 10 + ["T"], "noise_pulses", 21, 10, wf_mod.WINF_HANNING),
    ("wf_wide_flush", ["W 100000 30"] + ["F"] * 8 + ["T"], "silent_loud", 22, 8, wf_mod.WINF_BLACKMAN_HARRIS),
    ("wf_setup_between", ["W 600 40"] + ["F"] * 4 + ["T", "W 2000 20"] + ["F"] * 4 + ["T"], "noise_pulses", 23, 8, wf_mod.WINF_HAMMING),
]
KEEP_FRAMES = {"wf_seq": [0, 5], "wf_wide_flush": [2], "wf_setup_between": [4]}


def run(exe, tmp, script, x):
    np.ascontiguousarray(x, np.float32).tofile(os.path.join(tmp, "in.bin"))
    open(os.path.join(tmp, "s.txt"), "w").write("\n".join(script) + "\n")
    subprocess.run([exe, os.path.join(tmp, "s.txt"), os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
    return open(os.path.join(tmp, "out.bin"), "rb").read()


def split(raw, script, unit):
    """the outputs of each B / F line and the states of each S / T line"""
    outs, ints, flts, p = [], [], [], 0
    for l in script:
        if l[0] in "BF":
            n = unit if l[0] == "F" else int(l.split()[1])
            outs.append(np.frombuffer(raw[p:p + 8 * n], np.float32).reshape(n, 2)); p += 8 * n
        elif l[0] in "ST":
            ints.append(np.frombuffer(raw[p:p + 24], np.int32)); flts.append(np.frombuffer(raw[p + 24:p + 32], np.float32)); p += 32
    assert p == len(raw)
    return outs, np.array(ints, np.int32), np.array(flts, np.float32)


def main():
    out = {}
    win = wf_mod.window_functions()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, script, kind, seed in AUDIO:
            n = sum(int(l.split()[1]) for l in script if l[0] == "B")
            x = nb_signals.audio(kind, n, seed)
            outs, si, sf = split(run(exe, tmp, script, x), script, 0)
            y = np.concatenate(outs) if outs else np.zeros((0, 2), np.float32)
            out[name + "_script"] = np.array(script)
            out[name + "_sig"] = np.array([kind, str(seed)])
            out[name + "_sha"] = np.array([digest(o.tobytes()) for o in outs], np.uint8)
            out[name + "_blanked"] = np.packbits(np.all(y == 0, axis=1))
            out[name + "_state_i"] = si
            out[name + "_state_f"] = sf
            print("nb_ref.npz: %-20s %6d samples, %6d blanked" % (name, n, int(np.count_nonzero(np.all(y == 0, axis=1)))))
        for name, script, kind, seed, nf, wfn in WF:
            frames = nb_signals.wf_frames(kind, nf, seed)
            x = nb_signals.windowed(frames, win[wfn])
            outs, si, sf = split(run(exe, tmp, script, x), script, 8192)
            out[name + "_script"] = np.array(script)
            out[name + "_sig"] = np.array([kind, str(seed), str(nf), str(wfn)])
            out[name + "_sha"] = np.array([digest(o.tobytes()) for o in outs], np.uint8)
            keep = KEEP_FRAMES[name]
            out[name + "_keep"] = np.array(keep, np.int32)
            out[name + "_frames"] = np.array([outs[k] for k in keep], np.float32)
            out[name + "_state_i"] = si
            out[name + "_state_f"] = sf
            print("nb_ref.npz: %-20s %6d frames, %6d blanked samples" % (name, nf, sum(int(np.count_nonzero(np.all(o == 0, axis=1))) for o in outs)))
    out["audio_names"] = np.array([s[0] for s in AUDIO])
    out["wf_names"] = np.array([s[0] for s in WF])
    c = consts()
    out["const_names"] = np.array(sorted(c))
    out["const_values"] = np.array([c[k] for k in sorted(c)], np.int32)
    np.savez_compressed(os.path.join(GOLD, "nb_ref.npz"), **out)


if __name__ == "__main__":
    main()
