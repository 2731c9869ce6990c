"""Generates tests/golden/nbw_ref.npz from the REFERENCE ITSELF: NB_WILD of c2s_sound()'s noise-blanker switch
(rx/rx_sound.cpp:922-931 -> rx/Teensy/NB_Wild.cpp) driven by the `SET nb` commands of rx/rx_sound_cmd.cpp (:454-462, :473-475,
:477-503).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_nrs_golden.py: the line ranges are cut (each checked against its text) into
a temporary directory (deleted on exit), tools/ref/ref_nbw_main.cpp is compiled around them with -O2 -ffp-contract=off, with
NB_Wild.cpp, the eight CMSIS files it calls (arm_dot_prod_f32, arm_fir_init_f32, arm_fir_f32, arm_var_f32, arm_power_f32,
arm_negate_f32, arm_mult_f32, arm_add_f32) and rx/CuteSDR/noiseproc.cpp compiled where they lie; only data is kept.  Needs
oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both).

Inputs come from the seeded pool of tests/nbw_common.py (the file holds each stream's digest, not the stream); a scenario names its
stream, its first block, the blocks it zeroes and the clicks it adds, and a 12000 and a 20250 Hz connection share streams: the stage
has no rate.  Outputs are stored in full for the short scenarios and as per-block SHA-256 prefixes for all; per block that ran the
stage the number of hits and the largest |float| handed to the int16 conversion; at every S the state.

    python tools/make_ref_nbw_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT, read  # ref_cut puts the repository root on sys.path
from tests import nbw_common as C  # noqa: E402

BLK = C.BLK

CUTS = [
    ("rx/rx_sound_cmd.cpp", "NBW_CUT_ALGO", 454, 462, "case CMD_NB_ALGO:", "break;"),
    ("rx/rx_sound_cmd.cpp", "NBW_CUT_DECLS", 473, 475, "int n_type, n_en;", "float n_pval;"),
    ("rx/rx_sound_cmd.cpp", "NBW_CUT_TYPE", 477, 503, "case CMD_NB_TYPE:", "break;"),
    ("rx/rx_sound.cpp", "NBW_CUT_STAGE", 922, 931, "// noise & autonotch processors that only operate on real samples", "}"),
]
PINS = [("rx/rx_sound_cmd.cpp", 459, "memset(s->nb_enable, 0, sizeof(s->nb_enable));"),
        ("rx/rx_sound_cmd.cpp", 490, "if (s->nb_algo == NB_STD || n_type == NB_CLICK) {"),
        ("rx/rx_sound_cmd.cpp", 498, "case NB_WILD: nb_Wild_init(rx_chan, s->nb_param[n_type]); break;"),
        ("rx/rx_sound.cpp", 923, "if (!IQ_or_DRM_or_stereo) {"),
        ("rx/rx_sound.cpp", 924, "if (s->nb_enable[NB_BLANKER]) {"),
        ("rx/rx_sound.cpp", 929, "case NB_WILD: nb_Wild_process(rx_chan, ns_out, out_samps_s2, out_samps_s2); break;"),
        ("rx/rx_sound.cpp", 236, "memset(s, 0, sizeof(snd_t));"),
        ("rx/Teensy/NB_Wild.cpp", 27, "#define WORKING_BUFFER"),
        ("rx/Teensy/NB_Wild.cpp", 41, "memset(w, 0, sizeof(nb_Wild_t));"),
        ("rx/Teensy/NB_Wild.cpp", 112, "R[0] = R[0] * (1.0 + 1.0e-9);"),
        ("rx/Teensy/NB_Wild.cpp", 199, "assert_array_dim(i, DIM_WBUF);"),
        ("rx/Teensy/NB_Wild.cpp", 202, "assert_array_dim(i, DIM_WBUF);"),
        ("rx/rx_init.cpp", 369, 'cfg_default_float("nb_thresh2", 0.95, &update_cfg);'),
        ("rx/rx_init.cpp", 370, 'cfg_default_int("nb_taps", 10, &update_cfg);'),
        ("rx/rx_init.cpp", 371, 'cfg_default_int("nb_samps", 7, &update_cfg);')]
ENUMS = [("rx/rx_noise.h", "typedef enum { NB_OFF = 0, NB_STD = 1, NB_WILD = 2 } nb_algo_e;"),
         ("rx/rx_noise.h", "typedef enum { NB_BLANKER = 0, NB_WF = 1, NB_CLICK = 2 } nb_type_e;"),
         ("rx/rx_noise.h", "#define NOISE_PARAMS 8")]
PARAMS = ["NB_THRESH", "NB_TAPS", "NB_SAMPLES"]
WILD_CONSTS = [("MAX_ORDER", "#define MAX_ORDER"), ("MAX_IMPULSE_LEN", "#define MAX_IMPULSE_LEN"), ("N_IMPULSE_COUNT", "#define N_IMPULSE_COUNT")]
CMSIS = ["arm_dot_prod_f32", "arm_fir_init_f32", "arm_fir_f32", "arm_var_f32", "arm_power_f32", "arm_negate_f32", "arm_mult_f32", "arm_add_f32"]


def consts():
    for rel, t in ENUMS:
        assert any(t in l for l in read(rel)), ("reference enum moved", rel, t)
    out = dict(NB_WILD=2.0, NB_BLANKER=0.0, NOISE_PARAMS=8.0, default_thresh=0.95, default_taps=10.0, default_samples=7.0)
    nb = read("extensions/noise_blank/noise_blank.h")
    for p in PARAMS:
        v = [l.split() for l in nb if l.startswith("#define") and l.split()[1] == p]
        assert len(v) == 1, p
        out[p] = float(v[0][2])
    w = read("rx/Teensy/NB_Wild.cpp")
    for name, frag in WILD_CONSTS:
        v = [l for l in w if l.strip().startswith(frag)]
        assert len(v) == 1, name
        out[name] = float(v[0].strip()[len(frag):].split()[0])
    return out


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    # the scalar forms are what the reference's build compiles: no Makefile asks for another (and the harness refuses to compile if
    # arm_math.h switches one on for this machine)
    for f in os.listdir(R):
        if f.startswith("Makefile"):
            assert "ARM_MATH_" not in open(os.path.join(R, f), encoding="latin-1").read(), ("the reference now builds another CMSIS form", f)
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
    exe = os.path.join(tmp, "nbw_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"] + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp]
           + ['-DNB_WILD_CPP="%s"' % os.path.join(R, "rx/Teensy/NB_Wild.cpp"), "-no-pie", "-o", exe,
              os.path.join(ROOT, "tools", "ref", "ref_nbw_main.cpp"), os.path.join(R, "rx/CuteSDR/noiseproc.cpp")]
           + [os.path.join(R, "rx/CMSIS", f + ".cpp") for f in CMSIS] + ["-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


def params(thresh="0.95", taps="10", samples="7"):
    # the client's order (one parameter per command; every one runs nb_Wild_init from the whole stored vector)
    return ["P 0 0 %s" % thresh, "P 0 1 %s" % taps, "P 0 2 %s" % samples]


def B(k, stereo=0):
    return ["B 512 %d" % stereo] * k


ON = ["E 0 1"]
CLICK = 14000


def edge_clicks(order_pl):
    """clicks in the last and in the first order + PL samples of a block (repairs that read and write across the carried history)"""
    out = []
    for b, d in ((2, -3), (4, -order_pl + 1), (6, -1), (8, 2), (10, order_pl - 2), (12, 0), (14, -order_pl // 2), (15, order_pl // 2)):
        out.append((b * BLK + d, 1, CLICK if b % 4 else -CLICK))
    return out


# name, rate, pool stream, first block, zeroed blocks, own clicks, full output kept, must repair, script
sc = [
    ("defaults_noisy", 12000, "speech", 0, [], [], False, True, ["A 2"] + params() + ON + B(40) + ["S"]),
    ("sparse", 12000, "clicks", 0, [], [], False, True, ["A 2"] + params("3") + ON + B(40) + ["S"]),
    ("sparse_20250", 20250, "clicks", 0, [], [], False, True, ["A 2"] + params("3") + ON + B(40) + ["S"]),
    ("limits_40_41", 12000, "clicks", 4, [], [], False, True, ["A 2"] + params("5", "40", "41") + ON + B(40) + ["S"]),
    ("least_1_2", 12000, "clicks", 8, [], [], False, True, ["A 2"] + params("0.95", "1", "2") + ON + B(24) + ["S"]),
    ("even_samples_12", 12000, "clicks", 2, [], [], False, True, ["A 2"] + params("4", "16", "12") + ON + B(24) + ["S"]),
    ("never_triggers", 12000, "clicks", 0, [], [], True, False, ["A 2"] + params("20") + ON + B(12) + ["S"]),
    ("silence_then_signal", 12000, "clicks", 10, [0, 1, 2, 3, 4, 5], [], False, True, ["A 2"] + params("3") + ON + B(6) + ["S"] + B(18) + ["S"]),
    ("silence_mid", 12000, "speech", 6, [9, 10, 11], [], False, True, ["A 2"] + params() + ON + B(20) + ["S"]),
    ("edge_clicks", 12000, "quiet", 0, [], edge_clicks(13), True, True, ["A 2"] + params("3") + ON + B(16) + ["S"]),
    ("edge_clicks_40_41", 12000, "quiet", 8, [], edge_clicks(60), False, True, ["A 2"] + params("5", "40", "41") + ON + B(16) + ["S"]),
    ("close_clicks", 12000, "quiet", 4, [],
     [(2 * BLK + 200, 1, CLICK), (2 * BLK + 209, 1, -CLICK), (5 * BLK + 100, 2, CLICK), (5 * BLK + 106, 1, CLICK), (5 * BLK + 112, 1, -CLICK),
      (7 * BLK + 508, 1, CLICK), (8 * BLK + 4, 1, CLICK)], True, True, ["A 2"] + params("3") + ON + B(10) + ["S"]),
    ("reinit_midstream", 12000, "clicks", 12, [], [], False, True,
     ["A 2"] + params("3") + ON + B(8) + ["S", "P 0 1 20", "S"] + B(8) + ["S", "P 0 0 2"] + B(8) + ["S"]),
    ("three_messages_fresh", 12000, "clicks", 20, [], [], False, True,
     ["A 2", "S", "P 0 0 3", "S", "P 0 1 10", "S", "P 0 2 7", "S"] + ON + B(12) + ["S"]),
    ("stereo_skips", 12000, "clicks", 16, [], [], False, True, ["A 2"] + params("3") + ON + B(6) + B(2, 1) + B(6) + B(1, 1) + B(5) + ["S"]),
    ("enable_off_on", 12000, "clicks", 24, [], [], False, True, ["A 2"] + params("3") + ON + B(6) + ["E 0 0"] + B(3) + ON + B(7) + ["S"]),
    ("new_connection", 12000, "clicks", 28, [], [], False, True,
     ["A 2"] + params("3") + ON + B(8) + ["S", "C"] + B(2) + ["A 2"] + ON + B(8) + ["S"]),
    ("algo_away_and_back", 12000, "clicks", 30, [], [], False, True,
     ["A 2"] + params("3") + ON + B(6) + ["A 1"] + B(2) + ["A 2"] + B(2) + ON + B(8) + ["S"]),
    ("loud", 12000, "loud", 0, [], [], True, True, ["A 2"] + params("3") + ON + B(24) + ["S"]),
    ("loud_defaults", 12000, "loud", 0, [], [], False, True, ["A 2"] + params() + ON + B(24) + ["S"]),
]
FULL_BUDGET = 300535          # tests/golden/nrs_ref.npz


def main():
    out = {}
    streams = C.pool()
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        P = lambda f: os.path.join(tmp, f)
        by_script = {}
        for name, rate, src, off, zero, clicks, full, repairs, script in sc:
            nb = sum(1 for l in script if l[0] == "B")
            x = C.make_input(streams, src, off, nb, zero, clicks)
            x.tofile(P("in.bin"))
            open(P("s.txt"), "w").write("\n".join(script) + "\n")
            subprocess.run([exe, P("s.txt"), P("in.bin"), P("out.bin"), P("st.bin"), P("tr.bin"), P("misc.bin"), str(rate)], check=True)
            y = np.fromfile(P("out.bin"), np.int16)
            assert y.size == x.size
            states = C.split_states(open(P("st.bin"), "rb").read())
            assert len(states) == script.count("S"), name
            hits, mx = C.split_trace(open(P("tr.bin"), "rb").read())
            oob, dim_wbuf, outbuf = (int(v) for v in np.fromfile(P("misc.bin"), np.int32))
            assert oob == 0, (name, "the reference indexed outside its arrays %d times" % oob)
            assert np.isfinite(mx).all(), (name, "a NaN reached the int16 conversion")
            assert not repairs or hits.sum() > 0, (name, "meant to repair and never hit")
            assert repairs or hits.sum() == 0, (name, "meant never to trigger", hits)
            out[name + "_script"] = np.array(script)
            out[name + "_rate"] = np.int32(rate)
            out[name + "_src"] = np.array(src)
            out[name + "_off"] = np.int32(off)
            out[name + "_zero"] = np.array(zero, np.int32)
            out[name + "_clicks"] = np.array(clicks, np.int32).reshape(-1, 3)
            if full:
                out[name + "_out"] = y.copy()
            out[name + "_out_sha"] = np.array([np.frombuffer(C.digest(y[b * BLK:(b + 1) * BLK].tobytes()), np.uint8) for b in range(nb)], np.uint8)
            out[name + "_state_i"] = np.array([s[0] for s in states], np.int32)      # per S: taps, impulse_samples, nb_algo, nb_enable[NB_BLANKER]
            out[name + "_state_t"] = np.array([s[1][0] for s in states], np.float32)  # per S: thresh
            out[name + "_state_h"] = np.array([s[2] for s in states], np.float32)     # per S: working_buffer[0 .. 120), 0 from 2 order + 2 PL on
            out[name + "_hits"] = hits
            out[name + "_max_abs"] = mx
            worst = max(worst, float(mx.max()) if mx.size else 0.0)
            key = (src, off, tuple(zero), tuple(clicks), tuple(script))
            if key in by_script:
                assert np.array_equal(y, by_script[key]), (name, "the same stream and script at another rate gave another output")
            by_script[key] = y
            print("nbw_ref.npz: %-22s %5d Hz %3d blocks, %5d samples changed beyond the delay, hits/block max %2d sum %4d in %2d blocks, max |float| %.1f"
                  % (name, rate, nb, changed(x, y, states, script), int(hits.max()) if hits.size else 0, int(hits.sum()),
                     int(np.count_nonzero(hits)), float(mx.max()) if mx.size else 0.0))
        assert int(out["defaults_noisy_hits"].max()) == 20, "the defaults on noisy input are meant to reach the cap of 20 hits"
        assert np.array_equal(out["sparse_out_sha"], out["sparse_20250_out_sha"])
    out["names"] = np.array([s[0] for s in sc])
    out["pool_names"] = np.array(sorted(streams))
    out["pool_sha"] = np.array([np.frombuffer(C.digest(streams[k].tobytes()), np.uint8) for k in sorted(streams)], np.uint8)
    out["leaves_int16"] = np.int32(worst > 32767.0)
    c = consts()
    c.update(DIM_WBUF=float(dim_wbuf), FASTFIR_OUTBUF_SIZE=float(outbuf))
    out["const_names"] = np.array(sorted(c))
    out["const_values"] = np.array([c[k] for k in sorted(c)], np.float64)
    path = os.path.join(C.GOLD, "nbw_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("largest |float| handed to the int16 conversion over all scenarios: %.1f (%s int16)" % (worst, "LEAVES" if worst > 32767.0 else "inside"))
    print("wrote %s, %d bytes" % (path, size))
    assert size <= FULL_BUDGET, size


def changed(x, y, states, script):
    """samples of y that differ from x delayed by the scenario's first order + PL (a figure for the log only; scenarios that change
    the delay or skip blocks show large numbers)"""
    taps = impulse = None
    for l in script:
        f = l.split()
        if f[0] == "P" and f[1] == "0" and f[2] == "1" and taps is None:
            taps = int(float(f[3]))
        if f[0] == "P" and f[1] == "0" and f[2] == "2" and impulse is None:
            impulse = int(float(f[3]))
    d = taps + ((impulse | 1) - 1) // 2
    return int(np.count_nonzero(y[d:] != x[:-d]))


if __name__ == "__main__":
    main()
