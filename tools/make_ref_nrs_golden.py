"""Generates tests/golden/nrs_ref.npz from the REFERENCE ITSELF: NR_SPECTRAL of c2s_sound()'s noise-reduction switch
(rx/rx_sound.cpp:933-949 -> rx/Teensy/NR_spectral.cpp) driven by the `SET nr` commands of rx/rx_sound_cmd.cpp (:464-471, :473-475,
:505-523) and the normalised passband of `SET mod=` (:252-266).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_nr_golden.py: the line ranges are cut (each checked against its text) into
a temporary directory (deleted on exit), tools/ref/ref_nrs_main.cpp is compiled around them with -O2 -ffp-contract=off, with
NR_spectral.cpp and the three CMSIS files it calls (arm_cfft_f32.cpp, arm_cfft_radix8_f32.cpp, arm_bitreversal2.cpp) compiled where
they lie; only data is kept.  Needs oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both).

THE TRANSFORM'S TABLES ARE OURS.  rx/CMSIS/arm_common_tables.h declares twiddleCoef_512[1024] and armBitRevIndexTable512[448] and
no file of the reference tree defines them, so the reference's FFT cannot be linked as it lies.  This builder supplies
twiddleCoef_512[2k], [2k+1] = (float) cos(2 pi k / 512), (float) sin(2 pi k / 512) evaluated in double (stored here as `twiddle`;
tests/test_nrs_cpu.py holds kg_tables.h's copy equal to it) and the harness the bit-reversal table as the 224 disjoint swaps
(8 i, 8 rev(i)).  With these the transform agrees with a double-precision DFT to 1.4e-7 of the largest bin (checked below).

Inputs come from a small pool of int16 streams made here from a fixed seed; a scenario names its stream, its first block and the
blocks it zeroes (tests/nrs_common.py rebuilds them), and the same stream serves 12000 and 20250.  Outputs are stored in full for
a few short scenarios and as per-block SHA-256 prefixes for the rest; the state arrays as NaN-canonical digests.

    python tools/make_ref_nrs_golden.py
"""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT, read  # ref_cut puts the repository root on sys.path
from tests.script_common import digest_u8 as digest  # noqa: E402
GOLD = os.path.join(ROOT, "tests", "golden")

CUTS = [
    ("rx/rx_sound_cmd.cpp", "NR_CUT_ALGO", 464, 471, "case CMD_NR_ALGO:", "break;"),
    ("rx/rx_sound_cmd.cpp", "NR_CUT_DECLS", 473, 475, "int n_type, n_en;", "float n_pval;"),
    ("rx/rx_sound_cmd.cpp", "NR_CUT_TYPE", 505, 523, "case CMD_NR_TYPE:", ""),
    ("rx/rx_sound_cmd.cpp", "NR_CUT_NORM", 252, 266, "// normalized passband", "}"),
    ("rx/rx_sound.cpp", "NR_CUT_STAGE", 933, 949, "// ordered so denoiser can cleanup residual noise from autonotch", "}"),
]
PINS = [("rx/rx_sound_cmd.cpp", 469, "memset(s->nr_enable, 0, sizeof(s->nr_enable));"),
        ("rx/rx_sound_cmd.cpp", 520, "case NR_SPECTRAL: nr_spectral_init(rx_chan, s->nr_param[n_type]); break;"),
        ("rx/rx_sound_cmd.cpp", 253, "if (s->locut <= 0 && s->hicut >= 0) {"),
        ("rx/rx_sound_cmd.cpp", 255, "s->norm_hicut = MAX(-s->locut, s->hicut);"),
        ("rx/rx_sound.cpp", 923, "if (!IQ_or_DRM_or_stereo) {"),
        ("rx/rx_sound.cpp", 946, "nr_spectral_process(rx_chan, ns_out, out_samps_s2, out_samps_s2);"),
        ("rx/Teensy/NR_spectral.cpp", 116, "assert(nsamps == FFT_FULL);"),
        ("rx/Teensy/NR_spectral.cpp", 334, "ai = FFT_FULL - bindx - 1;"),
        ("rx/CMSIS/arm_common_tables.h", 102, "extern const float32_t twiddleCoef_512[1024];"),
        ("rx/CMSIS/arm_common_tables.h", 334, "extern const uint16_t armBitRevIndexTable512[ARMBITREVINDEXTABLE_512_TABLE_LENGTH];")]
ENUMS = [("rx/rx_noise.h", "typedef enum { NR_OFF_ = 0, NR_WDSP = 1, NR_ORIG = 2, NR_SPECTRAL = 3 } nr_algo_e;"),
         ("rx/rx_noise.h", "#define NOISE_PARAMS 8")]
# constants of NR_spectral.cpp, read from its text: name -> (line fragment before the value)
SPECTRAL_CONSTS = [("FFT_FULL", "#define FFT_FULL"), ("psthr", "const f32_t psthr ="), ("pnsaf", "const f32_t pnsaf ="),
                   ("psini", "const f32_t psini ="), ("pspri", "const f32_t pspri ="), ("NR_width", "const int NR_width ="),
                   ("power_threshold", "const f32_t power_threshold ="), ("snr_prio_min_dB", "const f32_t snr_prio_min_dB =")]
PARAMS = ["NR_S_GAIN", "NR_ALPHA", "NR_ASNR"]


def consts():
    out = {}
    for rel, t in ENUMS:
        assert any(t in l for l in read(rel)), ("reference enum moved", rel, t)
    out.update(NR_SPECTRAL=3.0, NOISE_PARAMS=8.0)
    nf = read("extensions/noise_filter/noise_filter.h")
    for p in PARAMS:
        v = [l.split() for l in nf if l.startswith("#define") and l.split()[1] == p]
        assert len(v) == 1, p
        out[p] = float(v[0][2])
    sp = read("rx/Teensy/NR_spectral.cpp")
    for name, frag in SPECTRAL_CONSTS:
        v = [l for l in sp if l.strip().startswith(frag)]
        assert len(v) == 1, name
        out[name] = float(v[0].strip()[len(frag):].split(";")[0].split()[0])
    return out


def twiddle():
    t = np.empty(1024, np.float32)
    for k in range(512):
        a = 2.0 * math.pi * k / 512
        t[2 * k] = np.float32(math.cos(a)); t[2 * k + 1] = np.float32(math.sin(a))
    return t


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    # the tables are declared and nowhere defined: the reason this builder supplies them
    for d, _, files in os.walk(os.path.join(R, "rx")):
        for f in files:
            if f.endswith((".c", ".cpp", ".h")):
                txt = open(os.path.join(d, f), encoding="latin-1").read()
                assert "twiddleCoef_512[1024] =" not in txt and "armBitRevIndexTable512[ARMBITREVINDEXTABLE_512_TABLE_LENGTH] =" not in txt, \
                    ("the reference now defines the table itself: use it", d, f)
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
    exe = os.path.join(tmp, "nrs_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"] + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp]
           + ['-DNR_ANR_CPP="%s"' % os.path.join(R, "rx/wdsp/ANR.cpp"), '-DNR_SPECTRAL_CPP="%s"' % os.path.join(R, "rx/Teensy/NR_spectral.cpp"),
              "-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_nrs_main.cpp"), os.path.join(R, "rx/kiwi/lms.cpp"),
              os.path.join(R, "rx/CMSIS/arm_cfft_f32.cpp"), os.path.join(R, "rx/CMSIS/arm_cfft_radix8_f32.cpp"),
              os.path.join(R, "rx/CMSIS/arm_bitreversal2.cpp")]
           + ["-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


rng = np.random.Generator(np.random.PCG64(0x4E525301))
RATE = 12000.0
BLK = 512


def i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def sig_speech(nb):
    n = nb * BLK
    t = np.arange(n) / RATE
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    gate = 0.5 * (1 + np.sin(2 * np.pi * 3.1 * t)) ** 2
    return gate * (3000 * np.sin(ph) + 1800 * np.sin(3 * ph + 0.4) + 900 * np.sin(5 * ph + 1.1) + 700 * np.sin(9 * ph)) + 400 * rng.standard_normal(n)


def sig_tone(nb):
    n = nb * BLK
    t = np.arange(n) / RATE
    return 3000 * np.sin(2 * np.pi * 500 * t) + 2500 * np.sin(2 * np.pi * 1000 * t + 0.3) + 1200 * np.sin(2 * np.pi * 1800 * t) + 300 * rng.standard_normal(n)


def sig_burst(nb):
    x = 150 * rng.standard_normal(nb * BLK)
    for b in range(12, nb, 4):
        x[b * BLK:(b + 1) * BLK] *= 9
    return x


def sig_long(nb):
    n = nb * BLK
    t = np.arange(n) / RATE
    on = (np.arange(n) >= 14 * BLK).astype(float)
    return on * (8000 * np.sin(2 * np.pi * 700 * t) + 6000 * np.sin(2 * np.pi * 1500 * t) + 5000 * np.sin(2 * np.pi * 2300 * t + 1.0)) \
        + 300 * rng.standard_normal(n)


def sig_loud(nb):
    n = nb * BLK
    t = np.arange(n) / RATE
    return 30000 * np.sin(2 * np.pi * 450 * t) + 2000 * rng.standard_normal(n)


POOL = [("speech", sig_speech, 48), ("tone", sig_tone, 36), ("burst", sig_burst, 36), ("long", sig_long, 80), ("loud", sig_loud, 16)]

G_HI, G_LO = "%.9g" % 10 ** (30 / 20), "%.9g" % 10 ** (-30 / 20)        # the UI's gain slider, -30..30 dB
A_LO, A_HI = "0.9", "0.99"                                             # alpha slider
S_LO, S_HI = "%.9g" % 10 ** (2 / 10), "1000"                            # active-SNR slider, 2..30 dB


def params(t=0, gain="1", alpha="0.95", asnr="1000"):
    # the client's order and defaults (one parameter per command; every one re-inits from the type's whole vector)
    return ["P %d 0 %s" % (t, gain), "P %d 1 %s" % (t, alpha), "P %d 2 %s" % (t, asnr)]


def B(k, stereo=0):
    return ["B 512 %d" % stereo] * k


SSB = "M 300 2700"
# name, rate, pool stream, first block, zeroed blocks, full output kept, degenerate (outputs may equal inputs), script
sc = [
    ("speech12", 12000, "speech", 0, [], False, False, [SSB, "A 3"] + params() + B(40) + ["S"]),
    ("tone12", 12000, "tone", 0, [], False, False, [SSB, "A 3"] + params() + B(36) + ["S"]),
    ("burst12", 12000, "burst", 0, [], False, False, [SSB, "A 3"] + params() + B(36) + ["S"]),
    ("speech20", 20250, "speech", 4, [], False, False, [SSB, "A 3"] + params() + B(36) + ["S"]),
    ("tone20", 20250, "tone", 0, [], False, False, [SSB, "A 3"] + params() + B(32) + ["S"]),
    ("gain_hi_alpha_lo_asnr_lo", 12000, "speech", 8, [], False, False, [SSB, "A 3"] + params(0, G_HI, A_LO, S_LO) + B(32) + ["S"]),
    ("gain_lo_alpha_hi_type1", 12000, "tone", 2, [], False, False, [SSB, "A 3"] + params(1, G_LO, A_HI, S_HI) + B(32) + ["S"]),
    ("midstream_params", 12000, "speech", 2, [], False, False,
     [SSB, "A 3"] + params() + B(16) + ["P 1 1 0.9"] + B(8) + ["S", "P 0 2 10"] + B(8) + ["P 1 0 2"] + B(4) + ["S"]),
    ("never_initialised", 12000, "speech", 0, [], True, True, [SSB, "A 3"] + B(4) + ["S"]),
    ("select_leave_select", 12000, "tone", 0, [], False, True, [SSB, "A 3"] + params() + B(14) + ["S", "A 1"] + B(2) + ["A 3"] + B(16) + ["S"]),
    ("new_connection", 12000, "speech", 6, [], False, True,
     [SSB, "A 3"] + params() + B(14) + ["S", "C"] + B(1) + [SSB, "A 3"] + B(4) + ["S", "P 0 0 1"] + B(6) + ["S"]),
    ("am_passband", 12000, "burst", 0, [], False, False, ["M -4900 4900", "A 3"] + params() + B(32) + ["S"]),
    ("nbfm_passband", 12000, "speech", 10, [], False, False, ["M -5999 5999", "A 3"] + params() + B(30) + ["S"]),
    ("sam_passband_20k", 20250, "tone", 4, [], False, False, ["M -4900 4900", "A 3"] + params() + B(30) + ["S"]),
    ("lsb_passband", 12000, "tone", 6, [], False, False, ["M -2700 -300", "A 3"] + params() + B(30) + ["S"]),
    ("passband_change", 12000, "speech", 12, [], False, False,
     [SSB, "A 3"] + params() + B(16) + ["M -4900 4900"] + B(8) + ["S", "M 470 530"] + B(8) + ["S"]),
    ("cw_narrow", 12000, "tone", 0, [], False, False, ["M 470 530", "A 3"] + params() + B(24) + ["S"]),
    ("vad_high_17", 12000, "speech", 14, [], False, False, ["M 0 390", "A 3"] + params() + B(30) + ["S"]),
    ("vad_low_244", 12000, "burst", 4, [], False, False, ["M 5720 5999", "A 3"] + params() + B(30) + ["S"]),
    ("loud_wrap", 12000, "loud", 0, [], True, False, [SSB, "A 3"] + params(0, G_HI) + B(16) + ["S"]),
    ("zeros_start", 12000, "speech", 16, list(range(12)), False, True, [SSB, "A 3"] + params() + B(30) + ["S"]),
    ("zeros_mid", 12000, "speech", 18, [14, 15, 16, 17], False, True, [SSB, "A 3"] + params() + B(30) + ["S"]),
    ("stereo_skips", 12000, "speech", 3, [], False, True,
     [SSB, "A 3"] + params() + B(12) + B(2, 1) + B(10) + B(1, 1) + B(6) + ["S"]),
    ("long_tones_on", 12000, "long", 0, [], False, False, [SSB, "A 3"] + params() + B(80) + ["S"]),
]


def fdigest(b):
    """digest of a float32 vector with every NaN as 0x7FC00000 (tools/make_ref_nr_golden.py's rule: x86's default NaN is the
    negative quiet one, the GPU's the positive one)"""
    u = np.frombuffer(bytes(b), np.uint32).copy()
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return digest(u.tobytes())


REC = 2 * 4 + 12 * 4 + 9 * 256 * 4


def check_transform(tw):
    """the supplied tables against a double-precision DFT, through our own restatement of the radix-8 tree is NOT what is checked
    here: this is the table itself (cos / sin of the right angles, to float precision)"""
    k = np.arange(512)
    assert np.abs(tw[0::2] - np.cos(2 * np.pi * k / 512)).max() < 6e-8 and np.abs(tw[1::2] - np.sin(2 * np.pi * k / 512)).max() < 6e-8


def main():
    out = {}
    tw = twiddle()
    check_transform(tw)
    pool = {name: i16(f(nb)) for name, f, nb in POOL}
    nn_all, over_any, over_none = {}, False, False
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        P = lambda f: os.path.join(tmp, f)
        tw.tofile(P("tw.bin"))
        window = None
        for name, rate, src, off, zero, full, degenerate, script in sc:
            nb = sum(1 for l in script if l[0] == "B")
            x = pool[src][off * BLK:(off + nb) * BLK].copy()
            assert x.size == nb * BLK, (name, "the pool stream is too short")
            for z in zero:
                x[z * BLK:(z + 1) * BLK] = 0
            x.tofile(P("in.bin"))
            open(P("s.txt"), "w").write("\n".join(script) + "\n")
            subprocess.run([exe, str(rate), P("s.txt"), P("in.bin"), P("tw.bin"), P("out.bin"), P("st.bin"), P("tr.bin"), P("misc.bin")], check=True)
            y = np.fromfile(P("out.bin"), np.int16)
            assert y.size == x.size
            st = open(P("st.bin"), "rb").read()
            ns = script.count("S")
            assert len(st) == ns * REC, (name, len(st))
            tr = np.fromfile(P("tr.bin"), np.int32).reshape(-1, 4)
            misc = open(P("misc.bin"), "rb").read()
            oob = int(np.frombuffer(misc[:4], np.int32)[0])
            assert oob == 0, (name, "the reference indexed outside its arrays %d times: outside its defined behaviour" % oob)
            w = np.frombuffer(misc[4:], np.float32)
            assert window is None or np.array_equal(window, w)
            window = w.copy()
            ints, flts, shas = [], [], []
            for i in range(ns):
                r = st[i * REC:(i + 1) * REC]
                ints.append(np.frombuffer(r[:8], np.int32)); flts.append(np.frombuffer(r[8:56], np.float32))
                shas.append([fdigest(r[56 + 1024 * a:56 + 1024 * (a + 1)]) for a in range(9)])
            out[name + "_script"] = np.array(script)
            out[name + "_rate"] = np.int32(rate)
            out[name + "_src"] = np.array(src)
            out[name + "_off"] = np.int32(off)
            out[name + "_zero"] = np.array(zero, np.int32)
            out[name + "_degenerate"] = np.int32(degenerate)
            if full:
                out[name + "_out"] = y.copy()
            out[name + "_out_sha"] = np.array([digest(y[b * BLK:(b + 1) * BLK].tobytes()) for b in range(nb)], np.uint8)
            out[name + "_state_i"] = np.array(ints, np.int32)       # per S: first_time, init_counter
            out[name + "_state_f"] = np.array(flts, np.float32)     # per S: final_gain, alpha, asnr, xih1r, pfac, tinc, tax, tap, ax, ap, norm_locut, norm_hicut
            out[name + "_state_sha"] = np.array(shas, np.uint8)     # per S: the nine arrays, in nr_spectral_t's order
            out[name + "_trace"] = tr                               # per spectral block: NN, NN, bins with pslp > psthr, first_time
            hist = {}
            for v in tr[:, :2].ravel():
                if v:
                    hist[int(v)] = hist.get(int(v), 0) + 1
                    nn_all[int(v)] = nn_all.get(int(v), 0) + 1
            p3 = tr[tr[:, 3] == 3]
            over_any |= bool((p3[:, 2] > 0).any()); over_none |= bool((p3[:, 2] == 0).any())
            same = [b for b in range(nb) if np.array_equal(y[b * BLK:(b + 1) * BLK], x[b * BLK:(b + 1) * BLK])]
            assert degenerate or not same, (name, "blocks left unchanged", same)
            print("nrs_ref.npz: %-26s %5d Hz %3d blocks, %6d of %6d samples changed, first_time %d, NN %s, max bins over psthr %d"
                  % (name, rate, nb, int(np.count_nonzero(y != x)), x.size, ints[-1][0], dict(sorted(hist.items())), int(tr[:, 2].max()) if len(tr) else 0))
    assert set(nn_all) == {1, 3, 5, 7, 9}, nn_all
    assert over_any and over_none
    print("NN over all phase-3 frames:", dict(sorted(nn_all.items())))
    out["names"] = np.array([s[0] for s in sc])
    for name, _, _ in POOL:
        out["pool_" + name] = pool[name]
    out["twiddle"] = tw
    out["window"] = window
    c = consts()
    out["const_names"] = np.array(sorted(c))
    out["const_values"] = np.array([c[k] for k in sorted(c)], np.float64)
    path = os.path.join(GOLD, "nrs_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
