"""Generates tests/golden/sam_ref.npz from the REFERENCE ITSELF: c2s_sound()'s synchronous-AM arm (rx/rx_sound.cpp:791-806 ->
rx/wdsp/SAM_demod.cpp) with the S-meter, CAgc, de-emphasis, payload and header statements around it.

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Like oracle/build_ref.sh's sndpath_ref, it cuts the line ranges of rx/rx_sound.cpp into a temporary directory
(deleted on exit), compiles tools/ref/ref_sam_main.cpp around them with the reference's agc.cpp, fir.cpp, squelch.cpp, ima_adpcm.cpp,
timing.cpp and rx/wdsp/SAM_demod.cpp linked where they lie, runs it on scripted scenarios and keeps only the data: the scripts, the
inputs made here from a fixed seed, and the outputs the reference's code produced (agc_samps_c and the packet payloads as
SHA-256 digests, to keep the file small).  Nothing of the reference's text enters the
repository.  Needs oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api (oracle/build_ref.sh makes both; run first if absent).

    python tools/make_ref_sam_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT  # ref_cut puts the repository root on sys.path
from tests.script_common import digest_u8 as digest  # noqa: E402
GOLD = os.path.join(ROOT, "tests", "golden")
SND = "rx/rx_sound.cpp"

# the cuts of oracle/build_ref.sh's sndpath_ref: (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    (SND, "SND_CUT_GPSCONST", 92, 93, "const double gps_delay    = ", "const double gps_week_sec = "),
    (SND, "SND_CUT_DECLS", 244, 250, "double z1 = 0;", "float sMeterAvg_dB = 0, sMeter_dBm;"),
    (SND, "SND_CUT_NORM", 306, 319, "int ref_nrx_samps = NRX_SAMPS_CHANS(8);", "}"),
    (SND, "SND_CUT_TICKS", 536, 537, "const u64_t ticks   = rx->ticks[rx->rd_pos];", "const u64_t dticks  = time_diff48(ticks, clk.ticks);"),
    (SND, "SND_CUT_GPSSEC", 557, 557, "s->gpssec = fmod(gps_week_sec + clk.gps_secs", "s->gpssec = fmod("),
    (SND, "SND_CUT_GPSSTAMP", 638, 661, "int sample_filter_delays = norm_nrx_samps - fir_pos;", "s->last_gpssec = s->gpssec;"),
    (SND, "SND_CUT_PKTINIT", 252, 255, 'strncpy(s->out_pkt_real.h.id, "SND", 3);', "s->seq = 0;"),
    (SND, "SND_CUT_MASKED", 285, 285, "bool masked = false, masked_area = false, check_masked = false;", "bool masked = false"),
    (SND, "SND_CUT_OVERLOAD", 295, 295, "bool squelched_overload = false;", "bool squelched_overload = false;"),
    (SND, "SND_CUT_FLAGS", 461, 482, "#define\tSND_FLAG_LPF", "bool do_de_emp = "),
    (SND, "SND_CUT_HOOKS", 488, 497, "u2_t bc = 0;", "tid_t receive_real_tid"),
    (SND, "SND_CUT_PATH", 676, 908, "TYPECPX *s_samps_c = fir_samps_c;", "}"),
    (SND, "SND_CUT_PACKET", 1035, 1140, "#define SILENCE_VALUE 1", "}"),
    (SND, "SND_CUT_HEADER", 1222, 1253, "#define SMETER_BIAS 127.0", "wf->snd_seq = s->seq;"),
]
# the SAM arm inside the path cut
ARM = [(SND, 791, "case MODE_SAM:"), (SND, 802, "wdsp_SAM_demod(rx_chan, s->mode, s->SAM_mparam, ns_out, agc_samps_c, out_samps_s2);"),
       (SND, 804, "m_chan_null_FIR[rx_chan].ProcessData(rx_chan, ns_out, agc_samps_c, NULL);")]


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(ARM)
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
    for top in ("extensions", "pkgs"):
        inc += [os.path.join(R, top, d) for d in sorted(os.listdir(os.path.join(R, top))) if os.path.isdir(os.path.join(R, top, d))]
    dfn = ["-std=gnu++11", "-DKIWI", "-DKIWISDR", "-DHOST", "-DDEBIAN_VERSION=11", "-DVERSION_MAJ=1", "-DVERSION_MIN=663", "-DARCH_CPU=x86",
           "-DCPU_AM3359", "-DPLATFORM_beaglebone_black"]
    cuts = ref_cut.cut_macros(CUTS)
    exe = os.path.join(tmp, "sam_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"]
           + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp] + cuts + ["-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_sam_main.cpp")]
           + [os.path.join(R, f) for f in ("rx/CuteSDR/agc.cpp", "rx/CuteSDR/fir.cpp", "rx/CuteSDR/squelch.cpp", "rx/csdr/ima_adpcm.cpp",
                                           "support/timing.cpp", "rx/wdsp/SAM_demod.cpp")]
           + ["-L/opt/rocm/lib", "-lhipfftw", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    return exe


# mode numbers: rx/mode.h:69-70
M_AM, M_AMN, M_USB, M_LSB, M_CW, M_CWN, M_NBFM, M_IQ, M_DRM, M_USN, M_LSN, M_SAM, M_SAU, M_SAL, M_SAS, M_QAM, M_NNFM = range(17)
rng = np.random.Generator(np.random.PCG64(0x5A3D0001))


def am_station(n, rate, f0=31.0, drift=2.5, amp=6000.0, fade=0.5, isb=True, noise=25.0, t0=0):
    """A broadcast as CFastFIR hands it over: a carrier f0 Hz off tune drifting by `drift` Hz/s, different audio on the two
    sidebands (an upper tone pair and a lower tone), selective fading of the carrier and the sidebands, noise."""
    t = (np.arange(n) + t0) / rate
    car_ph = 2 * np.pi * (f0 * t + 0.5 * drift * t * t) + 0.7
    fade_c = 1.0 - fade * 0.5 * (1 + np.sin(2 * np.pi * 0.8 * t))
    fade_s = 1.0 - fade * 0.5 * (1 + np.cos(2 * np.pi * 1.3 * t))
    usb = 0.35 * np.exp(2j * np.pi * 700.0 * t) + 0.2 * np.exp(2j * np.pi * 1900.0 * t)
    lsb = 0.3 * np.exp(-2j * np.pi * 1250.0 * t) if isb else 0.35 * np.exp(-2j * np.pi * 700.0 * t) + 0.2 * np.exp(-2j * np.pi * 1900.0 * t)
    x = amp * np.exp(1j * car_ph) * (fade_c + fade_s * (usb + lsb))
    return (x + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


AGC = "A 1 0 -100 50 6 1000"
B4 = ["B 512"] * 4                                       # one packet of compressed mono audio
sc = [
    # name, rate, script lines ("B n": a CFastFIR block; grouped into packets as the server does), the signal's keyword arguments
    ("sam_12k", 12000.0, [AGC, "M %d" % M_SAM] + B4, {}),
    ("sam_12k_am_first_then_sam", 12000.0, [AGC, "M %d" % M_AM] + B4 + ["M %d" % M_SAM] + B4, {"f0": -45.0}),
    ("sau_deemp_12k", 12000.0, [AGC, "E 1 0", "M %d" % M_SAU] + B4, {}),
    ("sal_fast_12k", 12000.0, [AGC, "G 2", "M %d" % M_SAL] + B4, {"f0": 12.0, "drift": -4.0}),
    ("sas_12k_le_be", 12000.0, [AGC, "W 1 1", "M %d" % M_SAS, "B 512", "B 512", "W 1 0", "B 512", "B 512"], {}),
    ("qam_dx_12k", 12000.0, [AGC, "G 0", "M %d" % M_QAM] + B4, {"f0": 8.0, "drift": 0.5}),
    ("sam_mparam_steps_12k", 12000.0, [AGC, "N 4", "M %d" % M_SAM] + B4 + ["N 8"] + B4 + ["N 12"] + B4, {"fade": 0.8}),
    ("sam_null_lsb_12k", 12000.0, [AGC, "N 1", "M %d" % M_SAM] + B4 + ["N 13"] + B4, {}),
    ("sam_null_usb_12k", 12000.0, [AGC, "N 2", "M %d" % M_SAM] + B4 + ["N 10", "E 2 0"] + B4, {}),
    ("sam_pll_reset_midstream", 12000.0, [AGC, "G 2", "M %d" % M_SAM] + B4 + ["G -1"] + B4, {"f0": 60.0}),
    ("sam_then_sas_then_qam", 12000.0, [AGC, "N 12", "M %d" % M_SAM] + B4 + ["M %d" % M_SAS, "B 512", "B 512", "M %d" % M_QAM, "B 512",
                                                                            "B 512"], {}),
    ("sau_sas_odd_blocks_raw", 12000.0, [AGC, "W 0 1", "N 4", "M %d" % M_SAU, "B 512", "B 301", "B 211", "B 512", "B 7", "M %d" % M_SAS,
                                        "B 333", "B 512"], {}),
    ("sam_agc_off", 12000.0, ["A 0 0 -100 40 6 1000", "N 8", "M %d" % M_SAM] + B4, {"amp": 900.0}),
    ("all_modes_20250", 20250.0, ["A 1 1 -90 50 4 500", "N 12", "M %d" % M_SAM] + B4 + ["M %d" % M_SAU] + B4 + ["M %d" % M_SAL] + B4
     + ["M %d" % M_SAS, "B 512", "B 512", "M %d" % M_QAM, "B 512", "B 512", "N 1", "M %d" % M_SAM] + B4, {"f0": -70.0, "drift": 6.0}),
    ("sau_deemp_20250_fast", 20250.0, [AGC, "E 1 0", "G 2", "M %d" % M_SAU] + B4, {"f0": 150.0}),
]


def script_of(rate, lines):
    """R / L first, then the lines with the blocks grouped into packets: 4 x 512 samples of compressed mono audio, one block otherwise"""
    fw_sel, nrx, adc = (2, 226, 66.6666e6) if rate > 15000 else (0, 170, 66.6666e6)
    script = ["R %r %d %d %d %r" % (rate, fw_sel, nrx, int(round(adc / rate)), adc), "L 4900.0 6000.0" if rate < 15000 else "L 6000.0 10125.0"]
    pend, comp, mode = [], 1, M_USB
    stereo = lambda m: m in (M_IQ, M_DRM, M_SAS, M_QAM)       # IS_STEREO (rx/mode.h:45-55)
    for ln in lines + ["#end"]:
        if ln[0] == "B":
            pend.append(int(ln.split()[1]))
            if len(pend) == (4 if comp and not stereo(mode) else 1):
                script.append("P " + " ".join(str(v) for v in pend)); pend = []
            continue
        if pend:
            script.append("P " + " ".join(str(v) for v in pend)); pend = []
        if ln[0] == "W":
            comp = int(ln.split()[1])
        if ln[0] == "M":
            mode = int(ln.split()[1])
        if ln[0] != "#":
            script.append(ln)
    return script


def pack(script, y):
    """The harness's float stream -> compact typed arrays (the golden file stays small): per block the 7-float record, out_samps_s2 of
    the mono blocks as int16, a 16-byte SHA-256 prefix of agc_samps_c (SAM-family and stereo blocks); per packet hsize / bc, the header
    bytes and a SHA-256 prefix of the payload bytes.  Equality of a digest is equality of the bytes."""
    stereo = lambda m: m in (M_IQ, M_DRM, M_SAS, M_QAM)
    rec, s16, agc_sha, plen, phead, psha = [], [], [], [], [], []
    mode, ypos = M_USB, 4                                 # (the first 4 floats: sndpath_ref's firmware-mode record, unused here)
    for line in script:
        f = line.split()
        if f[0] == "M":
            mode = int(f[1])
        if f[0] != "P":
            continue
        for n in (int(v) for v in f[1:]):
            rec.append(y[ypos:ypos + 7]); ypos += 7
            if not stereo(mode):
                s16.append(y[ypos:ypos + n].astype(np.int16)); ypos += n
            if stereo(mode) or M_SAM <= mode <= M_QAM:
                agc_sha.append(digest(y[ypos:ypos + 2 * n].astype(np.float32).tobytes())); ypos += 2 * n
        hsize, bc = int(y[ypos]), int(y[ypos + 1]); ypos += 2
        pkt = y[ypos:ypos + hsize + bc].astype(np.uint8); ypos += hsize + bc
        plen.append([hsize, bc]); phead.append(np.pad(pkt[:hsize], (0, 20 - hsize))); psha.append(digest(pkt[hsize:].tobytes()))
    assert ypos == y.size
    return {"rec": np.array(rec, np.float32), "s16": np.concatenate(s16 + [np.zeros(0, np.int16)]).astype(np.int16), "agc_sha": np.array(agc_sha, np.uint8).reshape(-1, 16),
            "pkt_len": np.array(plen, np.int32), "pkt_head": np.array(phead, np.uint8), "pkt_sha": np.array(psha, np.uint8)}


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, rate, lines, kw in sc:
            script = script_of(rate, lines)
            n = sum(sum(int(v) for v in l.split()[1:]) for l in script if l[0] == "P")
            # whole-number samples, kept as int16 pairs: a valid CFastFIR output that the golden file stores in half the bytes
            x = np.clip(np.round(am_station(n, rate, **kw).view(np.float32)), -32768, 32767).astype(np.int16)
            x.astype(np.float32).tofile(os.path.join(tmp, "in.bin"))
            open(os.path.join(tmp, "s.txt"), "w").write("\n".join(script) + "\n")
            subprocess.run([exe, os.path.join(tmp, "s.txt"), os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
            y = np.fromfile(os.path.join(tmp, "out.bin"), np.float32)
            out[name + "_script"] = np.array(script)
            out[name + "_rate"] = np.array([rate], np.float64)
            out[name + "_in"] = x
            for k, v in pack(script, y).items():
                out[name + "_" + k] = v
            print("sam_ref.npz: %-28s %5d samples in, %2d packets, %6d floats out" % (name, n, sum(l[0] == "P" for l in script), y.size))
    out["names"] = np.array([s[0] for s in sc])
    np.savez_compressed(os.path.join(GOLD, "sam_ref.npz"), **out)


if __name__ == "__main__":
    main()
