"""Generates tests/golden/post_rand_ref.npz from the REFERENCE ITSELF: c2s_sound()'s body from `s_samps_c = fir_samps_c` down to the
end of the noise-reduction switch (rx/rx_sound.cpp:676-949) as one program with every stage linked, driven by the seeded random
scripts and the AGC-window shapes of tests/post_random.py.

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_sam_golden.py and its siblings for the Wild and NR stages: the line ranges
are cut (each checked against its text) into a temporary directory (deleted on exit), tools/ref/ref_post_main.cpp is compiled around
them with -O2 -ffp-contract=off, with agc.cpp, fir.cpp, squelch.cpp, noiseproc.cpp, ima_adpcm.cpp, timing.cpp, SAM_demod.cpp, lms.cpp
and the CMSIS files compiled where they lie; only data is kept.  Needs oracle/_ref/gen/kiwi.gen.h and oracle/_ref/fftw3_api
(oracle/build_ref.sh makes both).  The transform's two tables are ours, as in tools/make_ref_nrs_golden.py.

    python tools/make_ref_post_golden.py --random              # writes the golden
    python tools/make_ref_post_golden.py --search [first [n]]  # the first base whose 40 seeds reach every condition
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, REF, ROOT  # ref_cut puts the repository root on sys.path
import make_ref_sam_golden as sam
import make_ref_nbw_golden as nbw
import make_ref_nrs_golden as nrs
import make_ref_nr_golden as nr
from tests import post_random as C  # noqa: E402

CUTS = sam.CUTS + nbw.CUTS + nrs.CUTS
PINS = sam.ARM + nbw.PINS + nrs.PINS + nr.PINS[1:3] + [
    ("rx/rx_sound.cpp", 908, "}"), ("rx/rx_sound.cpp", 1052, "m_Agc[rx_chan].ProcessData(ns_out, out_samps_c, out_samps_c);"),
    ("rx/CuteSDR/agc.cpp", 155, "m_WindowSamples = (int) (m_SampleRate * WINDOW_TIMECONST);"),
    ("rx/CuteSDR/agc.cpp", 158, "if(m_DelaySamples >= MAX_DELAY_BUF-1)"),
    ("rx/CuteSDR/agc.h", 16, "#define MAX_DELAY_BUF 2048")]
SAM_MACROS = ref_cut.cut_macros(sam.CUTS)


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
    for top in ("extensions", "pkgs"):
        inc += [os.path.join(R, top, d) for d in sorted(os.listdir(os.path.join(R, top))) if os.path.isdir(os.path.join(R, top, d))]
    dfn = ["-std=gnu++11", "-DKIWI", "-DKIWISDR", "-DHOST", "-DDEBIAN_VERSION=11", "-DVERSION_MAJ=1", "-DVERSION_MIN=663", "-DARCH_CPU=x86",
           "-DCPU_AM3359", "-DPLATFORM_beaglebone_black"]
    exe = os.path.join(tmp, "post_ref")
    cmd = (["g++", "-O2", "-ffp-contract=off", "-w"] + dfn + ["-I" + fftw, "-I/opt/rocm/include/hipfft", "-I/opt/rocm/include"]
           + ["-I" + d for d in inc] + ["-I" + gen, "-I" + tmp] + SAM_MACROS
           + ['-DNR_ANR_CPP="%s"' % os.path.join(R, "rx/wdsp/ANR.cpp"), '-DNB_WILD_CPP="%s"' % os.path.join(R, "rx/Teensy/NB_Wild.cpp"),
              '-DNR_SPECTRAL_CPP="%s"' % os.path.join(R, "rx/Teensy/NR_spectral.cpp"),
              "-no-pie", "-o", exe, os.path.join(ROOT, "tools", "ref", "ref_post_main.cpp")]
           + [os.path.join(R, f) for f in ("rx/CuteSDR/agc.cpp", "rx/CuteSDR/fir.cpp", "rx/CuteSDR/squelch.cpp", "rx/CuteSDR/noiseproc.cpp",
                                           "rx/csdr/ima_adpcm.cpp", "support/timing.cpp", "rx/wdsp/SAM_demod.cpp", "rx/kiwi/lms.cpp",
                                           "rx/CMSIS/arm_cfft_f32.cpp", "rx/CMSIS/arm_cfft_radix8_f32.cpp", "rx/CMSIS/arm_bitreversal2.cpp")]
           + [os.path.join(R, "rx/CMSIS", f + ".cpp") for f in nbw.CMSIS]
           + ["-L/opt/rocm/lib", "-lhipfftw", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-Wl,--unresolved-symbols=ignore-all"])
    subprocess.run(cmd, check=True)
    nrs.twiddle().tofile(os.path.join(tmp, "tw.bin"))
    return exe


def run(exe, tmp, lines, samples, full=False):
    """-> (the arrays of C.pack, exit status)"""
    P = lambda f: os.path.join(tmp, f)
    x = C.script_input(lines, samples)
    x.astype(np.float32).tofile(P("in.bin"))
    open(P("s.txt"), "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, P("s.txt"), P("in.bin"), P("tw.bin"), P("out.bin"), P("st.bin")])
    if r.returncode:
        return None, r.returncode
    return C.pack(lines, open(P("out.bin"), "rb").read(), open(P("st.bin"), "rb").read(), full), 0


def seed_features(exe, tmp, samples):
    feats = []
    for s in range(C.NSEED):
        lines = C.post_script(s)
        o, rc = run(exe, tmp, lines, samples)
        assert rc == 0, ("the harness refused a seed's script", s, rc)
        feats.append(C.features(lines, C.Record(o, "r%02d" % s, lines)))
    return feats


def search(first, count):
    samples = C.pool()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for base in range(first, first + count * 0x100, 0x100):
            C.BASE = base
            cnt, missing = C.check_conditions(seed_features(exe, tmp, samples))
            print("base 0x%08X: %s" % (base, "every condition reached" if not missing else "short of " + ", ".join("%s (%d)" % (m, cnt[m]) for m in missing)))
            sys.stdout.flush()
            if not missing:
                return base
    return None


def main():
    out = {}
    samples = C.pool()
    out["pool_sha"] = np.frombuffer(C.digest(samples.tobytes()), np.uint8)
    sc = C.all_scripts()
    feats = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        kept, packed = [], {}
        for name in sc:
            lines = sc[name]
            o, rc = run(exe, tmp, lines, samples, name in C.FULL)
            if rc:
                assert name[0] == "w" and name not in ("w1", "w256", "w2047"), ("the harness refused a script that may not be dropped", name, rc)
                print("post_rand_ref.npz: %-5s DROPPED: the harness left with status %d" % (name, rc))
                continue
            kept.append(name)
            packed[name] = o
            rec = C.Record(o, name, lines)
            ran = sorted({s for b in rec.blocks for s in b["stages"]})
            if name[0] == "r":
                feats.append(C.features(lines, rec))
            elif name[0] == "w":
                rate, W, D = C.shape_wd(name)
                assert (int(o["wd"][0]), int(o["wd"][1])) == (W, D), (name, o["wd"], W, D)
            print("post_rand_ref.npz: %-5s %6g Hz %2d blocks %5d samples, W %4d D %4d, modes %s, stages %s, changed %d, Wild hits %d"
                  % (name, float(lines[0].split()[1]), len(rec.blocks), sum(b["n"] for b in rec.blocks), o["wd"][0], o["wd"][1],
                     "/".join(sorted({C.MODE_NAMES[b["mode"]] for b in rec.blocks})), "/".join(ran) or "-", int(o["chg"].sum()),
                     int(np.maximum(o["hits"], 0).sum())))
    cnt, missing = C.check_conditions(feats)
    for c in C.CONDITIONS:
        print("  %-20s %2d seeds" % (c, cnt[c]))
    assert not missing, ("conditions reached by fewer than two seeds", missing)
    out.update(C.join(kept, packed))
    path = os.path.join(C.GOLD, C.GOLDEN)
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        a = [int(v, 0) for v in sys.argv[2:]]
        search(a[0] if a else C.BASE, a[1] if len(a) > 1 else 64)
    else:
        main()
