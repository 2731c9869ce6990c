"""Generates tests/golden/wspr_dec_ref.npz from the REFERENCE ITSELF: stage 2 of the WSPR extension (extensions/wspr/wspr.cpp, fano.cpp,
tab.cpp, metric_tables.h, wspr_util.cpp, wspr.h).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_wspr_golden.py: the line ranges are cut (each checked against its first and
last line) into a temporary directory (deleted on exit), tools/ref/ref_wspr_dec_main.cpp -- stubs of ours, none of the reference's
headers -- is compiled around them with g++ -O2 -ffp-contract=off; only data is kept.

TWO builds of the reference (stage 2, decision 1): A as it is, with the host libm's double sin / cos as the seeds of the
phase recurrences; B with sin / cos inside the cut of sync_and_demodulate defined to kg_libm::sin_f2d / cos_f2d.  The host twin
(tools/wspr_dec_host_driver.cpp) must equal build B in every field of every record and every byte of every jiggle; A against B is
measured, required to agree in every record (a seed that breaks this is replaced, not excused) and recorded; differing jiggle bytes
are capped at 1 % of a scene's bytes and 1 count each.

Checked and recorded, so that a scene cannot hide a failure: every result class is reached by at least two scenes; a decoded scene's
decdata is the encoder's; every winning ss is strictly above its runner-up in every search call (the least margin is kept); no
pre-clamp soft value lies within 1e-4 of an integer; sin_f2d / cos_f2d equal libquadmath's sinq / cosq rounded to double on every seed
argument of every scene (tools/check_wspr_dtrig.cpp does ALL floats of the domain).  The report goes to
profiles/wspr_decode_golden.txt.

    python tools/make_ref_wspr_dec_golden.py
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

import ref_cut
from ref_cut import ROOT  # ref_cut puts the repository root on sys.path
from tests import wspr_common as W1  # noqa: E402
from tests import wspr_dec_common as W  # noqa: E402

D, U, H = "extensions/wspr/wspr.cpp", "extensions/wspr/wspr_util.cpp", "extensions/wspr/wspr.h"
F, FH, T, MT = "extensions/wspr/fano.cpp", "extensions/wspr/fano.h", "extensions/wspr/tab.cpp", "extensions/wspr/metric_tables.h"

CUTS = [
    (H, "WSPR_DEC_CUT_H", 110, 332, "#define WSPR_CHECKING", "} wspr_shmem_t;"),
    (D, "WSPR_DEC_CUT_SYNC", 31, 212, "static const unsigned char pr3[NSYM_162]=", "}"),
    (D, "WSPR_DEC_CUT_TABLE", 437, 441, "// setup metric table", "}"),
    (D, "WSPR_DEC_CUT_TUNE", 505, 513, "unsigned int maxcycles=200;				//Decoder timeout limit", "int delta=60;							//Fano threshold step"),
    (D, "WSPR_DEC_CUT_CHAIN", 733, 880, "for (pki=0; pki < npk && !w->abort_decode; pki++) {", ""),
    (FH, "WSPR_DEC_CUT_FANO_H", 15, 37, "int fano(unsigned int *metric, unsigned int *cycles, unsigned int *maxnp,", "}"),
    (F, "WSPR_DEC_CUT_FANO", 21, 244, "struct node {", "}"),
    (T, "WSPR_DEC_CUT_TAB", 9, 42, "unsigned char _Partab[] = {", "};"),
    (MT, "WSPR_DEC_CUT_METRIC", 1, 138, "/*******************************************************************************", "0.00019371575,   2.80722121e-041}};"),
    (U, "WSPR_DEC_CUT_DEINT", 208, 230, "void deinterleave(unsigned char *sym)", "}"),
]
PINS = [(D, 42, "static const float DT = 1.0/FSRATE, DF = FSRATE/FSPS;"), (D, 43, "static const float TWOPIDT = 2*K_PI*DT;"),
        (D, 59, "float const DF15=DF*1.5, DF05=DF*0.5;"), (D, 88, "f0=*f1+ifreq*fstep;"), (D, 93, "fp = f0 + (drift1/2.0)*((float)i-FHSYM_81)/FHSYM_81;"),
        (D, 96, "dphi0=TWOPIDT*(fp-DF15);"), (D, 97, "cdphi0=cos(dphi0);"), (D, 98, "sdphi0=sin(dphi0);"), (D, 141, "if( (k>0) && (k<np) ) {"),
        (D, 143, "i0[i]=i0[i] + id[k]*c0[j] + qd[k]*s0[j];"), (D, 144, "q0[i]=q0[i] - id[k]*s0[j] + qd[k]*c0[j];"), (D, 155, "p0=i0[i]*i0[i] + q0[i]*q0[i];"),
        (D, 165, "totp=totp+p0+p1+p2+p3;"), (D, 167, "ss = (pr3[i] == 1) ? ss+cmet : ss-cmet;"), (D, 176, "ss=ss/totp;"), (D, 177, "if( ss > syncmax ) {"),
        (D, 198, "fac=sqrt(f2sum-fsum*fsum);"), (D, 205, "symbols[i] = fsymb[i] + 128;"), (D, 430, '#include "./metric_tables.h"'),
        (D, 431, "static int mettab[2][256];"), (D, 435, "float bias = 0.45;"), (D, 529, "#define MORE_EFFORT"), (D, 737, "u4_t decode_start = timer_ms();"),
        (D, 740, "if (ipass != 0 && p->ignore)"), (D, 807, "p->ignore = true;"), (D, 819, "while (!w->abort_decode && r_minsync1 && !r_decoded && idt <= (jig_range/iifac)) {"),
        (D, 821, "if ((idt&1) == 1) ii = -ii;"), (D, 838, "if ((sync1 > minsync2) && (rms > minrms)) {"), (D, 866, "if (w->quickmode) break;"),
        (D, 869, "bool r_timeUp = (!w->abort_decode && r_minsync1 && !r_decoded && idt > (jig_range/iifac));"), (D, 875, "p->ignore = true;"),
        (D, 881, "if (r_decoded) {"), (D, 883, "p->ignore = true;"),
        (H, 364, "#define YIELD_EVERY_N_TIMES 64"), (H, 376, "typedef enum { FIND_BEST_TIME_LAG, FIND_BEST_FREQ, CALC_SOFT_SYMS } wspr_mode_e;"),
        (F, 15, "#define	LL 1"), (F, 52, "#define	POLY1	0xf2d05351"), (F, 53, "#define	POLY2	0xe4613c47"), (F, 154, "maxcycles *= nbits;"), (F, 239, "*cycles = i+1;"),
        (F, 242, "if(i >= maxcycles) return 0;"),
        ("rx/CuteSDR/datatypes.h", 104, "#define K_PI (3.14159265358979323846)")]

SEED_CHECK = r"""
#include <quadmath.h>
#include <stdio.h>
#include <string.h>
#include "%s/flydog_sdr_gps_amd/csrc/kg_wspr_dec.h"
int main() { float d; unsigned long long n = 0, bad = 0;
  while (fread(&d, 4, 1, stdin) == 1) { double c, s; kg_wspr_df::seed_of(d, &c, &s); n++;
    const double wc = (double) cosq((__float128) (double) d), ws = (double) sinq((__float128) (double) d);
    if (memcmp(&c, &wc, 8) || memcmp(&s, &ws, 8)) bad++; }
  printf("%%llu %%llu\n", n, bad); return 0; }
"""


def build(tmp, ours):
    ref_cut.cut(tmp, CUTS, whole=True)
    ref_cut.pin(PINS, white_space_aside=True)
    pr3 = "".join(c for c in open(os.path.join(tmp, "WSPR_DEC_CUT_SYNC.inc")).read().split("=")[1].split(";")[0] if c in "01")
    assert pr3 == "".join(str(int(v)) for v in W1.PR3), "PR3"
    exe = os.path.join(tmp, "wspr_dec_ref_b" if ours else "wspr_dec_ref_a")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I" + tmp] + (["-DWSPR_DEC_OURS"] if ours else []) +
                   ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_wspr_dec_main.cpp"), "-lm"], check=True)
    return exe


def seed_arguments(recs, cands, passes):
    """every dphi the refinement calls and jiggles of a scene's records can have asked a seed for -- a superset, in float as the decoder forms them"""
    out = []
    twopidt = np.float32(2 * np.pi * float(np.float32(1.0 / 375.0)))
    df = np.float32(1.46484375)
    i = np.arange(W.NSYM)
    for ps in range(recs.shape[0]):
        for c, r in enumerate(recs[ps]):
            if r["result"] == W.SKIPPED:
                continue
            f1s = [np.float32(cands[c]["freq0"])] + [np.float32(v) for v in r["tr_f"]]
            drifts = {float(cands[c]["drift0"]), float(cands[c]["drift0"]) + 0.5, float(cands[c]["drift0"]) - 0.5}
            for f1 in f1s:
                for step in (0.25, 0.05, 0.0):
                    for ifr in range(-2, 3):
                        f0 = np.float32(f1 + np.float32(ifr * np.float32(step)))
                        for dr in drifts:
                            fp = (float(f0) + (np.float32(dr) / 2.0) * (i.astype(np.float32).astype(np.float64) - 81.0) / 81.0).astype(np.float32)
                            for off in (-df * np.float32(1.5), -df * np.float32(0.5), df * np.float32(0.5), df * np.float32(1.5)):
                                out.append((twopidt * (fp + np.float32(off))).astype(np.float32))
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.float32)


def main():
    out, report = {}, []
    say = lambda s: (print(s), report.append(s))
    names = sorted(W.SCENES)
    out["scene_names"] = np.array(names)
    reached = {}
    worst_margin, worst_int = np.inf, np.inf
    total_ab_bytes = total_jig_bytes = 0
    seeds_n = seeds_bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe_a, exe_b, twin = build(tmp, False), build(tmp, True), W.build_driver(tmp)
        chk = os.path.join(tmp, "seedchk")
        open(chk + ".cpp", "w").write(SEED_CHECK % ROOT)
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", chk, chk + ".cpp", "-lquadmath", "-lm"], check=True)
        mettab = None
        say("scene          pass  results per candidate (0 skipped 1 minsync1 2 no change 3 time up 4 decoded 5 quick miss)   A against B")
        for name in names:
            a = W.run_scene(exe_a, name, tmp)
            b = W.run_scene(exe_b, name, tmp)
            mettab = b["mettab"] if mettab is None else mettab
            assert np.array_equal(a["mettab"], mettab) and np.array_equal(b["mettab"], mettab)
            t = W.run_scene(twin, name, tmp, mettab=mettab)
            assert t["recs"].tobytes() == b["recs"].tobytes(), (name, "the twin differs from build B", [f for f in W.rec_dtype.names if not np.array_equal(t["recs"][f], b["recs"][f])])
            assert t["jig"].tobytes() == b["jig"].tobytes(), (name, "the twin's jiggle bytes differ from build B's")
            # A against B: every record field (floats by their bits), then the jiggle bytes
            same_rec = a["recs"].tobytes() == b["recs"].tobytes()
            assert same_rec, (name, "builds A and B differ in a record", [f for f in W.rec_dtype.names if not np.array_equal(a["recs"][f], b["recs"][f])])
            assert a["jig"].shape == b["jig"].shape, name
            dj = np.abs(a["jig"].astype(np.int32) - b["jig"].astype(np.int32))
            assert (dj != 0).sum() <= 0.01 * max(dj.size, 1) and (dj.max() if dj.size else 0) <= 1, (name, "jiggle bytes of A and B")
            if name in W.AB_BYTEWISE:
                assert (dj != 0).sum() == 0, (name, "A and B are compared byte for byte here")
            total_ab_bytes += int((dj != 0).sum())
            total_jig_bytes += int(dj.size)
            x, cands, passes = W.scene_inputs(name)
            k = "s_%s_" % name
            out[k + "sha"] = W.scene_sha(name)
            out[k + "recs"] = b["recs"].view(np.uint8).reshape(b["recs"].shape + (W.rec_dtype.itemsize,))
            out[k + "jig_sha"] = np.frombuffer(W.digest(b["jig"].tobytes()), np.uint8)
            out[k + "njig"] = np.array([b["jig"].shape[0]], np.int32)
            out[k + "ab"] = np.array([int((dj != 0).sum()), int(dj.size), int(dj.max() if dj.size else 0)], np.int64)
            out[k + "watch"] = t["watch"]
            for ps in range(passes.shape[0]):
                res = b["recs"][ps]["result"].tolist()
                for v in res:
                    reached.setdefault(v, set()).add(name)
                w = t["watch"][ps]
                say("%-14s %d/%d   %-40s margin %.2e  soft values off integers by %.2e   A-B bytes %d of %d" %
                    (name, passes[ps][0], passes[ps][1], res, w["least"], w["int_dist"], int((dj != 0).sum()), dj.size))
                assert w["strict"] == 1, (name, "a winning ss is not above its runner-up")
                worst_margin = min(worst_margin, float(w["least"]))
                if name in W.AB_BYTEWISE and np.isfinite(w["int_dist"]):
                    assert w["int_dist"] >= 1e-4, (name, "a pre-clamp soft value within 1e-4 of an integer", float(w["int_dist"]))
                    worst_int = min(worst_int, float(w["int_dist"]))
            # a decoded candidate's data is the encoder's
            for ps in range(passes.shape[0]):
                for c, r in enumerate(b["recs"][ps]):
                    if r["result"] == W.DECODED:
                        want = [W.channel_symbols(s[4])[1] for s in W.SCENES[name]["signals"]]
                        assert bytes(r["decdata"][:10]) in want, (name, ps, c, "decoded something that was not sent")
            args = seed_arguments(b["recs"], cands, passes)
            n, bad = (int(v) for v in subprocess.run([chk], input=args.astype(np.float32).tobytes(), capture_output=True, check=True).stdout.split())
            seeds_n += n
            seeds_bad += bad
        for cls in (W.SKIPPED, W.MINSYNC1, W.NO_CHANGE, W.TIME_UP, W.DECODED, W.QUICK_MISS):
            say("result class %d reached by %d scenes: %s" % (cls, len(reached.get(cls, ())), " ".join(sorted(reached.get(cls, ())))))
            assert len(reached.get(cls, ())) >= (1 if cls == W.QUICK_MISS else 2), cls
        assert seeds_bad == 0, "a seed argument on which sin_f2d / cos_f2d is not the correctly rounded value"
        say("seed arguments checked against sinq / cosq: %d, differing: %d" % (seeds_n, seeds_bad))
        say("A against B over all scenes: records equal in every field and float bit; %d of %d jiggle bytes differ" % (total_ab_bytes, total_jig_bytes))
        say("least margin of a winning ss over its runner-up: %.3e (relative); least distance of a pre-clamp soft value from an integer: %.3e" % (worst_margin, worst_int))
        # fano alone, from the reference's own fano (build A: no seeds involved)
        fs = W.fano_sets()
        out["fano_names"] = np.array(sorted(fs))
        for n in sorted(fs):
            sy, mc = fs[n]
            W.table_file(mettab, tmp)
            sy.tofile(os.path.join(tmp, "syms.bin"))
            subprocess.run([exe_a, "-f", os.path.join(tmp, "syms.bin"), "1", str(mc), os.path.join(tmp, "fano_ref.bin")], check=True)
            want = np.fromfile(os.path.join(tmp, "fano_ref.bin"), W.fano_dtype)
            got = W.run_fano(twin, sy, mc, mettab, tmp)
            assert got.tobytes() == want.tobytes(), (n, got, want)
            out["f_%s" % n] = want.view(np.uint8).copy()
            out["f_%s_sha" % n] = np.frombuffer(W.digest(sy.tobytes() + bytes([mc & 255, mc >> 8])), np.uint8)
            say("fano %-11s maxcycles %4d: ok %d metric %d cycles %d maxnp %d" % (n, mc, want["ok"][0], want["metric"][0], want["cycles"][0], want["maxnp"][0]))
        out["mettab"] = mettab.astype(np.int32)
        out["cond"] = np.array([worst_margin, worst_int], np.float64)
        out["ab_total"] = np.array([total_ab_bytes, total_jig_bytes, seeds_n, seeds_bad], np.int64)
        path = os.path.join(tmp, "wspr_dec_ref.npz")
        np.savez_compressed(path, **out)
        W.golden_conditions(np.load(path), os.path.getsize(path))
        final = os.path.join(W.GOLD, "wspr_dec_ref.npz")
        shutil.copyfile(path, final)
    say("wrote tests/golden/wspr_dec_ref.npz, %d bytes" % os.path.getsize(final))
    if "--report" in sys.argv:
        open(os.path.join(ROOT, "profiles", "wspr_decode_golden_scenes.txt"), "w").write("\n".join(report) + "\n")


if __name__ == "__main__":
    main()
