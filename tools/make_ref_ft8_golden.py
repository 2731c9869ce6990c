"""Generates tests/golden/ft8_ref.npz from the REFERENCE ITSELF: stage 1 of the FT8 / FT4 extension (extensions/FT8/ft8_lib:
decode_ft8.c, common/monitor.c, ft8/decode.c).

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  Same construction as tools/make_ref_wspr_golden.py: the line ranges are cut (each checked against its first and
last line, and a table of pinned statements) into a temporary directory (deleted on exit), tools/ref/ref_ft8_main.cpp -- stubs of ours
-- is compiled around them with g++ -O2 -ffp-contract=off; the reference's headers, its kiss_fft and its constants are read and compiled
in place; only data is kept.

The monitor is built TWICE: build A with the reference's own kiss_fftr, build B with an independent double-precision DFT rounded to
float (tools/ref/ft8_harness.h).  Per stream scene n_AB -- the waterfall bytes in which A and B differ --, the largest difference and
|max_mag_A - max_mag_B| are recorded; every difference must be 1 and n_AB at most 0.1 % of the scene's bytes.  The host twin
(tools/ft8_host_driver.cpp) is built twice too: with kiss_fftr it must write build A's records BYTE FOR BYTE (schedule, events, waterfall
bytes, max_mag, candidates, log174, end state), with the double DFT build B's.  The golden keeps build A's bytes (what the device is
measured against) and build B's records (what the CPU suite's twin, which has no kiss_fft, must equal).

    python tools/make_ref_ft8_golden.py          (writes profiles/ft8_golden.txt too)
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ref_cut
from ref_cut import ROOT, R  # ref_cut puts the repository root on sys.path
from tests import ft8_common as F  # noqa: E402

LIB = "extensions/FT8/ft8_lib"
D, M, C = LIB + "/decode_ft8.c", LIB + "/common/monitor.c", LIB + "/ft8/decode.c"
K, KC, H = LIB + "/ft8/constants.h", LIB + "/ft8/constants.c", LIB + "/ft8/decode.h"

# file, name, first line, last line, text of the first, text of the last
CUTS = [
    ("extensions/FT8/FT8.h", "FT8_CUT_PASSBAND", 8, 9, "#define FT8_PASSBAND_LO     100", "#define FT8_PASSBAND_HI     3100"),
    (M, "FT8_CUT_HANN", 9, 13, "static float hann_i(int i, int N)", "}"),
    (M, "FT8_CUT_WFALL", 37, 53, "static void waterfall_init(", "}"),
    (M, "FT8_CUT_MON", 55, 203, "void monitor_init(monitor_t* me, const monitor_config_t* cfg)", "}"),
    (C, "FT8_CUT_CANDMAG", 54, 61, "static const WF_ELEM_T* get_cand_mag(", "}"),
    (C, "FT8_CUT_SCORE", 63, 190, "static int ft8_sync_score(", "}"),
    (C, "FT8_CUT_FIND", 192, 254, "int ftx_find_candidates(", "}"),
    (C, "FT8_CUT_LIKE", 256, 328, "static void ft4_extract_likelihood(", "}"),
    (C, "FT8_CUT_L174", 332, 342, "float log174[FTX_LDPC_N];", "ftx_normalize_logl(log174);"),
    (C, "FT8_CUT_MAX", 393, 401, "static float max2(float a, float b)", "}"),
    (C, "FT8_CUT_HEAPS", 403, 454, "static void heapify_down(", "}"),
    (C, "FT8_CUT_SYM4", 457, 469, "static void ft4_extract_symbol(", "}"),
    (C, "FT8_CUT_SYM8", 472, 511, "static void ft8_extract_symbol(", "}"),
    (D, "FT8_CUT_STRUCT", 37, 69, "typedef struct {", "} decode_ft8_t;"),
    (D, "FT8_CUT_ARRAY", 71, 71, "static decode_ft8_t decode_ft8[MAX_RX_CHANS];", "static decode_ft8_t decode_ft8[MAX_RX_CHANS];"),
    (D, "FT8_CUT_CONSTS", 73, 80, "const int kMin_score = 10;", "const int kTime_osr = 2;"),
    (D, "FT8_CUT_FREQ", 229, 230, "float freq_hz = (mon->min_bin + cand->freq_offset + (float)cand->freq_sub / wf->freq_osr) / mon->symbol_period;",
     "float time_sec = (cand->time_offset + (float)cand->time_sub / wf->time_osr) * mon->symbol_period;"),
    (D, "FT8_CUT_SNR", 303, 303, "float snr = cand->score * 0.5f + ft8_conf.SNR_adj;", "float snr = cand->score * 0.5f + ft8_conf.SNR_adj;"),
    (D, "FT8_CUT_SAMPLES", 503, 559, "void decode_ft8_samples(int rx_chan, TYPEMONO16 *samps, int nsamps, int freqHz, u1_t *start_test)", "}"),
    (D, "FT8_CUT_INIT", 561, 617, "void decode_ft8_init(int rx_chan, int proto)", "}"),
]
PINS = [("extensions/FT8/FT8.h", 8, "#define FT8_PASSBAND_LO     100"), ("extensions/FT8/FT8.h", 9, "#define FT8_PASSBAND_HI     3100"),
        ("extensions/FT8/FT8.cpp", 312, 'ft8_conf.SNR_adj = cfg_default_int("ft8.SNR_adj", -22, &update_cfg);'),
        (D, 74, "const int kMax_candidates = 140;"), (D, 79, "const int kFreq_osr = 2;"),
        (D, 510, "const float time_shift = 0.8;"), (D, 514, "double time_within_slot = fmod(time_sec - time_shift, ft8->slot_period);"),
        (D, 515, "if (time_within_slot > ft8->slot_period / 4) {"), (D, 524, "ft8->in_pos = ft8->frame_pos = 0;"), (D, 527, "ft8->slot++;"),
        (D, 531, "for (int i = 0; i < nsamps /*&& ft8->in_pos < ft8->num_samples*/; i++) {"), (D, 533, "ft8->samples[ft8->in_pos] = ((TYPEREAL) samps[i]) / 32768.0f;"),
        (D, 541, "while (ft8->in_pos >= ft8->frame_pos + block_size && ft8->frame_pos < ft8->num_samples) {"), (D, 545, "if (ft8->frame_pos < ft8->num_samples)"),
        (D, 557, "monitor_reset(&ft8->mon);"), (D, 558, "ft8->tsync = false;"), (D, 577, "num_samples = (slot_period - 0.4f) * sample_rate;"),
        (M, 11, "float x = sinf((float)M_PI * i / N);"), (M, 60, "me->block_size = (int)(cfg->sample_rate * symbol_period);"), (M, 63, "me->fft_norm = 2.0f / me->nfft;"),
        (M, 70, "me->window[i] = me->fft_norm * hann_i(i, me->nfft);"), (M, 75, "me->last_frame = (float*)calloc(me->nfft, sizeof(me->last_frame[0]));"),
        (M, 136, "me->wf.num_blocks = 0;"), (M, 137, "me->max_mag = -120.0f;"), (M, 170, "me->timedata[pos] = me->window[pos] * me->last_frame[pos];"),
        (M, 172, "kiss_fftr(me->fft_cfg, me->timedata, me->freqdata);"), (M, 181, "float db = 10.0f * log10f(1E-12f + mag2);"),
        (M, 191, "int scaled = (int)(2 * db + 240);"), (M, 196, "if (db > me->max_mag)"),
        (C, 79, "if (block_abs < 0)"), (C, 81, "if (block_abs >= wf->num_blocks)"), (C, 124, "score /= num_average;"),
        (C, 208, "for (candidate.time_offset = -10; candidate.time_offset < 20; ++candidate.time_offset)"), (C, 214, "if (candidate.score < min_score)"),
        (C, 219, "if ((heap_size == num_candidates) && (candidate.score > heap[0].score))"), (C, 323, "float norm_factor = sqrtf(24.0f / variance);"),
        (C, 395, "return (a >= b) ? a : b;"),
        (H, 28, "#define WF_ELEM_T          uint8_t"), (H, 29, "#define WF_ELEM_MAG(x)     ((float)(x)*0.5f - 120.0f)"), (H, 21, "// #define WATERFALL_USE_PHASE"),
        (K, 11, "#define FT8_SYMBOL_PERIOD (0.160f)"), (K, 12, "#define FT8_SLOT_TIME     (15.0f)"), (K, 14, "#define FT4_SYMBOL_PERIOD (0.048f)"),
        (K, 15, "#define FT4_SLOT_TIME     (7.5f)"), (K, 42, "#define FTX_LDPC_N       (174)"),
        (KC, 4, "const uint8_t kFT8_Costas_pattern[7] = { 3, 1, 4, 0, 6, 5, 2 };"), (KC, 13, "const uint8_t kFT8_Gray_map[8] = { 0, 1, 3, 2, 5, 6, 4, 7 };"),
        (KC, 14, "const uint8_t kFT4_Gray_map[4] = { 0, 1, 3, 2 };"), (KC, 6, "{ 0, 1, 3, 2 },"), (KC, 9, "{ 3, 2, 0, 1 }")]


def build(tmp):
    """-> (build A, build B, the twin with kiss_fftr, the twin with the double DFT)"""
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS, white_space_aside=True)
    lib = os.path.join(R, LIB)
    objs = []
    for src in ("fft/kiss_fft.c", "fft/kiss_fftr.c", "ft8/constants.c"):
        o = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-w", "-I" + lib, "-I" + os.path.join(lib, "fft"), "-c", os.path.join(lib, src), "-o", o], check=True)
        objs.append(o)
    exes = []
    for name, extra in (("ft8_ref_a", []), ("ft8_ref_b", ["-DFT8_DFT_DOUBLE"])):
        exe = os.path.join(tmp, name)
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-ffp-contract=off", "-w", "-I" + tmp, "-I" + lib, "-I" + os.path.join(ROOT, "tools", "ref")] + ref_cut.cut_macros(CUTS) + extra +
                       ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_ft8_main.cpp")] + objs + ["-lm"], check=True)
        exes.append(exe)
    twin_a = os.path.join(tmp, "ft8_twin_a")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-DFT8_USE_KISS", "-I" + lib, "-o", twin_a, os.path.join(ROOT, "tools", "ft8_host_driver.cpp")] + objs[:2] + ["-lm"], check=True)
    return exes[0], exes[1], twin_a, F.build_driver(tmp)


def run_raw(exe, scene, tmp):
    sp, op = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
    open(sp, "wb").write(scene)
    subprocess.run([exe, sp, op], check=True)
    return open(op, "rb").read()


def main():
    out, lines = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        ref_a, ref_b, twin_a, twin_b = build(tmp)
        out["load_names"] = np.array(sorted(F.LOADS))
        out["stream_names"] = np.array(sorted(F.STREAMS))
        for name in sorted(F.LOADS):
            p, kw, ncand, min_score = F.LOADS[name]
            scene = F.scene_bytes(name)
            raw = run_raw(ref_a, scene, tmp)
            assert raw == run_raw(twin_b, scene, tmp), (name, "the twin's records are not the reference's")
            got = F.parse(raw)
            sz, sl = got["sizes"], got["slots"][0]
            k = "l_%s_" % name
            out[k + "sha"] = np.frombuffer(F.digest(scene), np.uint8)
            for key, v in F.slot_golden(sl, F.LDPC_N if name == F.FULL_LOG else F.KEEP).items():
                out[k + key] = v
            # how many pass: the reference run again with one candidate slot per hypothesis is not possible (the list is 140 at most), so
            # count with the scores themselves: every hypothesis is a candidate of a waterfall search with min_score at its own score
            mag = F.waterfall(p, **kw)
            npass = count_passing(p, mag, min_score)
            ntie = int((sl["cand"]["score"] == sl["cand"]["score"][-1]).sum()) if sl["ncand"] else 0
            out[k + "npass"] = np.array([npass], np.int32)
            out[k + "ntie_min"] = np.array([ntie], np.int32)
            lines.append("   %-16s num_blocks %2d  num_candidates %3d  min_score %3d: %5d pass, %3d kept, %3d share the lowest kept score" %
                         (name, mag.shape[0], ncand, min_score, npass, sl["ncand"], ntie))
        for name in sorted(F.STREAMS):
            p, make = F.STREAMS[name]
            scene = F.scene_bytes(name)
            raw_a, raw_b = run_raw(ref_a, scene, tmp), run_raw(ref_b, scene, tmp)
            assert raw_a == run_raw(twin_a, scene, tmp), (name, "the twin on kiss_fftr does not write build A's records")
            assert raw_b == run_raw(twin_b, scene, tmp), (name, "the twin on the double DFT does not write build B's records")
            a, b = F.parse(raw_a), F.parse(raw_b)
            pn = F.pname(p)
            sz = a["sizes"]
            if "sizes_" + pn not in out:
                full = [e for e in a["events"] if e[1] == 1]
                if full:
                    out["sizes_" + pn] = np.array([sz[f] for f in ("block", "nfft", "num_bins", "min_bin", "max_blocks", "num_samples", "block_stride", "subblock")] + [full[0][2]],
                                                  np.int32)
                    out["window_" + pn] = a["window"]
            assert a["events"] == b["events"] and np.array_equal(a["end"]["state"], b["end"]["state"]) and len(a["slots"]) == len(b["slots"]) <= 1
            assert a["end"]["last_frame"].tobytes() == b["end"]["last_frame"].tobytes()
            k = "s_%s_" % name
            out[k + "sha"] = np.frombuffer(F.digest(scene), np.uint8)
            out[k + "events"] = np.array(a["events"], np.int64).reshape(-1, 5)
            out[k + "state"] = a["end"]["state"]
            out[k + "last_frame_sha"] = np.frombuffer(F.digest(a["end"]["last_frame"].tobytes()), np.uint8)
            mags_a = [s["mag"] for s in a["slots"]] + [a["end"]["mag"]]
            mags_b = [s["mag"] for s in b["slots"]] + [b["end"]["mag"]]
            all_a, all_b = np.concatenate(mags_a).astype(np.int32), np.concatenate(mags_b).astype(np.int32)
            d = np.abs(all_a - all_b)
            mm_a = np.array([s["max_mag"] for s in a["slots"]] + [a["end"]["max_mag"]], np.float32)
            mm_b = np.array([s["max_mag"] for s in b["slots"]] + [b["end"]["max_mag"]], np.float32)
            out[k + "n_ab"] = np.array([(d != 0).sum()], np.int32)
            out[k + "nbytes"] = np.array([d.size], np.int32)
            out[k + "ab_max"] = np.array([d.max() if d.size else 0], np.int32)
            out[k + "max_mag_a"], out[k + "max_mag_b"] = mm_a, mm_b
            out[k + "max_mag_ab"] = np.array([np.abs(mm_a.astype(np.float64) - mm_b.astype(np.float64)).max()], np.float64)
            # build A's bytes of the slot under way at the end, and where build B's differ
            ea, eb = a["end"]["mag"], b["end"]["mag"]
            out[k + "end_mag"] = ea
            out[k + "end_ab_idx"] = np.flatnonzero(ea != eb).astype(np.int32)
            out[k + "end_ab_val"] = eb[ea != eb]
            n_kept = int((ea != eb).sum())
            if a["slots"]:
                sa, sb = a["slots"][0], b["slots"][0]
                tail = F.TAIL_BLOCKS * sz["block_stride"]
                out[k + "tail_mag"] = sa["mag"][-tail:]
                n_kept += int((sa["mag"][-tail:] != sb["mag"][-tail:]).sum())
                out[k + "slot_mag_sha_b"] = np.frombuffer(F.digest(sb["mag"].tobytes()), np.uint8)
                for key, v in F.slot_golden(sb, F.KEEP).items():
                    out[k + "b_" + key] = v
                out[k + "a_cand"] = sa["cand"]
            out[k + "n_ab_kept"] = np.array([n_kept], np.int32)
            assert d.max(initial=0) <= 1, (name, "a byte of builds A and B differs by more than 1")
            assert (d != 0).sum() <= 0.001 * d.size, (name, "builds A and B differ in %d of %d bytes" % ((d != 0).sum(), d.size))
            lines.append("   %-16s %7d bytes: n_AB %3d (%.4f %%), largest difference %d, |max_mag_A - max_mag_B| %.3g dB; %d in the bytes kept; %d slot end(s)%s" %
                         (name, d.size, (d != 0).sum(), 100.0 * (d != 0).mean() if d.size else 0.0, d.max(initial=0), float(out[k + "max_mag_ab"][0]), n_kept, len(a["slots"]),
                          ", %d candidates (A), %d (B)" % (a["slots"][0]["ncand"], b["slots"][0]["ncand"]) if a["slots"] else ""))
        path = os.path.join(tmp, "ft8_ref.npz")
        np.savez_compressed(path, **out)
        F.golden_conditions(np.load(path), os.path.getsize(path))
        final = os.path.join(F.GOLD, "ft8_ref.npz")
        shutil.copyfile(path, final)
    size = os.path.getsize(final)
    print("\n".join(lines))
    print("wrote %s, %d bytes" % (final, size))
    return lines, size


def count_passing(p, mag, min_score):
    """the hypotheses with score >= min_score, by an integer model of decode.c:63-190 of this maker's own (vectorised over freq_offset):
    used for the golden's recorded counts alone, never for an expected record"""
    nb_blocks, nbins = mag.shape[0], mag.shape[3]
    tones = 4 if p == F.FT4 else 8
    length = 4 if p == F.FT4 else 7
    nfo = nbins - tones + 1
    m32 = mag.astype(np.int32)
    total = 0
    for ts in range(2):
        for fs in range(2):
            for to in range(-10, 20):
                score, navg = np.zeros(nfo, np.int64), 0
                stop_group = None
                for idx, (blk, sm) in enumerate(F.sync_blocks(p)):
                    g, kk = divmod(idx, length)
                    if stop_group == g:
                        continue
                    ba = to + blk
                    if ba < 0:
                        continue
                    if ba >= nb_blocks:
                        stop_group = g
                        continue
                    row = m32[ba, ts, fs]
                    cen = row[sm:sm + nfo]
                    if sm > 0:
                        score += cen - row[sm - 1:sm - 1 + nfo]; navg += 1
                    if sm < tones - 1:
                        score += cen - row[sm + 1:sm + 1 + nfo]; navg += 1
                    if kk > 0 and ba > 0:
                        score += cen - m32[ba - 1, ts, fs][sm:sm + nfo]; navg += 1
                    if kk + 1 < length and ba + 1 < nb_blocks:
                        score += cen - m32[ba + 1, ts, fs][sm:sm + nfo]; navg += 1
                if navg:
                    score = np.sign(score) * (np.abs(score) // navg)
                total += int((score >= min_score).sum())
    return total


if __name__ == "__main__":
    lines, size = main()
    path = os.path.join(ROOT, "profiles", "ft8_golden.txt")
    old = open(path).read() if os.path.exists(path) else ""
    mark = "\nKernels of csrc/kg_ft8.hip"                    # the kernels' resource table below the scenes is kept as it stands
    kept = old[old.index(mark):] if mark in old else ""
    with open(path, "w") as f:
        f.write("tests/golden/ft8_ref.npz as tools/make_ref_ft8_golden.py made it (%d bytes).  Build A: the reference's kiss_fftr; build B: the double-precision\n"
                "DFT rounded to float.  The host twin wrote build A's records byte for byte on kiss_fftr and build B's on the double DFT, in every scene.\n\n" % size)
        f.write("\n".join(lines) + "\n")
        f.write(kept)
