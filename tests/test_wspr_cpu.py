"""kg_wspr.h, stage 1 of the WSPR extension (extensions/wspr/) as kg_wspr's kernels and host schedule run it, compiled for the host with
g++ -O2 -ffp-contract=off in the driver tools/wspr_host_driver.cpp, against tests/golden/wspr_ref.npz (made by
tools/make_ref_wspr_golden.py from the reference's own statements).  With the golden's own stand-in for FFTW as the transform, the host
model equals the reference in every record: the status changes, every row, the end state, pwr_sampavg, the planes by digest, and --
from the planes -- every peak and candidate bit for bit.  Then the rows from the golden's savg, the conditions the golden must meet,
the refusals, and the prototypes.  Every comparison is an equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from . import wspr_common as W

ROOT = W.ROOT
WSPR_SYMBOLS = {
    "kg_wspr_create": ("int kg_wspr_create(kg_ctx *ctx, int nconn, kg_wspr **out);", 3),
    "kg_wspr_destroy": ("void kg_wspr_destroy(kg_wspr *q);", 1),
    "kg_wspr_init": ("int kg_wspr_init(kg_wspr *q, int conn, double snd_rate);", 3),
    "kg_wspr_set_capture": ("int kg_wspr_set_capture(kg_wspr *q, int conn, int capture);", 3),
    "kg_wspr_set_type": ("int kg_wspr_set_type(kg_wspr *q, int conn, int type);", 3),
    "kg_wspr_set_more_candidates": ("int kg_wspr_set_more_candidates(kg_wspr *q, int conn, int on);", 3),
    "kg_wspr_push": ("int kg_wspr_push(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride, const int32_t *minute,", 20),
    "kg_wspr_plan": ("int kg_wspr_plan(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const int32_t *minute, const int32_t *second, size_t time_stride,", 12),
    "kg_wspr_state": ("int kg_wspr_state(kg_wspr *q, int conn, kg_wspr_info *info, float *pwr_sampavg, float *pwr_samp, float *iq_data);", 6),
    "kg_wspr_load": ("int kg_wspr_load(kg_wspr *q, int conn, int half, const float *pwr_samp, const float *pwr_sampavg, kg_wspr_cycle *cycle);", 6),
}
BANK = ("_init", "_set_capture", "_set_type", "_set_more_candidates", "_set_now", "", "_out")


@pytest.fixture(scope="module")
def golden():
    return W.load()


@pytest.fixture(scope="module")
def pool():
    return W.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return W.build_driver(tmp_path_factory.mktemp("wspr"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded samples and the scripts are the ones the reference binary was fed"""
    assert W.digest(pool.tobytes()) == bytes(golden["pool_sha"])
    sc = W.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert W.digest("\n".join(lines).encode()) == bytes(golden["s_%s_script_sha" % k]), k


@pytest.mark.parametrize("name", sorted(W.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name):
    """schedule and events, rows, state, pwr_sampavg, the planes' digests, peaks and candidates: equal"""
    got = W.golden_of(W.run_script_exe(driver, W.scripts()[name], pool, tmp_path))
    for key, v in got.items():
        if key != "cond":
            want = golden["s_%s_%s" % (name, key)]
            assert v.dtype == want.dtype and v.tobytes() == want.tobytes(), (name, key)


def test_rows_from_the_goldens_savg(golden, tmp_path):
    """kg_wspr.h's row_of on the savg the reference had: the row byte for byte (through a driver of three lines around the header)"""
    src = tmp_path / "row.cpp"
    src.write_text('#include "%s/flydog_sdr_gps_amd/csrc/kg_wspr.h"\n#include <stdio.h>\nint main(int c, char **v) { float s[512]; unsigned char w[412]; int t, f;\n'
                   'while (fread(&t, 4, 1, stdin) == 1 && fread(&f, 4, 1, stdin) == 1 && fread(s, 4, 512, stdin) == 512) { kg_wspr_cf::row_of(s, t, f, w); fwrite(w, 1, 412, stdout); }\n'
                   'return 0; }\n' % ROOT)
    exe = str(tmp_path / "row")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, str(src), "-lm"], check=True)
    n = 0
    for name in W.scripts():
        k = "s_%s_" % name
        typ = int(golden[k + "info"][14])
        for r, savg in zip(golden[k + "savg_rows"], golden[k + "savg"]):
            inp = np.array([typ, golden[k + "meta"][r][3]], np.int32).tobytes() + savg.astype(np.float32).tobytes()
            out = subprocess.run([exe], input=inp, capture_output=True, check=True).stdout
            assert out == golden[k + "rows"][r].tobytes(), (name, int(r))
            n += 1
    assert n >= 12


def golden_conditions(g, size):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    sc = W.scripts()
    C = lambda name: [W.cycle_fields(c) for c in g["s_%s_cyc" % name]]
    f32 = lambda a: np.ascontiguousarray(a, np.int32).view(np.float32)
    assert {"load_" + n for n in W.LOADS} <= set(sc) and set(W.E2E) <= set(sc)
    for name in sc:
        cond = g["s_%s_cond" % name]
        assert (cond[:, :3] == 1).all(), name                           # no ties in snr0, log10 off the float ties, winners above their runners-up
        if name in W.E2E:
            assert cond.shape[0] >= 1 and (f32(cond[:, 3]) >= 1e-3).all(), name
    # the `_load` cases reach what they are named for (a planted pattern's peak is its bin or a neighbour: the 7-bin sums are symmetric)
    def won_near(cand, npk, b):
        hit = [c for c in cand[:npk] if abs(int(c[5]) - b) <= 1]
        assert hit, (b, cand[:npk, 5].tolist())
        return int(hit[0][1]), float(f32(hit[0][2:3])[0])
    (_, _, npk, pk, cand), = C("load_planted3")
    assert 3 <= npk < 12 and won_near(cand, npk, 150) == (128 * 1, 0.0) and won_near(cand, npk, 233) == (128 * 6, -3.0) and won_near(cand, npk, 301) == (128 * -3, 4.0)
    (_, _, npk, pk, cand), = C("load_edges")
    assert pk[0, 0] == 55 and f32(pk[0, 1:2])[0] == np.float32(-150 * W.DF2) and abs(f32(pk[0, 1:2])[0]) <= 110          # the last bin inside FMIN
    assert pk[npk - 1, 0] in (354, 355) and won_near(cand, npk, 55)[1] == 1.0 and won_near(cand, npk, 355)[1] == -1.0
    (_, _, npk, pk, cand), = C("load_lags")
    assert won_near(cand, npk, 120)[0] == 128 * -9 and won_near(cand, npk, 290)[0] == 128 * 22                            # k0 -10: kindex below 0; k0 21: kindex reaches 343
    assert C("load_many")[0][2] == 12 and C("load_flat")[0][2] == 0
    (_, _, npk, pk, cand), = C("load_more")
    assert npk >= 8 and (cand[:npk, 5] % 2 == 0).all() and (np.diff(np.sort(cand[:npk, 5])) == 2).any()                   # every second bin: neighbours among them
    (_, _, npk, pk, cand), = C("load_power0")
    hole = [c for c in cand[:npk] if c[5] == 260]
    assert npk >= 2 and len(hole) == 1 and hole[0][1] == 0 and hole[0][2] == 0 and hole[0][3] == 0                        # no hypothesis won: the zeros of the memset
    assert f32(hole[0][0:1])[0] == np.float32(55 * W.DF2)                                                                 # and freq0 as the peak list left it
    assert g["s_load_type15_info"][14] == 15
    # the pushed scenes: a cycle end each, the signals found where they were put, rows with the sync flag, silence without peaks
    (_, _, npk, pk, cand), = C("e2e_a")
    assert npk >= 1 and abs(float(f32(cand[0, 0:1])[0]) - 20.0) < 1.5 and cand[0, 1] == 128 * 6 and f32(cand[0, 2:3])[0] == 0.0     # 750 samples: shift0 768 is the nearest
    (_, _, npk, pk, cand), = C("resync")
    f0 = sorted(float(v) for v in f32(cand[:2, 0]))
    assert abs(f0[0] + 61.0) < 1.5 and abs(f0[1] - 47.5) < 1.5
    assert g["s_resync_ev"][:, 1].tolist() == [W.IDLE, W.SYNC, W.RUNNING, W.DECODING, W.RUNNING]
    assert g["s_e2e_a_ev"][:, 1].tolist() == [W.IDLE, W.SYNC, W.RUNNING, W.DECODING, W.RUNNING, W.RUNNING]                         # and the next cycle's sync
    m = g["s_e2e_a_meta"]
    assert m.shape[0] >= 86 and m[0].tolist()[1:] == [0, 1, 1] and (m[1:86, 3] == 0).all() and m[85][1] == 85
    assert C("silence")[0][2] == 0 and (g["s_silence_rows"][:, 1:] == 0).all()
    e = g["s_edges_sched_meta"]
    blk, cnt = np.unique(e[:, 0], return_counts=True)
    assert cnt.max() >= 2 and len(C("edges_sched")) == 1 and g["s_edges_sched_info"][8] > 0                   # two groups in one callback; a cycle end; a cycle under way
    assert (e[:, 3] == 0).sum() >= 86 and set(e[:, 2].tolist()) == {0, 1}                                      # free-running groups; both halves
    for name in sc:
        if not name.startswith("load_"):
            d, mx = g["s_%s_rows32_diff" % name], g["s_%s_rows32_max" % name]
            assert d.sum() < 0.02 * 411 * max(d.size, 1) and (mx <= 1).all(), name
    assert size <= 400 * 1024


def test_golden_file_meets_its_conditions(golden):
    golden_conditions(golden, os.path.getsize(os.path.join(W.GOLD, "wspr_ref.npz")))


REFUSALS = {
    "rate_374": (["I 374.9"], 11),
    "rate_nan": (["I nan"], 11),
    "rate_inf": (["I inf"], 11),
    "type_3": (["I 375", "Y 3"], 12),
    "minute_60": (["I 375", "C 1", "B 0 512 60 0"], 13),
    "second_60": (["I 375", "C 1", "B 0 512 0 60"], 13),
    "second_negative": (["I 375", "C 1", "B 0 512 0 -1"], 13),
    "push_before_init": (["B 0 512 0 0"], 14),
    "capture_before_init": (["C 1"], 14),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    W.run_script_exe(driver, lines, pool, tmp_path, expect=status)


def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path):
    got = W.run_script_exe(driver, ["I 375", "Y 15", "Y 2", "C 1", "B 0 512 59 59", "B 512 512 0 0"], pool, tmp_path)
    assert got["info"][16] == 1 and got["info"][8] == 512 and got["ev"][:, 1].tolist() == [W.IDLE, W.SYNC, W.RUNNING]
    got = W.run_script_exe(driver, ["I 749.9", "C 1", "B 0 512 1 0"], pool, tmp_path)
    assert got["info"][16] == 1 and got["info"][8] == 512
    got = W.run_script_exe(driver, ["I 12000", "C 1", "B 0 512 1 0"], pool, tmp_path)
    assert got["info"][16] == 32 and got["info"][8] == 16


def test_wspr_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, wspr
    import flydog_sdr_gps_amd
    assert flydog_sdr_gps_amd.Wspr is wspr.Wspr
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in WSPR_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    protos = re.findall(r"\b(kg_wspr\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert len(protos) == len(WSPR_SYMBOLS)
    for n, a in protos:
        assert not re.search(r"\bvoid\s*\*", a), (n, "every pointer is typed")
        assert not re.search(r"(?<!\*)\*\s*d_\w+", a), (n, "no parameter is a single pointer named d_...")
        assert len(a.split(",")) == WSPR_SYMBOLS[n][1], n
    bank = dict(re.findall(r"\b(kg_rxbank_wspr\w*)\s*\(([^;{}()]*)\)\s*;", bare))
    assert sorted(bank) == sorted("kg_rxbank_wspr" + s for s in BANK)
    for s, args in bank.items():
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == len(args.split(",")) and hasattr(lib, s), s
        assert not re.search(r"\bvoid\s*\*", args) and not re.search(r"(?<!\*)\*\s*d_\w+", args), s       # the bank hands its buffers out
    assert re.search(r"uint8_t \*\*d_rows, kg_wspr_cycle \*\*d_cycles, int32_t \*\*d_counts", bank["kg_rxbank_wspr_out"])
    for s in list(WSPR_SYMBOLS) + list(bank):                              # every prototype cites the reference lines it replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void|kg_wspr \*)\s*\*?%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    d = {k: int(v) for k, v in re.findall(r"#define KG_WSPR_(\w+)\s+(\d+)", header)}
    assert (d["NBINS"], d["NFFT"], d["NT"], d["TPOINTS"], d["MAX_NPK"], d["ROW_STRIDE"]) == (wspr.NBINS, wspr.NFFT, wspr.NT, wspr.TPOINTS, wspr.MAX_NPK, wspr.ROW_STRIDE)
    assert (wspr.NBINS, wspr.NFFT, wspr.NT, wspr.TPOINTS, wspr.MAX_NPK) == (W.NBINS, W.NFFT, W.NT, W.TPOINTS, W.MAX_NPK)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_wspr.h")).read()
    pr3 = re.search(r"#define KG_WSPR_PR3\s*\\\s*\{([^}]*)\}", src).group(1)
    assert "".join(c for c in pr3 if c in "01") == "".join(str(int(v)) for v in W.PR3)


def test_messages_format():
    from flydog_sdr_gps_amd import wspr
    ev = np.zeros(2, wspr.ev_dtype)
    ev[0] = (0, -1, 0, wspr.EV_STATUS, wspr.SYNC, wspr.RUNNING)
    ev[1] = (0, 3, 5, wspr.EV_PEAKS, 1, 0)
    cy = np.zeros(1, wspr.cycle_dtype)
    cy[0]["npk"] = 2
    cy[0]["pk"][0] = (150, -40.3, -20.5, 0)
    cy[0]["pk"][1] = (233, 20.5, -7.49, 0)
    assert wspr.messages(ev, cy, now=(1700000000, 250)) == [(0, "EXT WSPR_STATUS=2 WSPR_TIME_MSEC=1700000000=250"), (0, "EXT WSPR_PEAKS=150:-21:233:-7:")]
    # a list that is not the identity: cycles lie by list entry, events name connections
    cy2 = np.zeros(2, wspr.cycle_dtype)
    cy2[1] = cy[0]
    cy2[0]["npk"] = 1
    cy2[0]["pk"][0] = (99, 0.0, 4.5, 0)
    ev["conn"] = (0, 0)
    assert wspr.messages(ev[1:], cy2, conns=[2, 0]) == [(0, "EXT WSPR_PEAKS=150:-21:233:-7:")]
    ev["conn"] = (2, 2)
    assert wspr.messages(ev[1:], cy2, conns=[2, 0]) == [(2, "EXT WSPR_PEAKS=99:5:")]
    assert wspr.messages(ev[1:], {2: cy2[1]}) == [(2, "EXT WSPR_PEAKS=150:-21:233:-7:")]
