"""kg_wspr_dec.h, stage 2 of the WSPR extension (extensions/wspr/wspr.cpp:45-212, :733-883, fano.cpp) as the host twin runs it, compiled
with g++ -O2 -ffp-contract=off in tools/wspr_dec_host_driver.cpp, against tests/golden/wspr_dec_ref.npz (made by
tools/make_ref_wspr_dec_golden.py from the reference's own statements, with the seeds of the phase recurrences from kg_libm_dtrig.h).
The twin equals the golden in every field of every record; the golden meets its conditions; the encoder and the scenes rebuild;
sin_f2d / cos_f2d are the correctly rounded values (mpmath); the refusals; the prototypes; and six mutations of the twin, each of which
the golden must notice (profiles/wspr_decode_golden.txt argues the one that is equivalent).  Every comparison is an equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from . import wspr_dec_common as W

ROOT = W.ROOT
DEC_SYMBOLS = {
    "kg_wspr_set_metric_table": ("int kg_wspr_set_metric_table(kg_wspr *q, const int32_t mettab[2][256]);", 2),
    "kg_wspr_load_iq": ("int kg_wspr_load_iq(kg_wspr *q, int conn, int half, const float *i_data, const float *q_data, const kg_wspr_cand *cands, int ncand);", 7),
    "kg_wspr_decode": ("int kg_wspr_decode(kg_wspr *q, const int32_t *conns, int nconn, uint32_t maxcycles, int iifac, int quickmode, kg_wspr_dec *out, int32_t *ncand);", 8),
    "kg_wspr_fano": ("int kg_wspr_fano(kg_wspr *q, const uint8_t *symbols, int n, uint32_t maxcycles, int32_t *ok, uint32_t *metric, uint32_t *cycles, uint32_t *maxnp,", 9),
    "kg_wspr_set_decode": ("int kg_wspr_set_decode(kg_wspr *q, int conn, int on);", 3),
    "kg_wspr_decodes": ("int kg_wspr_decodes(kg_wspr *q, int conn, kg_wspr_dec *out, int32_t *ncand);", 4),
    "kg_rxbank_wspr_set_metric_table": ("int kg_rxbank_wspr_set_metric_table(struct kg_rxbank *bank, const int32_t mettab[2][256]);", 2),
    "kg_rxbank_wspr_set_decode": ("int kg_rxbank_wspr_set_decode(struct kg_rxbank *bank, int rx, int on);", 3),
    "kg_rxbank_wspr_dec_out": ("int kg_rxbank_wspr_dec_out(struct kg_rxbank *bank, kg_wspr_dec **d_decs, int32_t **d_ncand, int32_t *rx_decoded, int max_rx);", 5),
}


@pytest.fixture(scope="module")
def golden():
    return W.load()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return W.build_driver(tmp_path_factory.mktemp("wspr_dec"))


def recs_of(g, name):
    return np.ascontiguousarray(g["s_%s_recs" % name]).view(W.rec_dtype)[..., 0]


def test_scenes_and_encoder_rebuild(golden):
    """the seeded samples, candidates, passes and symbol sets are the ones the reference binary was fed; the encoder's bits are what the
    reference's fano hands back for its saturated symbols"""
    assert sorted(W.SCENES) == [str(n) for n in golden["scene_names"]]
    for name in W.SCENES:
        assert bytes(W.scene_sha(name)) == bytes(golden["s_%s_sha" % name]), name
    fs = W.fano_sets()
    assert sorted(fs) == [str(n) for n in golden["fano_names"]]
    for n, (sy, mc) in fs.items():
        assert W.digest(sy.tobytes() + bytes([mc & 255, mc >> 8])) == bytes(golden["f_%s_sha" % n]), n
    sat = golden["f_saturated"].view(W.fano_dtype)[0]
    assert sat["ok"] == 1 and bytes(sat["data"]) == W.encode(W.message_bits(201))[1] and sat["cycles"] == 82
    sym, data = W.channel_symbols(101)
    assert sym.min() >= 0 and sym.max() <= 3 and ((sym & 1) == W.PR3).all() and len(data) == 10 and data[-1] == 0 and data[6] & 0x3f == 0


@pytest.mark.parametrize("name", sorted(W.SCENES))
def test_twin_equals_the_golden(golden, driver, tmp_path, name):
    """every field of every record of every pass, floats by their bits; every jiggle's bytes by digest"""
    got = W.run_scene(driver, name, tmp_path, mettab=golden["mettab"])
    want = recs_of(golden, name)
    for f in W.rec_dtype.names:
        assert got["recs"][f].tobytes() == want[f].tobytes(), (name, f)
    assert W.digest(got["jig"].tobytes()) == bytes(golden["s_%s_jig_sha" % name]) and got["jig"].shape[0] == golden["s_%s_njig" % name][0]


@pytest.mark.parametrize("name", sorted(W.fano_sets()))
def test_twin_fano_equals_the_reference(golden, driver, tmp_path, name):
    sy, mc = W.fano_sets()[name]
    assert W.run_fano(driver, sy, mc, golden["mettab"], tmp_path).tobytes() == golden["f_%s" % name].tobytes()


def test_golden_file_meets_its_conditions(golden):
    W.golden_conditions(golden, os.path.getsize(os.path.join(W.GOLD, "wspr_dec_ref.npz")))


def test_dtrig_is_correctly_rounded(golden, tmp_path):
    """sin_f2d / cos_f2d against mpmath on every 997th float with 0 < x <= 2.5, on their negatives, and on the FOUR tone steps of every
    golden record's final f1 -- a sample of the golden's arguments, not all of them: the maker checks every seed argument of every scene
    (294 122) against libquadmath when the golden is made, and tools/check_wspr_dtrig.cpp runs ALL floats of the domain"""
    import mpmath as mp
    src = tmp_path / "dtrig.cpp"
    src.write_text('#include "%s/flydog_sdr_gps_amd/csrc/kg_wspr_dec.h"\n#include <stdio.h>\nint main() { float d; while (fread(&d, 4, 1, stdin) == 1) { double v[2];\n'
                   'v[0] = kg_libm::sin_f2d((double) d); v[1] = kg_libm::cos_f2d((double) d); fwrite(v, 8, 2, stdout); } return 0; }\n' % ROOT)
    exe = str(tmp_path / "dtrig")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, str(src), "-lm"], check=True)
    x = np.arange(1, np.float32(2.5).view(np.uint32) + 1, 997, dtype=np.uint32).view(np.float32)
    twopidt = np.float32(2 * np.pi * float(np.float32(1.0 / 375.0)))
    extra = []
    for name in W.SCENES:
        for r in recs_of(golden, name).ravel():
            for off in (-1.5, -0.5, 0.5, 1.5):
                extra.append(twopidt * np.float32(r["f1"] + np.float32(off) * np.float32(1.46484375)))
    x = np.concatenate([x, np.array(extra, np.float32), np.array([2.5, 0.0], np.float32)])
    x = np.concatenate([x, -x])
    got = np.frombuffer(subprocess.run([exe], input=x.tobytes(), capture_output=True, check=True).stdout, np.float64).reshape(-1, 2)
    mp.mp.prec = 140
    bad = 0
    for v, (s, c) in zip(x.tolist(), got.tolist()):
        m = mp.mpf(v)
        bad += (float(mp.sin(m)) != s) + (float(mp.cos(m)) != c)
    assert bad == 0 and x.size > 2 * 1079000
    assert np.signbit(got[-1][0]) and got[-1][1] == 1.0                        # sin(-0) = -0


REFUSALS = {"no_table": ("T", 11), "freq0_114": ("C 114.0 768 0.0", 12), "shift0_45001": ("C 10.0 45001 0.0", 12), "drift0_4.5": ("C 10.0 768 4.5", 12),
            "freq0_nan": ("C nan 768 0.0", 12), "iifac_0": ("P 200 0 0", 13), "iifac_129": ("P 200 129 0", 13), "maxcycles_0": ("P 0 2 0", 14)}


def small_scene(path, cand=(10.0, 768, 0.0), ps=(200, 2, 0)):
    with open(path, "wb") as f:
        f.write(np.array([1, 1], np.int32).tobytes())
        f.write(np.zeros(2 * W.TPOINTS, np.float32).tobytes())
        f.write(np.array([(cand[0], cand[1], cand[2], 0.0)], W.cand_in_dtype).tobytes())
        f.write(np.array(ps, np.int32).tobytes())


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(golden, driver, tmp_path, name):
    what, status = REFUSALS[name]
    path = str(tmp_path / "scene.bin")
    kind, *a = what.split()
    small_scene(path, **({"cand": (float(a[0]), int(a[1]), float(a[2]))} if kind == "C" else {"ps": tuple(int(v) for v in a)} if kind == "P" else {}))
    if kind == "T":
        r = subprocess.run([driver, path, str(tmp_path / "o"), str(tmp_path / "j"), str(tmp_path / "no_such_table"), str(tmp_path / "w")])
        assert r.returncode == status
    else:
        W.run_scene(driver, None, tmp_path, mettab=golden["mettab"], expect=status, scene_path=path)


def test_neighbours_of_the_refusals_are_taken(golden, driver, tmp_path):
    for cand, ps in (((113.0, 45000, 4.0), (1, 128, 0)), ((-113.0, -45000, -4.0), (1 << 20, 1, 1))):
        path = str(tmp_path / "scene.bin")
        small_scene(path, cand=cand, ps=ps)
        got = W.run_scene(driver, None, tmp_path, mettab=golden["mettab"], scene_path=path)
        assert got["recs"][0][0]["result"] == W.MINSYNC1                     # silence


# the scene or symbol set that must notice each mutation of the twin (None: equivalent on a golden whose winners are all strictly
# above their runners-up -- which the golden's conditions demand; profiles/wspr_decode_golden.txt)
MUTATIONS = {
    "KG_WSPR_DEC_MUT_K0": ("scene", "early"),               # k > 0 becomes k >= 0
    "KG_WSPR_DEC_MUT_GE": (None, "strong"),                 # ss > syncmax becomes >=
    "KG_WSPR_DEC_MUT_JIG": ("scene", "jig_a"),              # the jiggle order with the sign swapped
    "KG_WSPR_DEC_ACC_T=double": ("scene", "strong"),        # the accumulators kept in double
    "KG_WSPR_DEC_MUT_TAIL": ("scene", "timeup_a"),          # np >= tail becomes >
    "KG_WSPR_DEC_MUT_CYC": ("fano", "last_cycle"),          # i >= maxcycles becomes >
}


@pytest.mark.parametrize("define", sorted(MUTATIONS))
def test_the_golden_notices_a_mutated_twin(golden, tmp_path, define):
    kind, name = MUTATIONS[define]
    exe = W.build_driver(tmp_path, defines=(define,))
    if kind == "fano":
        sy, mc = W.fano_sets()[name]
        assert W.run_fano(exe, sy, mc, golden["mettab"], tmp_path).tobytes() != golden["f_%s" % name].tobytes()
        return
    got = W.run_scene(exe, name, tmp_path, mettab=golden["mettab"])
    same = got["recs"].tobytes() == recs_of(golden, name).tobytes()
    assert same == (kind is None), (define, name)


def test_dec_symbols_declared_bound_and_exported():
    """the prototypes rule of tests/test_wspr_cpu.py, on include/kiwigpu_wspr_dec.h"""
    from flydog_sdr_gps_amd import _lib, wspr
    header = open(os.path.join(ROOT, "include", "kiwigpu_wspr_dec.h")).read()
    assert '#include "kiwigpu_wspr_dec.h"' in open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in DEC_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.WSPR_DEC_SYMBOLS and len(_lib.WSPR_DEC_SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
    protos = re.findall(r"\b(kg_\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert sorted(n for n, _ in protos) == sorted(DEC_SYMBOLS)
    for n, a in protos:
        assert not re.search(r"\bvoid\s*\*", a), (n, "every pointer is typed")
        assert not re.search(r"(?<!\*)\*\s*d_\w+", a), (n, "no parameter is a single pointer named d_...")
        assert len(a.split(",")) == DEC_SYMBOLS[n][1], n
    for s in DEC_SYMBOLS:                                                     # every prototype cites the reference lines it replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s*%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    assert wspr.dec_dtype.itemsize == 304 == W.rec_dtype.itemsize and [n for n in wspr.dec_dtype.names] == [n for n in W.rec_dtype.names]
    d = {k: int(v) for k, v in re.findall(r"KG_WSPR_(SKIPPED|MINSYNC1|NO_CHANGE|TIME_UP|DECODED|QUICK_MISS) = (\d+)", header)}
    assert d == dict(SKIPPED=0, MINSYNC1=1, NO_CHANGE=2, TIME_UP=3, DECODED=4, QUICK_MISS=5)
    assert "KG_WSPR_EV_DECODES = 2" in header and wspr.EV_DECODES == 2
    assert (wspr.SKIPPED, wspr.MINSYNC1, wspr.NO_CHANGE, wspr.TIME_UP, wspr.DECODED, wspr.QUICK_MISS) == (0, 1, 2, 3, 4, 5)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_wspr_dec.h")).read()
    assert "0xf2d05351u" in src and "0xe4613c47u" in src
