"""kg_cw.h, the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp) as kg_cw's kernel runs it, compiled for the host with
g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/cw_host_driver.cpp, against tests/golden/cw_ref.npz (made by
tools/make_ref_cw_golden.py from the reference's own statements): per script the events of every sound block, every event's fields and
the end state -- every scalar, the ring, data[] and the sample buffer -- bit for bit.  Then the conditions the golden file must meet so
that the parity tests cannot pass vacuously, every refusal with its neighbours, the event bound and the prototypes.  Every comparison
is an equality.

The directed case for data[data_len - 1] with data_len 0 (csrc/kg_cw.h, DEFINED 3) is the script `gaps`: K ends in a dash and is
finalised by the time-out, so the space that follows reads the word before data[]."""
import os
import re
import subprocess

import numpy as np
import pytest

from . import cw_common as cc

ROOT = cc.ROOT
CW_SYMBOLS = {
    "kg_cw_create": ("int kg_cw_create(kg_ctx *ctx, int nconn, kg_cw **out);", 3),
    "kg_cw_destroy": ("void kg_cw_destroy(kg_cw *q);", 1),
    "kg_cw_start": ("int kg_cw_start(kg_cw *q, int conn, int training_interval, double nom_rate, double srate);", 5),
    "kg_cw_set_wpm": ("int kg_cw_set_wpm(kg_cw *q, int conn, int wpm, int training_interval);", 4),
    "kg_cw_set_pboff": ("int kg_cw_set_pboff(kg_cw *q, int conn, uint32_t pboff);", 3),
    "kg_cw_set_wsc": ("int kg_cw_set_wsc(kg_cw *q, int conn, int wsc);", 3),
    "kg_cw_set_auto_threshold": ("int kg_cw_set_auto_threshold(kg_cw *q, int conn, int on);", 3),
    "kg_cw_set_threshold": ("int kg_cw_set_threshold(kg_cw *q, int conn, int threshold);", 3),
    "kg_cw_stop": ("int kg_cw_stop(kg_cw *q, int conn);", 2),
    "kg_cw_max_events": ("int kg_cw_max_events(int nblk);", 1),
    "kg_cw_push": ("int kg_cw_push(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const uint32_t *now_sec, "
                   "kg_cw_ev *evs,", 10),
    "kg_cw_state": ("int kg_cw_state(kg_cw *q, int conn, kg_cw_info *info);", 3),
}
BANK = ("_start", "_set_wpm", "_set_pboff", "_set_wsc", "_set_auto_threshold", "_set_threshold", "_stop", "_set_now", "", "_out")
FAX_GOLDEN_BYTES = 502916                       # the issue's size limit: no larger than fax_ref.npz


@pytest.fixture(scope="module")
def golden():
    return cc.load()


@pytest.fixture(scope="module")
def pool():
    return cc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return cc.build_driver(tmp_path_factory.mktemp("cw"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded audio and the scripts are the ones the reference binary was fed"""
    assert cc.digest(pool.tobytes()) == bytes(golden["pool_sha"])
    assert pool.size == cc.POOL and pool.size % cc.BLK == 0 and np.abs(pool.astype(np.int32)).max() <= 10000
    sc = cc.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert cc.digest("\n".join(lines).encode()) == bytes(golden["s_%s_script_sha" % k]), k
        assert 100 <= cc.nblocks(lines) <= 400, (k, cc.nblocks(lines))
        assert any(l[0] == "S" for l in lines) and any(l[0] == "P" for l in lines) and any(l[0] in "HA" for l in lines) and any(l[0] == "N" for l in lines), k


@pytest.mark.parametrize("name", sorted(cc.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name):
    got = cc.run_script_exe(driver, cc.scripts()[name], pool, tmp_path)
    cc.check_against_golden(golden, name, got)


def _evs(g, name):
    return np.frombuffer(np.ascontiguousarray(g["s_%s_evs" % name]).tobytes(), cc.ev_dtype)


def _info(g, name):
    return np.frombuffer(g["s_%s_info" % name].tobytes(), cc.info_dtype)[0]


def _train(g, name):
    e = _evs(g, name)
    return e[e["kind"] == cc.TRAIN]["a"]


def _letters(g, name):
    e = _evs(g, name)
    a = e[e["kind"] == cc.CHARS]["a"]
    return int(((a != 0xff) & (a != ord(" "))).sum())


def golden_conditions(g, size):
    """conditions on the reference's output alone, not measurements: without them the parity tests could pass on a file that never
    leaves the easy path.  stats (the harness's count, tools/ref/ref_cw_main.cpp): errors that took the first corrective branch, those
    that succeeded, the same for the second."""
    sc = cc.scripts()
    assert size <= FAX_GOLDEN_BYTES and len(sc) >= 16
    for name in sc:
        assert int(g["s_%s_nev" % name].sum()) == _evs(g, name).size >= 100, name
        assert set(_evs(g, name)["kind"].tolist()) | {cc.TRAIN} == {cc.CHARS, cc.WPM, cc.TRAIN, cc.PLOT}, name
    # the clean script spells the keyed message with its word spaces behind the preamble, prosign included; training completed on the way
    text = cc.text_of(_evs(g, "clean_fixed"))
    assert text.endswith(" " + cc.MSG + " ") and text.count(" ") >= len(cc.MSG.split()), text
    tr = _train(g, "clean_fixed")
    assert tr.max() == 39 and tr[-1] == 0 and (np.diff(tr[:-1]) >= 0).all() and _info(g, "clean_fixed")["initialized"] == 1 and (tr > cc_stable()).any()
    assert cc.text_of(_evs(g, "fixed_wpm")) == cc.PRE + cc.MSG + " " and _train(g, "fixed_wpm").size == 0 and _info(g, "fixed_wpm")["track"] == 0
    # automatic and fixed threshold each decode at least ten characters
    assert _letters(g, "auto_threshold") >= 10 and _info(g, "auto_threshold")["isAutoThreshold"] == 1 and _info(g, "auto_threshold")["threshold_linear"] == 15849
    assert _letters(g, "clean_fixed") >= 10 and _info(g, "clean_fixed")["isAutoThreshold"] == 0 and _info(g, "clean_fixed")["threshold_linear"] == 20000
    assert cc.text_of(_evs(g, "auto_threshold")).endswith(" " + cc.MSG + " ")
    assert cc.text_of(_evs(g, "jitter_25")).endswith("THE QUICK FOX <ar> ")
    # the first corrective branch succeeds; the second is taken and fails.  It cannot succeed: csrc/kg_cw.h shows it from the code
    st = {n: g["s_%s_stats" % n] for n in sc}
    assert st["glitch_dropped"][0] >= 1 and st["glitch_dropped"][1] >= 1 and "TEST F" in cc.text_of(_evs(g, "glitch_dropped")) and _train(g, "glitch_dropped").min() == 0
    assert st["run_on_split"][2] >= 1 and st["run_on_split"][3] == 0 and "[err]" in cc.text_of(_evs(g, "run_on_split")) and _train(g, "run_on_split").min() == -1
    assert sum(int(s[3]) for s in st.values()) == 0
    # the fourth error restarts the training
    tr = _train(g, "garble_retrain")
    neg = np.flatnonzero(tr < 0)
    assert tr[neg].tolist() == [-1, -2, -3, -4] and (tr[neg[-1] + 1:] > 0).any() and cc.text_of(_evs(g, "garble_retrain")).count("[err]") == 4
    # err_timeout clears err_cnt: `cw_train=0` behind the error count, outside any training
    tr, info = _train(g, "err_timeout"), _info(g, "err_timeout")
    neg = np.flatnonzero(tr < 0)
    assert tr[neg].tolist() == [-1] and tr[neg[0] + 1:].tolist() == [0] and info["err_cnt"] == 0 and info["err_timeout"] == 0 and info["initialized"] == 1
    # the time-out finalises K long before the key comes down again; the 3 s clamp (136 * 3) and the stuck key are in the ring
    e = _evs(g, "gaps")
    ch = e[e["kind"] == cc.CHARS]
    k = int(np.flatnonzero(ch["a"] == ord("K"))[-1])
    nxt = ch[k + 1:][ch[k + 1:]["a"] != ord(" ")]
    ring = _info(g, "gaps")["sig"]
    assert ch["a"][k + 1] == ord(" ") and nxt["a"][0] == ord("N") and nxt["blk"][0] - ch["blk"][k] >= 40
    assert ((ring & 1) == 0)[ring >> 1 == 408].any() and (ring >> 1 == 408).any() and (((ring & 1) == 1) & (ring >> 1 > 300)).any()
    # [err] for a character of 44 elements
    assert cc.text_of(_evs(g, "too_long")).count("[err]") == 1
    # the word-space correction swallows the space behind YOU
    on, off = cc.text_of(_evs(g, "wsc_on")), cc.text_of(_evs(g, "wsc_off"))
    assert "TEST YOUARE HERE " in on and "TEST YOU ARE HERE " in off and _info(g, "wsc_off")["wsc"] == 0 and _info(g, "wsc_on")["wsc"] == 1
    # the other scripts leave the easy path where they say they do
    assert _evs(g, "pboff_mid").tobytes() != _evs(g, "clean_fixed").tobytes() and cc.text_of(_evs(g, "pboff_mid")).endswith("K1ABC PSE <kn> ")
    r = _info(g, "restart_mid")
    assert r["threshold_linear"] == 15000 and r["training_interval"] == 30 and (_train(g, "restart_mid") == 29).any()
    s = _evs(g, "silence_then_signal")
    quiet = s[s["blk"] < 30]
    assert quiet.size >= 50 and set(quiet["kind"].tolist()) == {cc.PLOT, cc.TRAIN} and (quiet["a"] == 0).all() and _letters(g, "silence_then_signal") >= 10   # 0 dB, training at 0
    f = _info(g, "rate_20250")
    assert f["snd_rate"] == 20250 and f["sampling_freq"] == np.float32(20250.0) and f["g_a"] == 4 and "CQ" in cc.text_of(_evs(g, "rate_20250"))
    o = _info(g, "rate_off_nominal")
    assert o["sampling_freq"] == np.float32(12001.37) and o["started"] == 0 and g["s_rate_off_nominal_nev"][-5:].sum() == 0
    assert (_evs(g, "clean_fixed")["a"][_evs(g, "clean_fixed")["kind"] == cc.CHARS] < 12).any()


def cc_stable():
    return 32                                   # TRAINING_STABLE


def test_golden_file_meets_its_conditions(golden):
    golden_conditions(golden, os.path.getsize(os.path.join(cc.GOLD, "cw_ref.npz")))


HEAD = cc.HEAD
REFUSALS = {
    "interval_0": ([cc._S(0)], 21),
    "interval_256": ([cc._S(256)], 21),
    "interval_negative": ([cc._S(-5)], 21),
    "wpm_negative": ([cc._S(), "W -1 40"], 22),
    "wpm_0_interval_0": ([cc._S(), "W 0 0"], 21),
    "wpm_before_start": (["W 30 40"], 25),
    "pboff_bin_45": ([cc._S(), "P 6069"], 23),
    "pboff_far": ([cc._S(), "P 4000000000"], 23),
    "pboff_before_start": (["P 818"], 25),
    "nominal_87": ([cc._S(40, 87)], 24),
    "nominal_above_1e6": ([cc._S(40, 1000001)], 24),
    "srate_low": ([cc._S(40, 12000, 5999.0)], 24),
    "srate_high": ([cc._S(40, 12000, 24001.0)], 24),
    "srate_0": ([cc._S(40, 12000, 0.0)], 24),
    "srate_negative": ([cc._S(40, 12000, -12000.0)], 24),
    "srate_nan": ([cc._S(40, 12000, float("nan"))], 24),
    "srate_inf": ([cc._S(40, 12000, float("inf"))], 24),
}
ACCEPTED = {
    "interval_1": [cc._S(1), "P 818", "H 20000"],
    "interval_255": [cc._S(255), "P 818", "H 20000"],
    "wpm_0": [cc._S(), "W 0 40", "P 818", "H 20000"],
    "wpm_fixed_any_interval": [cc._S(), "W 30 0", "P 818", "H 20000"],
    "pboff_bin_44": [cc._S(), "P 6068", "H 20000"],
    "pboff_0": [cc._S(), "P 0", "H 20000"],
    "nominal_88": [cc._S(40, 88, 88.0), "P 10", "H 20000"],
    "nominal_1e6": [cc._S(40, 1000000), "P 818", "H 20000"],
    "srate_half": [cc._S(40, 12000, 6000.0), "P 818", "H 20000"],
    "srate_twice": [cc._S(40, 12000, 24000.0), "P 818", "H 20000"],
    "threshold_negative": [cc._S(), "P 818", "H -1"],
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    cc.run_script_exe(driver, lines, pool, tmp_path, expect=status)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path, name):
    lines = ACCEPTED[name] + cc._B("clean", 0, 30)
    got = cc.run_script_exe(driver, lines, pool, tmp_path)
    info = got["info"]
    assert info["started"] == 1 and info["process_samples"] == 1 and info["blocksize"] == 88 and 0 <= info["g_a"] <= 44
    assert info["sample_counter"] == (30 * 512) % 88 and (got["evs"]["kind"] == cc.PLOT).sum() == (30 * 512 // 88) // 3


def test_a_refusal_changes_nothing(pool, driver, tmp_path):
    """refused commands strewn through a script (the driver passes over them with -k) leave every event and the end state as they are
    without them"""
    bad = [cc._S(0), cc._S(256), "W -1 40", "W 0 0", "W 0 300", "P 6069", "P 100000", cc._S(40, 12000, 100.0), cc._S(40, 12000, float("nan")), cc._S(40, 50),
           cc._S(40, 2000000)]
    base = HEAD + cc._B("clean", 0, 120) + ["P 700"] + cc._B("clean", 120, 40) + ["P 818", "A 1"] + cc._B("clean", 160, 60)
    mixed = []
    for i, l in enumerate(base):
        mixed += [l] + ([bad[(i // 7) % len(bad)]] if i % 7 == 0 else [])
    want = cc.run_script_exe(driver, base, pool, tmp_path)
    raw = open(tmp_path / "out.bin", "rb").read()
    cc.run_script_exe(driver, mixed, pool, tmp_path, keep_on=True)
    assert open(tmp_path / "out.bin", "rb").read() == raw and want["evs"].size >= 300 and (want["evs"]["kind"] == cc.CHARS).sum() >= 5
    for l in bad:                                                         # and each of them IS refused
        r = subprocess.run([driver, "/dev/stdin", str(tmp_path / "pool.bin"), str(tmp_path / "o2.bin")], input="\n".join(HEAD + [l]) + "\n", text=True)
        assert 21 <= r.returncode <= 25, (l, r.returncode)


def test_event_bound_holds_for_every_script(golden):
    """kg_cw_max_events' bound, 7 events a Goertzel block and (512 nblk + 87) / 88 Goertzel blocks a push, against what the reference
    sent: per Goertzel block, and in every window of 1, 7 and 64 sound blocks of every script"""
    assert cc.max_events(1) == 42 and cc.max_events(7) == 7 * 41 and cc.max_events(256) == 7 * 1490 and cc.max_events(0) == 0
    most = 0
    for name in cc.scripts():
        e, nev = _evs(g := golden, name), golden["s_%s_nev" % name].astype(np.int64)
        assert e["gblk"].min() >= 0 and e["gblk"].max() <= 6
        per = np.bincount(e["blk"].astype(np.int64) * 8 + e["gblk"])
        assert per.max() <= 7, (name, per.max())
        most = max(most, int(per.max()))
        c = np.concatenate([[0], np.cumsum(nev)])
        for k in (1, 7, 64):
            assert (c[k:] - c[:-k]).max() <= cc.max_events(k), (name, k)
        assert g is golden
    assert most >= 4                                                    # a character, its space, the speed and the plot in one Goertzel block


def test_cw_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, cw
    import flydog_sdr_gps_amd
    assert flydog_sdr_gps_amd.CwDecoder is cw.CwDecoder
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in CW_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    protos = re.findall(r"\b(kg_cw\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert sorted(n for n, _ in protos) == sorted(CW_SYMBOLS) and not [n for n, a in protos if re.search(r"\bvoid\s*\*", a) or re.search(r"(?<!\*)\*\s*d_\w+", a)]
    for n, a in protos:
        assert len(a.split(",")) == CW_SYMBOLS[n][1], n
    # every prototype cites the reference lines it replaces
    for s in CW_SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void)\s*%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    bank = dict(re.findall(r"\b(kg_rxbank_cw\w*)\s*\(([^;{}()]*)\)\s*;", bare))
    assert sorted(bank) == sorted("kg_rxbank_cw" + s for s in BANK)
    for s, args in bank.items():
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == len(args.split(",")) and hasattr(lib, s), s
        assert not re.search(r"\bvoid\s*\*", args) and not re.search(r"(?<!\*)\*\s*d_\w+", args), s
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|kg_cw \*)\s*\*?%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    h = {k: int(v) for k, v in re.findall(r"\bKG_CW_([A-Z_0-9]+)\s*=\s*(-?\d+)", header)}
    assert (h["CHARS"], h["WPM"], h["TRAIN"], h["PLOT"]) == (cw.CHARS, cw.WPM, cw.TRAIN, cw.PLOT) == (cc.CHARS, cc.WPM, cc.TRAIN, cc.PLOT)
    d = {k: int(v) for k, v in re.findall(r"#define KG_CW_(\w+)\s+(\d+)", header)}
    assert (d["BLK"], d["GBLK"], d["EVENTS_PER_GBLK"]) == (cc.BLK, cc.GBLK, 7) == (cw.BLK, cw.GBLK, cw.EVENTS_PER_GBLK)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_cw.h")).read()
    assert "BLK = 512, GBLK = 88, SIG_BUFSIZE = 256, DATA_BUFSIZE = 40" in src and "EVENTS_PER_GBLK = 7" in src
    assert (cw.ev_dtype, cw.info_dtype) == (cc.ev_dtype, cc.info_dtype) and cw.PROSIGNS == cc.PROSIGNS
    assert lib.kg_cw_max_events(7) == cc.max_events(7) and lib.kg_cw_max_events(257) == -1
    ev = np.zeros(4, cc.ev_dtype)
    ev["kind"] = [cc.CHARS, cc.CHARS, cc.WPM, cc.PLOT]
    ev["a"] = [8, 0xff, 30, np.float32(47.5).view(np.int32)]
    ev["b"], ev["c"] = 1, np.float32(43.0103).view(np.int32)
    assert cw.messages(ev) == ["EXT cw_chars=<kn>", "EXT cw_chars=[err]", "EXT cw_wpm=30", "EXT cw_plot=47.50,1,43.01"] and cw.text(ev) == "<kn>[err]"


# ---- seeded random scripts and shape scripts (tests/ext_random.py): what the hand-written scripts leave out
@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("cw")


def test_random_scripts_host_model_equals_the_fixture(random_ref, pool, driver, tmp_path):
    """every seed's script and every shape script is the one the reference was fed, the host model takes it (exit status 0) and equals
    the reference in every field the fixture keeps: the events of every block, the text, the number of events of every kind, and the digests of the events and of the end state"""
    from . import ext_random as er
    scripts = [er.cw_script(seed) for seed in range(er.NSEED)] + list(er.cw_shapes().values())
    assert int(random_ref["n_script_sha"].size) == len(scripts)
    for k, lines in enumerate(scripts):
        assert cc.nblocks(lines) <= er.MOST_BLOCKS
        er.check_record("cw", k, lines, cc.run_script_exe(driver, lines, pool, tmp_path), er.unpack(random_ref, k))


def test_random_fixture_meets_its_conditions(random_ref):
    """conditions, not measurements: what the 40 seeds must reach between them (ext_random.CW_CONDITIONS), computed from the fixture
    and the regenerated scripts; none of the 40 was refused by the reference.  The shape scripts count towards none"""
    from . import ext_random as er
    er.check_conditions("cw", random_ref)
    assert os.path.getsize(er.fixture_path("cw")) <= 64 * 1024


def test_random_pushes_reach_every_size():
    """the pushes tests/test_cw_gpu.py makes with the seeds under their partitions and with the shape scripts are decided ahead of
    any run: one holds 256 blocks (the most a push takes), one 45 to 255 (a second turn of phase A's loop over the Goertzel blocks, and not the whole of it), one a single block"""
    from . import ext_random_dev as ed
    n = ed.planned_pushes("cw")
    assert max(n) == 256 and any(45 <= k <= 255 for k in n) and 1 in n and min(n) >= 1


def test_random_side_by_side_pushes_are_shared():
    """the pushes tests/test_cw_gpu.py makes with the seeds three at a time on one object are decided ahead of the run
    (cw_common.run_side_by_side): over all the groups at least half of them carry more than one connection"""
    from . import ext_random_dev as ed
    every, both = ed.shared_in_all("cw")
    assert 2 * both >= every, (both, every)
