"""kg_lorc.h, the Loran-C extension (extensions/Loran_C/loran_c.cpp) as kg_lorc's kernel and host schedule run it, compiled for the host
with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/lorc_host_driver.cpp, against tests/golden/lorc_ref.npz
(made by tools/make_ref_lorc_golden.py from the reference's own statements): per script every row -- bytes, command, length, channel,
block, sample, order -- and the end state bit for bit, sample by sample and through the run decomposition.  Then the run decomposition
against the per-sample schedule over 2.4 million samples, the conditions the golden file must meet so that the parity tests cannot
pass vacuously, every refusal with its neighbours, and the prototypes.  Every comparison is an equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from . import lorc_common as lc

ROOT = lc.ROOT
LORC_SYMBOLS = {
    "kg_lorc_create": ("int kg_lorc_create(kg_ctx *ctx, int nconn, kg_lorc **out);", 3),
    "kg_lorc_destroy": ("void kg_lorc_destroy(kg_lorc *q);", 1),
    "kg_lorc_init": ("int kg_lorc_init(kg_lorc *q, int conn, double srate, int i_srate);", 4),
    "kg_lorc_set_gri": ("int kg_lorc_set_gri(kg_lorc *q, int conn, int ch, int gri);", 4),
    "kg_lorc_set_offset": ("int kg_lorc_set_offset(kg_lorc *q, int conn, int ch, int offset);", 4),
    "kg_lorc_set_gain": ("int kg_lorc_set_gain(kg_lorc *q, int conn, int ch, int gain);", 4),
    "kg_lorc_set_avg_algo": ("int kg_lorc_set_avg_algo(kg_lorc *q, int conn, int ch, int avg_algo);", 4),
    "kg_lorc_set_avg_param": ("int kg_lorc_set_avg_param(kg_lorc *q, int conn, int ch, double avg_param);", 4),
    "kg_lorc_start": ("int kg_lorc_start(kg_lorc *q, int conn);", 2),
    "kg_lorc_stop": ("int kg_lorc_stop(kg_lorc *q, int conn);", 2),
    "kg_lorc_process": ("int kg_lorc_process(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride,", 12),
    "kg_lorc_plan": ("int kg_lorc_plan(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, int32_t *nruns, int32_t *nrows, size_t *row_bytes);", 8),
    "kg_lorc_state": ("int kg_lorc_state(kg_lorc *q, int conn, kg_lorc_info *info, float *avg);", 4),
    "kg_lorc_ms_per_bin": ("float kg_lorc_ms_per_bin(double srate, int i_srate);", 2),
}
BANK = ("_init", "_set_gri", "_set_offset", "_set_gain", "_set_avg_algo", "_set_avg_param", "_start", "_stop", "", "_map", "_rows")


@pytest.fixture(scope="module")
def golden():
    return lc.load()


@pytest.fixture(scope="module")
def pool():
    return lc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return lc.build_driver(tmp_path_factory.mktemp("lorc"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded samples and the scripts are the ones the reference binary was fed; |re|, |im| stay at or below 3e4"""
    assert lc.digest(pool.tobytes()) == bytes(golden["pool_sha"])
    assert pool.size == lc.POOL and (pool[lc.AT["silence_noise"]:][:lc.SILENCE] == 0).all() and pool[lc.AT["silence_noise"] + lc.SILENCE] != 0
    sc = lc.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert lines == [str(l) for l in golden["s_%s_script" % k]], k


@pytest.mark.parametrize("by_runs", [False, True], ids=["per_sample", "by_runs"])
@pytest.mark.parametrize("name", sorted(lc.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name, by_runs):
    got = lc.run_script_exe(driver, lc.scripts()[name], pool, tmp_path, by_runs=by_runs)
    lc.check_against_golden(golden, name, got)


def test_the_run_decomposition_equals_the_per_sample_schedule(driver):
    """per sample (bn, row, clear, navgs) and the scalars behind, one fmod a run against one a sample: samp below the offset at the
    start, the 2^32 wrap of samp, a halved GRI, the rate 12001.3, nbucket 1 and 2"""
    r = subprocess.run([driver, "selftest"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
    lines = dict(l.split(": ", 1) for l in r.stdout.strip().split("\n")[:-1])
    num = {k: [float(v) for v in re.findall(r"-?\d+\.?\d*", l)] for k, l in lines.items()}           # samples, runs, rows, clears, wraps, nbucket, samp_per_GRI
    assert sum(v[0] for v in num.values()) >= 2e6
    assert {"below_offset", "samp_wrap", "halved_12001.3", "rate_12001.3", "nbucket_1", "nbucket_2"} <= set(num)
    assert num["samp_wrap"][4] == 1 and num["halved_12001.3"][4] == 1 and num["nbucket_2"][4] == 1 and num["below_offset"][4] == 0
    assert num["halved_12001.3"][5] == 808 and abs(num["halved_12001.3"][6] - 12001.3 * 20250 / 12000 * 0.0798 / 2) < 1e-5
    assert abs(num["rate_12001.3"][6] - 12001.3 * 0.0897) < 1e-5
    assert num["nbucket_1"][5] == 1 and num["nbucket_1"][1] == 100000 and num["nbucket_2"][5] == 2
    for k, v in num.items():
        assert v[1] >= v[0] / 1200 and v[2] >= 5 and v[3] >= 1, (k, v)


def golden_conditions(g, size):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    sc = lc.scripts()
    S = lambda name: np.frombuffer(g["s_%s_scalars" % name].tobytes(), lc.scalars_dtype)[0]
    assert len(sc) >= 12
    varied, cmds, ended = 0, set(), set()
    for name in sc:
        k, st = "s_%s_" % name, S(name)
        ch, cmd, ln, samp, nrows = (g[k + f] for f in ("ch", "cmd", "len", "samp", "nrows"))
        assert g[k + "rows"].size == int(ln.sum()) and ch.size == int(nrows.sum())
        for c in range(2):                                                                     # a row per started channel with a GRI
            assert st["ch"][c]["nbucket"] >= 1 and (ch == c).sum() >= 1, (name, c)
        cmds |= set(cmd.tolist())
        allb = g[k + "rows"]
        varied += 2 * int(((allb == 0) | (allb == 255)).sum()) < allb.size
        for c in range(2):
            if (g[k + "avg"][c] != 0).any():
                ended.add(int(st["ch"][c]["avg_algo"]))
        blk = np.repeat(np.arange(nrows.size), nrows)                                          # send order: sample-major, channel 0 first
        key = list(zip(blk.tolist(), samp.tolist(), ch.tolist()))
        assert key == sorted(key), name
        assert np.isfinite(g[k + "avg"]).all(), name
    assert cmds == {0, 1} and ended == {0, 1, 2} and 2 * varied >= len(sc), (cmds, ended, varied)
    # both channels emit on the same sample
    k = "s_same_sample_"
    both = [a for a, b in zip(zip(np.repeat(np.arange(g[k + "nrows"].size), g[k + "nrows"]).tolist(), g[k + "samp"].tolist()),
                              zip(np.repeat(np.arange(g[k + "nrows"].size), g[k + "nrows"]).tolist()[1:], g[k + "samp"].tolist()[1:])) if a == b]
    assert len(both) >= 3
    assert g[k + "cmd"].tolist()[:2] == [1, 0] and g[k + "ch"].tolist()[:2] == [0, 1]          # one SCOPE_RESET for the two of them
    # a CMA reset by time-out, not by restart: no command behind `S`, restart long cleared, and navgs far below the GRIs gone by
    st = S("cma_ema_12000")["ch"][0]
    assert st["avg_algo"] == 0 and st["restart"] == 0 and st["avg_param_i"] == 2 and st["samp"] == 110 * 512
    assert int(st["samp"] / st["samp_per_GRI"]) == 58 and st["navgs"] < 12 and st["avg_samps"] < st["samp"] - 24000
    # the rates: 12000, 20250 (both GRIs halved), 12001.3; i_srate 600 and the real ones
    assert [int(v) for v in S("halved_20250")["ch"]["nbucket"]] == [808, 1008] and S("halved_20250")["i_srate"] == 20250
    assert S("rate_12001.3")["srate"] == 12001.3 and S("same_sample")["i_srate"] == 600 and S("cma_ema_12000")["i_srate"] == 12000
    # gains: auto, fixed with spread bytes, fixed and clipped, auto on silence
    assert S("halved_20250")["ch"][0]["gain"] == np.float32(10.0 ** 3.5) and S("ema_fixed_clipped")["ch"][0]["gain"] == np.float32(1e-3)
    k = "s_ema_fixed_clipped_"
    r0 = [lc_row for lc_row, c in zip(_rows_of(g, "ema_fixed_clipped"), g[k + "ch"]) if c == 0]
    assert all((r[1:-1] == 255).all() and r[-1] == 0 for r in r0[1:])                          # bucket nbucket - 1 is never written
    sil = _rows_of(g, "silence_auto")
    assert (sil[0][1:] == 0).all() and (sil[1][1:] == 0).all() and any((r[1:] != 0).any() for r in sil[4:])       # max == 0, then noise
    # offsets: the unsigned modulo
    assert [int(v) for v in S("offsets")["ch"]["offset"]] == [int(((int(((37 - 500) % 2 ** 32) % 958) - 2000000000) % 2 ** 32) % 958),
                                                              int(((((-3) % 2 ** 32) % 1196) + 700) % 1196 + 1000) % 1196]
    # nbucket 1 and 2: rows of 2 and 3 bytes; bucket 0 of the second is written, nothing of the first
    k = "s_nbucket_1_2_"
    assert set(zip(g[k + "ch"].tolist(), g[k + "len"].tolist())) == {(0, 2), (1, 3)}
    assert (g[k + "avg"][0] == 0).all() and g[k + "avg"][1][0] != 0 and (g[k + "avg"][1][1:] == 0).all()
    # stop / start and the second ext_server_init; ns 170
    k = "s_stop_start_reinit_"
    assert g[k + "nrows"][7:10].sum() == 0 and S("stop_start_reinit")["ch"][0]["gri"] == lc.GRI_B and S("stop_start_reinit")["ch"][0]["samp"] == 8 * 512
    assert any(l.startswith("B 170 ") for l in sc["ns170"]) and S("ns170")["ch"][0]["samp"] == 40 * 170
    # a command of each kind in mid-run
    mid = [l[0] for l in sc["commands_mid_run"][sc["commands_mid_run"].index("S") + 1:] if l[0] != "B"]
    assert set(mid) == {"I", "G", "A", "P"} and {"O"} <= {l[0] for l in sc["offsets"][sc["offsets"].index("S") + 1:]}
    assert size <= 400 * 1024


def _rows_of(g, name):
    k = "s_%s_" % name
    at = np.concatenate([[0], np.cumsum(g[k + "len"])])
    return [g[k + "rows"][at[i]:at[i + 1]] for i in range(g[k + "len"].size)]


def test_golden_file_meets_its_conditions(golden):
    golden_conditions(golden, os.path.getsize(os.path.join(lc.GOLD, "lorc_ref.npz")))


HEAD = ["N 12000.0 600"]
OK2 = ["I 0 7980", "I 1 9960"]
REFUSALS = {
    "channel_2": (HEAD + ["I 2 7980"], 11),
    "channel_negative": (HEAD + ["G -1 5"], 11),
    "gri_0": (HEAD + ["I 0 0"], 12),
    "gri_10000": (HEAD + ["I 0 10000"], 12),
    "gri_9990_at_12000": (HEAD + ["I 1 9990"], 13),                       # nbucket 1199: scope[1199] is one past the array
    "gri_9999_at_23990": (["N 23990.0 23990", "I 0 9999"], 13),           # 2399 halved is 1199
    "offset_before_gri": (HEAD + ["O 0 5"], 14),
    "algo_3": (HEAD + OK2 + ["A 0 3"], 15),
    "algo_negative": (HEAD + OK2 + ["A 1 -1"], 15),
    "push_one_gri_missing": (HEAD + ["I 0 7980", "P 0 1", "S", "B 512 0"], 16),
    "push_no_gri_after_reinit": (HEAD + OK2 + ["P 0 1", "P 1 1", "S", "B 512 0", "N 12000.0 600", "B 512 0"], 16),
    "push_ema_0": (HEAD + OK2 + ["A 0 1", "P 0 0.4", "P 1 1", "S", "B 512 0"], 17),
    "push_ema_negative": (HEAD + OK2 + ["A 1 1", "P 1 -3", "P 0 1", "S", "B 512 0"], 17),
    "push_iir_negative": (HEAD + OK2 + ["A 0 2", "P 0 -0.001", "S", "B 512 0"], 18),
    "push_iir_inf": (HEAD + OK2 + ["A 1 2", "P 1 inf", "S", "B 512 0"], 18),
    "push_iir_nan": (HEAD + OK2 + ["A 1 2", "P 1 nan", "S", "B 512 0"], 18),
    "command_before_init": (["I 0 7980"], 19),
    "block_before_init": (["B 512 0"], 19),
}
ACCEPTED = {
    "gri_1": HEAD + ["I 0 1", "I 1 9999"],                                # at 12 kHz 9999 gives nbucket 1200, halved to 600
    "gri_9980_at_12000": HEAD + ["I 0 9980", "I 1 9980"],                 # nbucket 1198
    "gri_9999_at_23970": ["N 23970.0 23970", "I 0 9999", "I 1 9999"],     # 2397 halved is 1198
    "ema_1": HEAD + OK2 + ["A 0 1", "P 0 0.5", "P 1 1"],                  # lround(0.5) is 1
    "iir_0": HEAD + OK2 + ["A 0 2", "P 0 0"],
    "cma_negative_param": HEAD + OK2 + ["P 0 -2", "P 1 1"],               # the unsigned product is defined
    "stopped_without_gri": HEAD + ["T"],                                  # not registered: the block goes nowhere
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    lc.run_script_exe(driver, lines, pool, tmp_path, expect=status)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path, name):
    lines = ACCEPTED[name] + ([] if "T" in ACCEPTED[name] else ["S"]) + lc._B("loran", 0, 3)
    got = lc.run_script_exe(driver, lines, pool, tmp_path)
    assert np.isfinite(got["avg"]).all()
    want = {"gri_1": [1, 600], "gri_9980_at_12000": [1198, 1198], "gri_9999_at_23970": [1198, 1198]}.get(name)
    if want:
        assert [int(v) for v in got["scalars"]["ch"]["nbucket"]] == want
    assert int(got["scalars"]["ch"][0]["samp"]) == (0 if name == "stopped_without_gri" else 3 * 512)


def test_a_refusal_changes_nothing(pool, driver, tmp_path):
    """refused commands strewn through a script (the driver passes over them with -k) leave every row and the end state as they are
    without them"""
    bad = ["I 0 9990", "I 2 100", "I 0 0", "I 1 10000", "A 0 3", "A 1 -1", "O 2 1", "G 5 1", "P -1 2.0"]
    base = HEAD + OK2 + ["O 0 5", "G 1 -33", "P 0 2", "P 1 2", "S"] + lc._B("loran", 0, 4) + ["A 1 1", "I 0 5930"] + lc._B("loran", 4, 4)
    mixed = []
    for i, l in enumerate(base):
        mixed += [l] + ([bad[i % len(bad)]] if i >= 3 else [])
    want = lc.run_script_exe(driver, base, pool, tmp_path)
    raw = open(tmp_path / "out.bin", "rb").read()
    lc.run_script_exe(driver, mixed, pool, tmp_path, keep_on=True)
    assert open(tmp_path / "out.bin", "rb").read() == raw and want["nrows"].sum() >= 4
    for l in bad:                                                         # and each of them IS refused
        r = subprocess.run([driver, "/dev/stdin", str(tmp_path / "pool.bin"), str(tmp_path / "o2.bin")], input="\n".join(HEAD + OK2 + [l]) + "\n", text=True)
        assert 11 <= r.returncode <= 15, (l, r.returncode)


def test_ms_per_bin():
    """the number of the `EXT ms_per_bin=` line (:223-224): float(1.0 / srate * 1e3), doubled in float above 12 kHz"""
    from flydog_sdr_gps_amd import lorc
    for srate, i_srate in ((12000.0, 12000), (12001.3, 12000), (20250.0, 20250), (20250.0, 12000), (11998.7, 12001)):
        want = np.float32(1.0 / srate * 1e3)
        if i_srate > 12000:
            want = np.float32(want * np.float32(2))
        assert np.float32(lorc.ms_per_bin(srate, i_srate)).tobytes() == want.tobytes(), (srate, i_srate)


def test_lorc_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, lorc
    import flydog_sdr_gps_amd
    assert flydog_sdr_gps_amd.LoranC is lorc.LoranC
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in LORC_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    protos = re.findall(r"\b(kg_lorc\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert len(protos) == len(LORC_SYMBOLS) and not [n for n, a in protos if re.search(r"\bvoid\s*\*", a)]
    bank = dict(re.findall(r"\b(kg_rxbank_lorc\w*)\s*\(([^;{}()]*)\)\s*;", bare))
    assert sorted(bank) == sorted("kg_rxbank_lorc" + s for s in BANK)
    for s, args in bank.items():
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == len(args.split(",")) and hasattr(lib, s) and not re.search(r"\bvoid\s*\*", args), s
    # no prototype of the extension takes a pointer to caller device memory; the bank hands its buffer out
    for n, a in protos + list(bank.items()):
        assert not re.search(r"(?<!\*)\*\s*d_\w+", a), n
    assert re.search(r"uint8_t \*\*d_rows", bank["kg_rxbank_lorc_rows"])
    # every prototype cites the reference lines it replaces
    for s in list(LORC_SYMBOLS) + list(bank):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void|float|kg_lorc \*)\s*\*?%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    h = {k: int(v) for k, v in re.findall(r"\bKG_LORC_([A-Z_]+)\s*=\s*(-?\d+)", header)}
    assert (h["CMA"], h["EMA"], h["IIR"], h["SCOPE_DATA"], h["SCOPE_RESET"]) == (lorc.CMA, lorc.EMA, lorc.IIR, lorc.SCOPE_DATA, lorc.SCOPE_RESET) == (0, 1, 2, 0, 1)
    d = {k: int(v) for k, v in re.findall(r"#define KG_LORC_(\w+)\s+(\d+)", header)}
    assert (d["MAX_BUCKET"], d["MAX_NS"], d["MAX_GRI"]) == (lc.MAX_BUCKET, lc.MAX_NS, 9999) == (lorc.MAX_BUCKET, lorc.MAX_NS, lorc.MAX_GRI)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_lorc.h")).read()
    assert "NCH = 2, MAX_GRI = 9999, MAX_BUCKET = 1199, HALF_THRESHOLD = 12000, MAX_NS = 512" in src
    assert (lorc.row_dtype.itemsize, lorc.info_dtype.itemsize) == (32, 152)


# ---- seeded random scripts (tests/ext_random.py): the combinations of commands and blocks nobody wrote down
@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("lorc")


@pytest.mark.parametrize("by_runs", [False, True], ids=["per_sample", "by_runs"])
def test_random_scripts_host_model_equals_the_fixture(random_ref, pool, driver, tmp_path, by_runs):
    """every seed's script is the one the reference was fed, the host model takes it (exit status 0) and equals the reference in every
    field the fixture keeps: rows per block, sample, channel, command and length of every row, the scalars of the end state bit for
    bit, and the digests of the row bytes and of avg[2][1199]"""
    from . import ext_random as er
    for seed in range(er.NSEED):
        lines = er.lorc_script(seed)
        er.check_record("lorc", seed, lines, lc.run_script_exe(driver, lines, pool, tmp_path, by_runs=by_runs), er.unpack(random_ref, seed))


def test_random_fixture_meets_its_conditions(random_ref):
    """conditions, not measurements: what the 40 seeds must reach between them (ext_random.LORC_CONDITIONS, 300 rows), computed from the
    fixture and the regenerated scripts; none of the 40 was refused by the reference.  SCOPE_RESET is sent behind `SET gri` and `SET
    start` alone (loran_c.cpp:119-121; the walk asserts it of every row), so what no command causes is the CMA's reset by time-out
    (:126): that is the condition"""
    from . import ext_random as er
    er.check_conditions("lorc", random_ref)
    assert os.path.getsize(er.fixture_path("lorc")) <= 64 * 1024
