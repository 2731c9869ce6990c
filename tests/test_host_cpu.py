"""CPU-side tests: oracle vs known answers / reference build, host logic, C-ABI
surface, and the N>1 sharding path on gloo (world_size 2)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- PRN generators: pinned --------------------------------------------------
# IS-GPS-200 table 3-Ia, "first 10 chips octal"
FIRST10_OCTAL = {1: 0o1440, 2: 0o1620, 3: 0o1710, 4: 0o1744, 5: 0o1133, 6: 0o1455, 7: 0o1131,
                 8: 0o1454, 9: 0o1626, 10: 0o1504, 11: 0o1642, 12: 0o1750, 13: 0o1764,
                 14: 0o1772, 15: 0o1775, 16: 0o1776, 17: 0o1156, 18: 0o1467, 19: 0o1633,
                 20: 0o1715, 21: 0o1746, 22: 0o1763, 23: 0o1063, 24: 0o1706, 25: 0o1743,
                 26: 0o1761, 27: 0o1770, 28: 0o1774, 29: 0o1127, 30: 0o1453, 31: 0o1625,
                 32: 0o1712}


def test_cacode_known_answers(oracle):
    from flydog_sdr_gps_amd import prn, sats
    for sat, (p, t1, t2, kind) in enumerate(sats.SATS):
        if kind == sats.E1B:
            continue
        chips = oracle.cacode(t1, t2)
        assert np.array_equal(chips, prn.cacode(t1, t2))
        assert chips.sum() == 512                      # balanced Gold code: 512 ones
        if kind == sats.NAVSTAR:
            first10 = int("".join(map(str, chips[:10])), 2)
            assert first10 == FIRST10_OCTAL[p], p


def test_cacode_matches_reference_build(oracle):
    """tests/golden/cacode_ref.npz: the chips of oracle/_ref/cacode_ref, the reference's own gps/cacode.h compiled in place
    (tools/make_ref_text_golden.py), for every C/A + QZSS row of Sats[]."""
    from flydog_sdr_gps_amd import sats
    g = np.load(os.path.join(ROOT, "tests", "golden", "cacode_ref.npz"))
    ref = {tuple(int(v) for v in t): np.unpackbits(c)[:1023] for t, c in zip(g["taps"], g["chips_packed"])}
    rows = [(p, t1, t2) for p, t1, t2, kind in sats.SATS if kind != sats.E1B]
    assert len(rows) == len(ref) == 36
    for p, t1, t2 in rows:
        assert np.array_equal(oracle.cacode(t1, t2), ref[(t1, t2)]), p


def test_gold_code_correlation_property(oracle):
    """Cyclic autocorrelation of a C/A code takes only the values {1023, -1, 63, -65}."""
    c = 1.0 - 2.0 * oracle.cacode(2, 6)
    ac = np.rint(np.fft.ifft(np.abs(np.fft.fft(c)) ** 2).real).astype(int)
    assert ac[0] == 1023 and set(ac[1:]) <= {-1, 63, -65}


def test_e1b_known_answers(oracle):
    """gps/search.cpp:295,302: first 20 chips of E01 = 0xf5d71, E02 = 0x96b85 (chips: the reference's E1BCODE outputs,
    tests/golden/e1b_ref.npz; the hex digits are re-derived from them, no reference text is kept here)."""
    from flydog_sdr_gps_amd import prn
    from tests.fixtures import e1b_chips
    from tests.test_ref_pins_cpu import chips_to_hex
    table = e1b_chips()
    for p, first in ((1, 0xF5D71), (2, 0x96B85)):
        hexstr = chips_to_hex(table[p])
        chips = oracle.e1b_from_hex(hexstr)
        assert np.array_equal(chips, prn.e1b_from_hex(hexstr)) and np.array_equal(chips, table[p])
        assert int("".join(map(str, chips[:20])), 2) == first
        assert chips.size == 4092
    with pytest.raises(ValueError):
        oracle.e1b_from_hex("G" * 1023)


# ---- FFT / filters -----------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 8192, 16384])
@pytest.mark.parametrize("sign", [-1, 1])
def test_oracle_fft_vs_numpy(oracle, n, sign):
    rng = np.random.default_rng(n + sign)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    ref = np.fft.fft(x.astype(np.complex128)) if sign < 0 else np.fft.ifft(x.astype(np.complex128)) * n
    for prec, tol in ((1, 2e-7), (0, 3e-6)):
        got = oracle.fft(x, sign, prec)
        assert np.abs(got - ref).max() / np.abs(ref).max() < tol


def test_decimate_by2_definition(oracle):
    """y[o] = sum_j c[j] x[2o+j] with a zero tail (gps/search.cpp:140-166)."""
    c = np.zeros(31)
    c[0:15:2] = [-0.010233, 0.010668, -0.016324, 0.024377, -0.036482, 0.056990, -0.101993, 0.316926]
    c[15] = 0.500009
    c[16:31:2] = c[14::-2]
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(256) + 1j * rng.standard_normal(256)).astype(np.complex64)
    xp = np.concatenate([x.astype(np.complex128), np.zeros(31)])
    want = np.array([np.dot(c, xp[2 * o:2 * o + 31]) for o in range(128)])
    got = oracle.decimate_by2(x)
    assert got.shape == (128,)
    assert np.abs(got - want).max() < 2e-6


def test_sample_bits_mix_convention(oracle):
    """A real tone at FC + f mixes to +f (search.cpp:383-423): the strongest bin of
    the Sample() spectrum is +f / BIN_SIZE."""
    n = np.arange(65536)
    f = 40 * 249.755859375
    x = np.cos(2 * np.pi * (4.092e6 + f) * n / 16.368e6 + 0.3)
    packed = np.packbits((x < 0).astype(np.uint8), bitorder="little")
    spec = oracle.sample_bits(packed)
    assert int(np.argmax(np.abs(spec))) == 40


def test_oracle_acquisition_recovers_injected_signal(oracle):
    from flydog_sdr_gps_amd import prn, synth
    bits = synth.config0_bits()
    r, cells = oracle.correlate(oracle.code_fft(prn.cacode(2, 6)), oracle.sample_bits(bits))
    assert (r["dop"], r["idx"], r["valid"]) == (6, 1202, 1) and r["snr"] > 16
    assert cells.shape == (41,)
    # fp32 "port" FFT agrees on the integers
    r0, _ = oracle.correlate(oracle.code_fft(prn.cacode(2, 6), prec=0),
                             oracle.sample_bits(bits, prec=0), prec=0)
    assert (r0["dop"], r0["idx"]) == (6, 1202) and abs(r0["snr"] - r["snr"]) < 1e-3 * r["snr"]


def test_golden_acquisition_vectors(oracle):
    """Committed fixtures (tests/golden/acq_golden.npz, made by tools/make_golden.py)."""
    from flydog_sdr_gps_amd import prn, sats
    g = np.load(os.path.join(ROOT, "tests", "golden", "acq_golden.npz"))
    for k in range(int(g["ncases"])):
        sat = int(g["case%d_sat" % k])
        kind = sats.SATS[sat][3]
        if kind == sats.E1B:
            chips = g["case%d_chips" % k]
            code = oracle.code_fft(chips, boc=True)
            limit = sats.E1B_LIMIT
        else:
            code = oracle.code_fft(prn.cacode(sats.SATS[sat][1], sats.SATS[sat][2]))
            limit = sats.L1_LIMIT
        r, cells = oracle.correlate(code, oracle.sample_bits(g["case%d_bits" % k]), limit=limit)
        want = g["case%d_result" % k]
        assert (r["dop"], r["idx"], r["valid"]) == (int(want[1]), int(want[2]), int(want[3]))
        assert abs(r["snr"] - want[0]) <= 1e-6 * max(1.0, want[0])
        assert np.array_equal(cells["idx"], g["case%d_cell_idx" % k])


# ---- C ABI surface -----------------------------------------------------------
def test_library_exports_every_declared_symbol():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    declared = set(re.findall(r"\b(kg_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load_library()                      # raises if the .so is missing a symbol
    assert lib.kg_abi_version() == _lib.ABI_VERSION == 4          # bumped with every change of an existing signature or layout
    assert lib.kg_strerror(-1).decode().startswith("no usable")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from flydog_sdr_gps_amd import Context, KiwiGpuError
    with pytest.raises(KiwiGpuError) as e:
        Context(0)
    assert "no CPU fallback" in str(e.value) or e.value.status == -1


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "flydog_sdr_gps_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "kiwi_oracle" not in text and "oracle/" not in text, f


# ---- host logic ----------------------------------------------------------------
def test_shard_helpers():
    from flydog_sdr_gps_amd import shard
    assert shard.block_ids(1, 4, 2) == [2, 3]
    assert shard.split_units(59, 8) == [(0, 8), (8, 16), (16, 24), (24, 31), (31, 38), (38, 45),
                                        (45, 52), (52, 59)]
    with pytest.raises(ValueError):
        shard.block_ids(4, 4, 1)


def test_weighted_sv_split_is_balanced_and_a_partition():
    """shard.split_units_weighted on the reference's own SV order (gps/sats.cpp:25-142: 36 C/A + QZSS rows, then the 23
    E1B rows, an E1B SV costing 1.6 C/A ones): the worst rank within 105 % of the mean at world 2, 4, 8 (the
    contiguous split: 124 % at world 8); every SV in exactly one share; shares ascending; deterministic."""
    from flydog_sdr_gps_amd import sats, shard
    is_e1b = [row[3] == sats.E1B for row in sats.SATS]
    assert (len(is_e1b), sum(is_e1b)) == (59, 23) and not any(is_e1b[:36])
    w = shard.sv_weights(is_e1b)
    mean_of = lambda world: sum(w) / world                                  # noqa: E731
    for world in (1, 2, 3, 4, 5, 6, 7, 8):
        shares = shard.split_units_weighted(w, world)
        assert len(shares) == world and sorted(i for sh in shares for i in sh) == list(range(59))
        assert all(sh == sorted(sh) for sh in shares)
        worst = max(sum(w[i] for i in sh) for sh in shares)
        assert worst <= 1.05 * mean_of(world), (world, worst / mean_of(world))
        assert shares == shard.split_units_weighted(w, world)
    contiguous = max(sum(w[i] for i in range(lo, hi)) for lo, hi in shard.split_units(59, 8))
    assert contiguous > 1.2 * mean_of(8)                                    # what the weighted split replaces
    # degenerate shapes: more ranks than units, one unit, equal weights
    assert sorted(map(tuple, shard.split_units_weighted([1.0, 1.0], 4))) == [(), (), (0,), (1,)]
    assert shard.split_units_weighted([2.5], 1) == [[0]]
    eq = shard.split_units_weighted([1.0] * 32, 8)
    assert sorted(len(sh) for sh in eq) == [4] * 8
    with pytest.raises(ValueError):
        shard.split_units_weighted([1.0, 0.0], 2)


def test_merge_sv_shards_takes_index_lists():
    from flydog_sdr_gps_amd import shard
    from flydog_sdr_gps_amd._lib import result_dtype
    B, shares = 2, [[0, 3, 4], [1, 5], [2, 6]]
    full = np.zeros((B, 7), result_dtype)
    full["snr"] = np.arange(14).reshape(B, 7)
    full["idx"] = 100 + full["snr"].astype(int)
    parts = np.zeros((3, B * 3), result_dtype)
    for r, sh in enumerate(shares):
        parts[r, :B * len(sh)] = full[:, sh].reshape(-1)
        parts[r, B * len(sh):]["snr"] = -1
    assert np.array_equal(shard.merge_sv_shards(parts, B, shares), full)
    with pytest.raises(AssertionError):
        shard.merge_sv_shards(parts, B, [[0, 1], [1, 2], [3]])              # not a partition


def test_nco_table_by_construction_equals_the_oracle_definition(oracle):
    """kg_ddc_nco_table (host function of libkiwigpu, no GPU): the device's ONE sine table with cos(a) = T[a + 2048]
    against the oracle's two separately rounded tables round(16383 cos / sin(2 pi a / 8192)) -- checked here once
    instead of inside kg_ddc_create / kg_rxddc_create (a libm that rounds a half-way point differently
    must fail a test, not a create call)."""
    import ctypes as C
    from flydog_sdr_gps_amd import load_library
    lib = load_library()
    c = np.empty(8192, np.int16)
    s = np.empty(8192, np.int16)
    assert lib.kg_ddc_nco_table(c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)) == 0
    want_c, want_s = oracle.ddc_nco_table()
    assert np.array_equal(s, want_s) and np.array_equal(c, want_c)
    assert (int(c[0]), int(s[2048]), int(c[4096]), int(s[6144])) == (16383, 16383, -16383, -16383)


def test_best_of_merges_like_serial_scan():
    from flydog_sdr_gps_amd import shard
    from flydog_sdr_gps_amd._lib import result_dtype
    a = np.array([(10.0, -3, 5, 1), (0.0, 0, 0, 0), (7.0, 2, 9, 1)], result_dtype)
    b = np.array([(10.0, 4, 6, 1), (3.0, 1, 1, 1), (6.0, 9, 9, 1)], result_dtype)
    m = shard.best_of([a, b])
    assert [tuple(x) for x in m] == [(10.0, -3, 5, 1), (3.0, 1, 1, 1), (7.0, 2, 9, 1)]
    m2 = shard.best_of([b, a])
    assert [tuple(x) for x in m2] == [tuple(x) for x in m]


_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch.distributed as dist
from flydog_sdr_gps_amd import shard
from flydog_sdr_gps_amd._lib import result_dtype
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
blocks = shard.block_ids(rank, world, 2)
local = np.zeros((2, 3), result_dtype)
for i, b in enumerate(blocks):
    local[i]["snr"] = 100 * b + np.arange(3); local[i]["dop"] = b; local[i]["valid"] = 1
g = shard.gather_results(local)
assert g.shape == (2 * world, 3)
for b in range(2 * world):
    assert np.all(g[b]["dop"] == b) and np.allclose(g[b]["snr"], 100 * b + np.arange(3))
# strong split of 32 SVs: every SV searched exactly once
lo, hi = shard.split_units(32, world)[rank]
mine = np.zeros(32, np.int32); mine[lo:hi] = 1
import torch
t = torch.from_numpy(mine); dist.all_reduce(t)
assert np.all(t.numpy() == 1)
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gloo_world2_gather(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
                          "29517", str(script)], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 2


def test_bench_gpus_flag_launches_ranks():
    """`python bench.py --gpus N` (the driver's command line) must START N ranks: the parent spawns
    them before touching torch or the GPU, relays rank 0's line and propagates failures.  Driven here
    with the GPU-free stub workload over gloo."""
    import json
    bench = os.path.join(ROOT, "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, bench, "--gpus", "2", "--workload", "stub"], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # ONE line, from rank 0
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["higher_is_better"] is True
    # the stdout line is the LAST stdout line, small and flat (the driver's record keeps 8 000 characters of it: round 5's
    # 24 KB line was lost whole), with the headline's roofline and cpu_baseline at top level; the stub carries > 24 KB of
    # workload objects, which must have gone to stderr instead
    assert out.stdout.rstrip().splitlines()[-1] == lines[0] and len(lines[0]) <= 8192 // 2
    assert line["roofline"]["frac"] is not None and line["cpu_baseline"]["value"] is not None
    assert set(line["workloads"]) == {"_cols"} | {"w%d" % i for i in range(8)} and line["workloads"]["w3"][4] == 0.5
    full = [l for l in out.stderr.splitlines() if l.startswith("FULL {")]
    assert not full                                          # the stub publishes nothing; a real workload writes `FULL {...}` to stderr
    # a rank started by torchrun with another world size than --gpus refuses to run
    out = subprocess.run([sys.executable, bench, "--gpus", "2", "--workload", "stub"],
                         env=dict(env, WORLD_SIZE="3", RANK="0"), capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "WORLD_SIZE" in out.stderr
    # no GPUs here: every GPU workload fails cleanly, the failure reaches the caller's exit status
    out = subprocess.run([sys.executable, bench, "--gpus", "2", "--workload", "acq", "--steps", "1"], env=env,
                         capture_output=True, text=True, timeout=240)
    if not _have_gpu_count(2):
        assert out.returncode != 0 and "needs GPU" in out.stderr


def test_bench_compact_line_of_a_recorded_full_line():
    """bench.compact_line on round 5's recorded 24 KB default line (profiles/r05_bench_default_final.json): parses, <= 4 KB,
    every contract field and the headline's roofline / cpu_baseline at top level, one row per workload."""
    import json
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default_final.json")))
    assert len(json.dumps(full)) > 20000
    txt = json.dumps(bench.compact_line(full), separators=(",", ":"))
    assert len(txt) <= 4096, len(txt)
    line = json.loads(txt)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"]
    assert line["roofline"]["frac"] == full["roofline"]["frac"] and line["roofline"]["traffic"] == full["roofline"]["traffic"]
    assert line["cpu_baseline"]["value"] == full["cpu_baseline"]["value"] and line["cpu_baseline"]["kind"] == "port"
    assert "workload" in line["config"] and "model" not in line["config"]
    cols = line["workloads"]["_cols"]
    for wl, r in full["workloads"].items():
        row = dict(zip(cols, line["workloads"][wl]))
        assert row["ms_per_step"] == r["ms_per_step"] and row["frac"] == r["roofline"]["frac"]
        assert row["cpu_value"] == r["cpu_baseline"]["value"]
    # a pathologically large input still yields a line under the cap (optional parts are dropped, the contract fields stay)
    huge = dict(full, workloads={("w%04d" % i): full["workloads"]["wf14"] for i in range(400)})
    txt = json.dumps(bench.compact_line(huge), separators=(",", ":"))
    assert len(txt) <= bench.COMPACT_MAX and "roofline" in json.loads(txt)


def test_bench_shard_sv_world2_on_the_stub():
    """`bench.py --workload acq10ms --shard sv` splits the 59 SVs of ONE block over the ranks, all-gathers the
    winners and merges them (shard.split_units_weighted / merge_sv_shards).  The exchange runs here at world 2 over gloo
    on the GPU-free stub: the merged table must equal the unsharded one (asserted inside, reported in the line)."""
    import json
    bench = os.path.join(ROOT, "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["KIWIGPU_BENCH_PREROLL_S"] = "0.2"
    env["KIWIGPU_BENCH_WATCHDOG_S"] = "200"           # a hung rank says where and exits
    out = subprocess.run([sys.executable, bench, "--gpus", "2", "--workload", "stub", "--shard", "sv", "--full-line"], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    # the timed loop with a collective inside every step (timed_steps, as the --shard sv leg runs it): the two ranks' steps
    # take 0.2 and 0.8 ms, their own pre-roll estimates differ fourfold -- they must still have run the same number of steps
    # (round 5: they did not, and the N > 1 line hung in its strong-scaling leg)
    ts = line["shard_sv_timed_steps"]["steps_per_rank"]
    assert len(ts) == 2 and ts[0] == ts[1] and ts[0] >= 64 + 12, ts
    sv = line["shard_sv"]
    assert line["scaling"] == "strong" and sv["world"] == 2 and sv["merged_equals_unsharded"] is True
    # the cost-balanced split (shard.split_units_weighted): both kinds of SV on both ranks, a partition of the 59
    assert sorted(sv["shares"][0] + sv["shares"][1]) == list(range(59))
    assert all(any(i < 36 for i in sh) and any(i >= 36 for i in sh) for sh in sv["shares"])
    assert max(sv["load"]) <= 1.05 * sum(sv["load"]) / 2


def test_merge_sv_shards_layout():
    from flydog_sdr_gps_amd import shard
    from flydog_sdr_gps_amd._lib import result_dtype
    B, ranges = 3, shard.split_units(7, 3)                    # shares of 3, 2, 2 SVs
    full = np.zeros((B, 7), result_dtype)
    full["snr"] = np.arange(21).reshape(B, 7)
    full["dop"] = full["snr"].astype(int) - 5
    parts = np.zeros((3, B * 3), result_dtype)               # rows padded to the largest share
    for r, (lo, hi) in enumerate(ranges):
        parts[r, :B * (hi - lo)] = full[:, lo:hi].reshape(-1)
        parts[r, B * (hi - lo):]["snr"] = -1                  # slack must not leak
    assert np.array_equal(shard.merge_sv_shards(parts, B, ranges), full)


def test_bench_attributes_counter_rows_to_marked_windows(tmp_path):
    """bench.py's live HBM-traffic passes: `rocprofv3 --pmc` rows carry no timestamps, so a workload's rows are the
    ones dispatched between its two kg_ctx_mark kernels (grid size = tag).  Parser and attribution on a made-up CSV."""
    import bench
    t_acq, t_ddc = bench.pmc_tag("acq"), bench.pmc_tag("ddc14")
    rows = [("setup_kernel", 10, 5.0), ("kg_mark_kernel()", t_acq, 0.0)]
    for _ in range(bench.PMC_STEPS):
        rows += [("acq_frontend_kernel<1>", 64, 7.0), ("void acq_correlate_kernel<4, 1, true, false>(...)", 512, 100.0)]
    rows += [("kg_mark_kernel()", t_acq + 1, 0.0), ("noise", 3, 1e6), ("kg_mark_kernel()", t_ddc, 0.0)]
    for _ in range(bench.PMC_STEPS):
        rows += [("ddc_pass_a", 100, 10.0), ("ddc_pass_b", 100, 30.0)]
    rows += [("kg_mark_kernel()", t_ddc + 1, 0.0)]
    f = tmp_path / "x_counter_collection.csv"
    with open(f, "w") as fh:
        fh.write("Dispatch_Id,Kernel_Name,Grid_Size,Workgroup_Size,Counter_Name,Counter_Value\n")
        for i, (name, groups, val) in enumerate(rows):
            fh.write('%d,"%s",%d,64,FETCH_SIZE,%f\n' % (i + 1, name, groups * 64, val))
            fh.write('%d,"%s",%d,64,OTHER,%f\n' % (i + 1, name, groups * 64, 999.0))
    parsed = bench.parse_counter_rows([str(f)], "FETCH_SIZE")
    assert len(parsed) == len(rows)
    kb, top = bench.window_traffic(parsed, "acq")            # the dominant kernel, per launch
    assert kb == 100.0 and max(top, key=top.get).startswith("void acq_correlate")
    kb, top = bench.window_traffic(parsed, "ddc14")          # every kernel of the step, per step
    assert kb == 40.0 and top == {"ddc_pass_b": 30.0, "ddc_pass_a": 10.0}
    with pytest.raises(RuntimeError):
        bench.window_traffic(parsed, "wf14")                 # no such window in this pass


def test_bench_numpy_waterfall_rows_equal_the_oracle(oracle):
    """bench.py's cpu_baseline_pocketfft leg for the waterfall (scipy.fft + numpy) must be the same computation as the
    oracle's compute_frame (WF_CMA), or its timing would be of something else: rows identical on two zooms."""
    import bench
    from flydog_sdr_gps_amd import WfParams, synth, wf
    tables = (wf.window_functions(), wf.cic_comp_table())
    base = np.stack([synth.wf_iq_frame(seed=i) for i in range(2)])
    for z in (0, 5):
        p = WfParams.for_zoom(z, 1.0e6)
        fmap, drop = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped, False)
        rows = bench.wf_rows_numpy(base, p, tables[0][wf.WINF_HANNING], tables[1], fmap, p.zoom > 1)
        sc = np.full(1024, p.fft_scale, np.float32)
        for f in range(2):
            samps = oracle.wf_window_iq(base[f], tables[0][wf.WINF_HANNING])
            want = oracle.wf_compute_frame(samps, p.zoom, wf.WINF_HANNING, wf.WF_CMA, True, False, p.fft_used, p.plot_width,
                                           p.plot_width_clamped, fmap, drop, sc, (sc / np.float32(2)).astype(np.float32),
                                           p.fft_offset, tables[1], prec=0)[0]
            d = np.abs(rows[f].astype(int) - want.astype(int))
            assert d.max() <= 1 and (d == 0).mean() > 0.99


def test_radix8_form_index_math_and_swizzles():
    """tools/proto_fft8.py is the numpy model of kg_subfft4096_r8 (the 512-thread, 8-points-per-thread transform of the
    16368-lag correlator): the four Stockham passes must be the 4096-point transform, the three exchange swizzles
    bijections that leave every ds_write_b64 / ds_read_b64 of the kernel conflict-free under the gfx950 banking rules,
    and the device code's address forms (base + XOR of a per-thread constant) the same positions."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import proto_fft8 as pf
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4096) + 1j * rng.standard_normal(4096)
    for sign, ref in ((+1, np.fft.ifft(x) * 4096), (-1, np.fft.fft(x))):
        assert np.abs(pf.subfft4096_r8(x, sign) - ref).max() <= 1e-12 * np.abs(ref).max()
    assert pf.conflicts() == 0
    i = np.arange(512)
    for m in range(8):
        assert np.array_equal(pf.P0(pf.write_idx(0, i, m)), 8 * i + (m ^ ((i >> 1) & 7)))
        assert np.array_equal(pf.P1(pf.write_idx(1, i, m)), (i >> 3) * 64 + (i & 7) + 8 * (m ^ ((i >> 3) & 1)))
    for j in range(8):
        assert np.array_equal(pf.P0(i + 512 * j), 512 * j + (i ^ ((i >> 4) & 7)))
        assert np.array_equal(pf.P1(i + 512 * j), 512 * j + (i ^ (((i >> 6) & 1) << 3)))


def _have_gpu_count(n):
    try:
        import torch
        return torch.cuda.device_count() >= n
    except Exception:
        return False


# ---- waterfall host logic vs oracle -------------------------------------------
def test_wf_tables_params_maps_match_oracle(oracle):
    from flydog_sdr_gps_amd import wf
    W = wf.window_functions()
    for k in range(4):
        assert np.array_equal(W[k], oracle.wf_window(k))
    # sinc^-5 of a float-rounded sinc: numpy's sin/pow vs libm differ in the last ulps
    assert np.allclose(wf.cic_comp_table(), oracle.wf_cic_comp(), rtol=2e-6, atol=0)
    for z in range(15):
        for inv in (False, True):
            p = wf.WfParams.for_zoom(z, 3.0e5 * z + 17, spectral_inversion=inv)
            q = oracle.wf_params(z, 3.0e5 * z + 17, spectral_inversion=inv)
            assert (p.decim, p.fft_used, p.plot_width, p.plot_width_clamped, p.i_offset) == \
                (q.decim, q.fft_used, q.plot_width, q.plot_width_clamped, q.i_offset)
            assert np.float32(p.fft_scale) == np.float32(q.fft_scale)
            m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped, inv)
            m2, d2 = oracle.wf_build_maps(q.fft_used, q.plot_width, q.plot_width_clamped, inv)
            assert np.array_equal(m, m2) and np.array_equal(d, d2)
    # FlyDog's plot widths never exceed the used FFT bins
    for ui, width in ((32e6, 2000), (42e6, 1523), (52e6, 1230), (62e6, 1032)):
        for z in (0, 1, 9):
            p = wf.WfParams.for_zoom(z, 0, ui_srate=ui)
            assert abs(p.plot_width - width) <= 1 and p.plot_width <= p.fft_used


def test_wf_oracle_tone_lands_on_the_right_pixel(oracle):
    """A tone at FFT bin b must light pixel plot_width*b/fft_used (:800)."""
    from flydog_sdr_gps_amd import wf
    p = wf.WfParams.for_zoom(3, 0.0)
    m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped)
    t = np.arange(8192)
    b = 300
    iq = np.empty((8192, 2), np.int16)
    iq[:, 0] = np.rint(8000 * np.cos(2 * np.pi * b * t / 8192))
    iq[:, 1] = np.rint(8000 * np.sin(2 * np.pi * b * t / 8192))
    samps = oracle.wf_window_iq(iq, wf.window_functions()[0])
    sc = np.full(1024, p.fft_scale, np.float32)
    out, pwr, pwr_out, dB = oracle.wf_compute_frame(samps, p.zoom, 0, wf.WF_MAX, 1, 0, p.fft_used,
                                                    p.plot_width, p.plot_width_clamped, m, d, sc, sc / 2,
                                                    p.fft_offset, wf.cic_comp_table())
    assert int(np.argmax(pwr)) == b and int(np.argmax(out)) == p.plot_width * b // p.fft_used
    assert out.min() >= 55


# ---- DDC oracle self-checks -----------------------------------------------------
def test_ddc_oracle_gain_and_state_carry(oracle):
    n = 1 << 16
    t = np.arange(n)
    adc = np.rint(20000 * np.cos(2 * np.pi * 0.111 * t + 0.3)).astype(np.int16)
    inc = (-int(round(0.111 * 2 ** 48))) & ((1 << 48) - 1)
    for log2r in (4, 9):
        iq, _ = oracle.ddc_wf(adc, inc, log2r)
        z = iq[8:, 0] + 1j * iq[8:, 1]
        assert abs(np.abs(z).mean() / 20000 - 0.5) < 2e-3       # real tone -> half amplitude at DC
        assert np.abs(z - z.mean()).std() < 1.0
    whole, _ = oracle.ddc_wf(adc, inc, 6)
    st, parts = None, []
    for k in range(0, n, 7777):
        p, st = oracle.ddc_wf(adc[k:k + 7777], inc, 6, st)
        parts.append(p)
    assert np.array_equal(np.concatenate(parts), whole)
    c, s = oracle.ddc_nco_table()
    assert c[0] == 16383 and s[2048] == 16383 and c[4096] == -16383 and abs(int(c[2048])) == 0


# ---- audio front oracle self-checks ----------------------------------------------
def test_fir_oracle_is_a_linear_convolution_and_counts_like_the_reference(oracle):
    coef, coef_cic, tc = oracle.fir_design(300.0, 2700.0, 0.0, 12000.0)
    assert np.array_equal(coef, coef_cic)                        # CIC compensation off (VAL_CICF_DECIM_BY_2 == 2)
    f = np.fft.fftfreq(1024, 1 / 12000.0)
    H = np.abs(coef) * 1024
    assert abs(H[(f > 700) & (f < 2300)].mean() - 1) < 1e-3 and H[(f < 0) | (f > 3300)].max() < 1e-4
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(170 * 7) + 1j * rng.standard_normal(170 * 7)).astype(np.complex64)
    st, sizes, pos = oracle.fir_new_state(), [], []
    for k in range(7):
        o, p = oracle.fir_process(st, coef_cic, x[170 * k:170 * (k + 1)])
        sizes.append(o.size)
        pos.append(p)
    assert sizes == [0, 0, 0, 512, 0, 0, 512] and pos == [170, 340, 510, 168, 338, 508, 166]
    y, _ = oracle.fir_process(oracle.fir_new_state(), coef_cic, x)
    ref = np.convolve(x, tc[:513] * 1024)[:y.size]
    assert np.abs(y - ref).max() / np.abs(ref).max() < 1e-6
    assert oracle.fir_design(2700.0, 300.0, 0.0, 12000.0) is None
    on = oracle.fir_design(300.0, 2700.0, 0.0, 12000.0, do_cic_comp=True)
    assert not np.array_equal(on[0], on[1])


def test_unpack_oracle_sign_extension_and_swap(oracle):
    from flydog_sdr_gps_amd import snd
    raw = snd.pack_rx_iq([[-1, 2 ** 23 - 1]], [[-2 ** 23, 5]])
    r = np.float32(oracle.dpump_rescale())
    out = oracle.dpump_unpack(raw, 1, 2)
    assert out[0, 0] == np.complex64(complex(np.float32(-2 ** 23) * r, np.float32(-1) * r))      # re = q, im = i
    assert out[1, 0] == np.complex64(complex(np.float32(5) * r, np.float32(2 ** 23 - 1) * r))
    inv = oracle.dpump_unpack(raw, 1, 2, spectral_inversion=True)
    assert inv[0, 0] == np.complex64(complex(np.float32(-1) * r, np.float32(-2 ** 23) * r))
    assert abs(float(r) - 2 ** -8 * 10 ** 0.225) < 1e-9 and np.float32(snd.RESCALE) == r


# ---- committed fixtures for the waterfall / audio / DDC rows ----------------------------
GOLD = os.path.join(ROOT, "tests", "golden")


def test_golden_wf_oracle(oracle):
    from flydog_sdr_gps_amd import wf
    g = np.load(os.path.join(GOLD, "wf_golden.npz"))
    W = wf.window_functions()
    for k in range(int(g["ncases"])):
        zoom, start, interp, winf, cic, inv = g["case%d_cfg" % k]
        p = wf.WfParams.for_zoom(int(zoom), float(start), spectral_inversion=bool(inv))
        m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped, bool(inv))
        sc = np.full(1024, p.fft_scale, np.float32)
        row, _, pwr_out, dB = oracle.wf_compute_frame(
            oracle.wf_window_iq(g["case%d_iq" % k], W[int(winf)]), p.zoom, int(winf), int(interp), int(cic), 0,
            p.fft_used, p.plot_width, p.plot_width_clamped, m, d, sc, (sc / np.float32(2)).astype(np.float32),
            p.fft_offset, g["cic_comp"])
        assert np.array_equal(row, g["case%d_row" % k])
        assert np.array_equal(pwr_out, g["case%d_pwr_out" % k])


def test_golden_snd_and_ddc_oracle(oracle):
    g = np.load(os.path.join(GOLD, "snd_golden.npz"))
    assert np.array_equal(oracle.dpump_unpack(g["raw"], 8, 4, dc_i=0.5, dc_q=-0.25), g["unpack_normal"])
    assert np.array_equal(oracle.dpump_unpack(g["raw"], 8, 4, dc_i=0.5, dc_q=-0.25, spectral_inversion=True),
                          g["unpack_inverted"])
    st, outs, pos = oracle.fir_new_state(), [], []
    for k in range(7):
        o, p = oracle.fir_process(st, g["fir_coef"], g["fir_in"][170 * k:170 * (k + 1)])
        outs.append(o)
        pos.append(p)
    assert np.array_equal(np.concatenate(outs), g["fir_out"]) and pos == list(g["fir_pos"])
    d = np.load(os.path.join(GOLD, "ddc_golden.npz"))
    for l2 in (0, 4, 11):
        assert np.array_equal(oracle.ddc_wf(d["adc"], int(d["inc"]), l2)[0], d["wf_r%d" % l2])
    assert np.array_equal(oracle.ddc_rx(d["adc_rx"], int(d["inc_rx"]))[0], d["rx_records"])


def test_golden_post_oracle(oracle):
    """tests/golden/post_golden.npz (tools/make_golden.py) against the oracle built here.  The
    fixture holds libm results (log10f, powf) of the image it was made on, so floats are
    compared to 1e-6 of their scale rather than bit for bit."""
    g = np.load(os.path.join(GOLD, "post_golden.npz"))
    x, n = g["x"], g["x"].size
    for k, args in enumerate(g["agc_args"]):
        a, b = oracle.Agc(), oracle.Agc()
        a.set_parameters(*[int(v) for v in args], float(g["rate"]))
        b.set_parameters(*[int(v) for v in args], float(g["rate"]))
        cp = np.concatenate([a.process_cpx(x[i:i + 512]) for i in range(0, n, 512)])
        s16 = np.concatenate([b.process_s16(x[i:i + 512]) for i in range(0, n, 512)])
        assert np.abs(cp - g["agc_cpx_%d" % k]).max() <= 1e-6 * np.abs(cp).max()
        assert np.abs(s16.astype(int) - g["agc_s16_%d" % k].astype(int)).max() <= 1
        am = oracle.am_detect(0.0, g["agc_cpx_%d" % k])[0]
        fm = oracle.nbfm_detect((0.0, 0.0), g["agc_cpx_%d" % k])[0]
        assert np.array_equal(am, g["am_%d" % k]) and np.array_equal(fm, g["nbfm_%d" % k])   # no libm inside
    al = oracle.smeter_alpha(12000.0)
    avg = 0.0
    for i in range(0, n, 512):
        avg, taps = oracle.smeter_process(avg, al, x[i:i + 512])
    assert np.allclose([al, avg, taps[0], taps[1]], g["smeter"], rtol=1e-6, atol=1e-5)


def test_post_oracle_known_answers(oracle):
    """Closed forms for the restatement of agc.cpp / rx_sound.cpp:676-881 (no reference vectors
    exist for these): steady-state AGC level, delay, manual gain, S-meter level, detectors."""
    t = np.arange(8192)
    for amp in (300.0, 20000.0):
        a = oracle.Agc()
        a.set_parameters(True, False, -130, 50, 0, 100, 12000.0)
        x = (amp * np.exp(2j * np.pi * 0.05 * t)).astype(np.complex64)
        y = a.process_cpx(x)
        assert np.allclose(np.abs(y[-256:]), 0.7 * 32767, rtol=2e-3)               # AGC_OUTSCALE, slope 0
        assert np.abs(np.angle(y[-256:] * np.conj(x[-256 - 180:-180]))).max() < 1e-3   # 12000 * .015 samples late
        avg, _ = oracle.smeter_process(0.0, oracle.smeter_alpha(12000.0), x)
        assert abs(avg - 10 * np.log10(amp * amp / 8191.0 ** 2)) < 1e-2
    m = oracle.Agc()
    m.set_parameters(False, False, -100, 80, 6, 1000, 12000.0)
    x = (1000 * np.exp(2j * np.pi * 0.01 * t)).astype(np.complex64)
    y = m.process_cpx(x)
    assert np.allclose(y, np.float32(32767.0 * 10 ** -1.0) * x, rtol=1e-6)
    fm, last = oracle.nbfm_detect((0.0, 0.0), y)
    k = 0.340447550238101026565118445432744920253753662109375
    assert np.allclose(fm[1:], 32767 * k * np.sin(2 * np.pi * 0.01), rtol=1e-3) and last == (float(y[-1].real), float(y[-1].imag))
    assert np.all(np.abs(oracle.nbfm_detect((0.0, 0.0), (1000 * np.exp(2j * np.pi * 0.2 * t)).astype(np.complex64))[0][1:]) == 8192)
    am, z1 = oracle.am_detect(0.0, np.full(4096, 100 + 0j, np.complex64))
    assert am[0] == 100 and abs(am[-1]) < 1e-3 and abs(z1 - 100 / (1 - 0.99)) < 0.1
    assert np.array_equal(oracle.Agc().process_s16(np.zeros(4, np.complex64)), np.zeros(4, np.int16))


def test_agc_peak_is_the_window_maximum():
    """The GPU path computes m_Peak as a sliding-window maximum instead of the reference's
    running maximum with rescans (agc.cpp:193-210).  Both bookkeepings, restated here on plain
    floats, give the same sequence for any input >= -8 -- including ties, decays where the
    maximum leaves the window at every step, and the initial fill of -16."""
    rng = np.random.default_rng(2)
    for W in (1, 2, 7, 216):
        for kind in range(4):
            n = 1500
            if kind == 0:
                m = rng.uniform(-8, 0, n)
            elif kind == 1:
                m = np.linspace(-0.5, -7.5, n)                           # strictly falling
            elif kind == 2:
                m = rng.integers(-8, 0, n).astype(float)                 # many exact ties
            else:
                m = np.where(np.arange(n) % 500 < 250, -8.0, -2.0)
            m = m.astype(np.float32)
            buf, pos, peak, ref = np.full(W, -16.0, np.float32), 0, np.float32(-16.0), []
            for v in m:                                                   # the reference's bookkeeping
                tmp = buf[pos]
                buf[pos] = v
                pos = 0 if pos + 1 >= W else pos + 1
                if v > peak:
                    peak = v
                elif tmp == peak:
                    peak = max(np.float32(-8.0), buf.max())
                ref.append(peak)
            hist = np.concatenate([np.full(W, -16.0, np.float32), m])
            win = np.array([hist[j + 1:j + 1 + W].max() for j in range(n)])   # the GPU's formulation
            assert np.array_equal(np.array(ref, np.float32), win)


def test_adpcm_oracle_pinned_against_audioop(oracle):
    """The oracle's restatement of rx/csdr/ima_adpcm.cpp against CPython's audioop (the CWI IMA
    ADPCM codec the reference file descends from), an independent implementation: same codes,
    same decoder output, same final state.  The reference packs the FIRST sample of a pair into
    the LOW nibble (ima_adpcm.cpp:192-193); audioop packs it into the high one."""
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(6)
    t = np.arange(6000)
    for x in (rng.normal(0, 9000, 6000), 20000 * np.sin(t / 7.0), np.where((t // 50) % 2, 32767, -32768),
              np.zeros(6000), rng.integers(-2, 3, 6000)):
        x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
        got, st = oracle.adpcm_encode_i16(x)
        ab, ast = audioop.lin2adpcm(x.tobytes(), 2, None)
        ab = np.frombuffer(ab, np.uint8)
        assert np.array_equal(got, ((ab >> 4) | (ab << 4)) & 0xFF)
        assert (st.previous, st.index) == ast
        dec, dst = oracle.adpcm_decode_i16(got)
        assert np.array_equal(dec, np.frombuffer(audioop.adpcm2lin(ab.tobytes(), 2, None)[0], np.int16))
        assert (dst.index, dst.previous) == (st.index, st.previous) and dec[-1] == st.previous
    tab = oracle.adpcm_step_table()
    assert tab[0] == 7 and tab[88] == 32767 and np.all(np.diff(tab) > 0)
    assert np.all(np.abs(tab[1:] / tab[:-1] - 1.1) < 0.15)             # the specification's ~1.1 ratio


def test_wire_oracle_properties_and_golden(oracle):
    g = np.load(os.path.join(GOLD, "wire_golden.npz"))
    st, enc = None, []
    for i in range(0, g["audio"].size, 512):
        e, st = oracle.adpcm_encode_i16(g["audio"][i:i + 512], st)
        enc.append(e)
    assert np.array_equal(np.concatenate(enc), g["adpcm"]) and [st.index, st.previous] == list(g["adpcm_state"])
    pc, pr = oracle.wf_packet(g["row"], 123456, 7, 4242, True), oracle.wf_packet(g["row"], 123456, 7, 4242, False)
    assert np.array_equal(pc, g["pkt_compressed"]) and np.array_equal(pr, g["pkt_raw"])
    assert pc.size == 16 + 517 and pr.size == 16 + 1024 and np.array_equal(pr[16:], g["row"])
    assert bytes(pc[:4]) == b"W/F " and int.from_bytes(bytes(pc[4:8]), "little") == 123456
    assert int.from_bytes(bytes(pc[8:12]), "little") == 7 | 0x10000 and int.from_bytes(bytes(pr[8:12]), "little") == 7
    assert int.from_bytes(bytes(pc[12:16]), "little") == 4242
    # what the client decodes: 10 pad pixels then the row, within the coder's tracking error,
    # never outside 0..255; the u8 coder is the i16 coder wherever its predictor stays in 0..255
    dec, _ = oracle.adpcm_decode_u8(pc[16:])
    assert dec.size == 1034 and np.abs(dec[10:].astype(int) - g["row"].astype(int)).mean() < 6
    smooth = (128 + 40 * np.sin(np.arange(512) / 20.0)).astype(np.uint8)
    e8, _ = oracle.adpcm_encode_u8(smooth)
    e16, _ = oracle.adpcm_encode_i16(smooth.astype(np.int16))
    assert np.array_equal(e8, e16)
    assert np.array_equal(oracle.snd_header(0x10, 4242, -87.31), g["snd_header"])
    h = oracle.snd_header(0xFF, 0xA1B2C3D4, 55.0)
    assert bytes(h[:3]) == b"SND" and h[3] == 0xFF and list(h[4:8]) == [0xD4, 0xC3, 0xB2, 0xA1]
    assert (int(h[8]) << 8 | int(h[9])) == int((np.float32(3.4) + 127.0) * 10)
    assert list(oracle.snd_header(0, 0, -500.0)[8:]) == [0, 0]


def test_handoff_oracle_known_answers(oracle):
    """gps/channel.cpp:281-311 and rx/rx_waterfall.cpp:1173-1273 restated: closed-form cases."""
    o = oracle.chan_start(False, 0, 1000, 0.5)
    assert (o.lo_rate, o.ca_rate, o.ca_pause, o.code_creep) == (0x40000000, 0x10000000, 16368 - 1000, 0)   # FC/FS = 1/4, CPS/FS = 1/16
    o = oracle.chan_start(False, 8, 0, 2.0)                        # +8 bins of FS/65536 Hz
    lo_dop = 8 * 16368000 / 65536.0
    assert o.lo_dop == lo_dop and abs(o.ca_dop - lo_dop / 1540.0) < 1e-9            # L1 = 1540 x the chip rate
    assert o.lo_rate == int((4.092e6 + lo_dop) / 16.368e6 * 2 ** 32)
    assert o.code_creep == round(lo_dop / 1540.0 * 2.0 / 1.023e6 * 16.368e6) and o.ca_pause == 16368 - o.code_creep
    assert oracle.chan_start(True, 0, 65000, 0.0).ca_pause == 4 * 16368 - 65000
    flat = np.full(1024, 150, np.uint8)                            # -105 + cal(-13) = -118 dBm
    avg = oracle.aper_update(np.zeros(1024, np.float32), flat, 1, 8.0, clear=True)
    assert np.all(avg == -118) and oracle.aper_report(avg) == (-80, -120)
    step = flat.copy(); step[:] = 230                              # -38 dBm
    assert np.allclose(oracle.aper_update(avg, step, 1, 8.0), (-118 * 7 - 38) / 8.0)             # MMA
    assert np.allclose(oracle.aper_update(avg, step, 2, 4.0), -118 + 80 / 4.0)                   # EMA
    assert np.allclose(oracle.aper_update(avg, step, 0, 2.5), -118 + 80 * 0.01)                  # IIR: gain floor
    avg[100] = -17.0
    assert oracle.aper_report(avg) == (-20, -120) and oracle.aper_report(avg, 256, 768) == (-80, -120)
    assert oracle.aper_report(np.full(1024, -200, np.float32)) == (-80, -120)                    # all masked: -110 -> -80
    half = np.concatenate([np.full(512, -113, np.float32), np.full(512, -103, np.float32)])
    assert oracle.aper_report(half) == (-80, -115)                                               # tie -> lower band


def _ref_text_pins():
    """Numbers parsed from the reference's files by tools/make_ref_text_golden.py (tests/golden/ref_text_pins.json)."""
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ref_text_pins.json")))


def _cic_vh(name):
    """Structural constants of a generated verilog/rx/cic_*.vh: (N, R, Bin, Bout, integrator widths,
    comb widths, comb input truncations, (out msb, out width, rounding bit))."""
    n, r, bin_, bout, integ, comb, trunc, out = _ref_text_pins()["cic_vh"][name]
    return n, r, bin_, bout, integ, comb, trunc, tuple(out)


def test_ddc_oracle_shapes_pinned_against_reference_verilog(oracle):
    """The DDC oracle has no executable reference (FPGA fabric), but its structural constants do:
    the register widths, comb truncations and output rounding slices it uses must be the ones in
    the reference's generated CIC headers.  The checked-in cic_rx1_12k.vh was generated for
    R = 926 (kiwi.config now says 1736): same structure, and the accumulator width follows
    cic_gen.c's Bin + ceil(N log2 R) for either R."""
    n, r, bin_, bout, integ, comb, trunc, out = _cic_vh("cic_wf1.vh")
    assert (n, r, bin_, bout) == (5, 8192, 24, 16)
    assert oracle.ddc_shape(0) == [n, bin_, bout] + integ + comb + trunc + list(out)
    n, r, bin_, bout, integ, comb, trunc, out = _cic_vh("cic_rx1_12k.vh")
    assert oracle.ddc_shape(1, r) == [n, bin_, bout] + integ + comb + trunc + list(out)
    want = oracle.ddc_shape(1, 1736)                       # RX1_STD_DECIM today
    assert want[3:6] == [22 + int(np.ceil(3 * np.log2(1736))), 22 + int(np.ceil(3 * np.log2(1736))), 26] == [55, 55, 26]
    assert want[6:] == oracle.ddc_shape(1, r)[6:]          # combs and rounding do not depend on R
    n, r, bin_, bout, integ, comb, trunc, out = _cic_vh("cic_rx2_12k.vh")
    assert (n, r) == (5, 3)
    assert oracle.ddc_shape(2) == [n, bin_, bout] + integ + comb + trunc + list(out)


def test_cicf_taps_pinned_against_reference_verilog(oracle):
    """The 65-tap CICF of the audio DDC: the oracle's (and, through the bit-exact GPU tests, the
    library's) 33 stored coefficients are the table of verilog/rx/fir_iq.sv (default branch,
    N=5 R=3), whose DC gain is 2^17 to within a few LSBs (the acc[41 -: 24] slice divides by 2^18
    after the /2 decimation)."""
    import ctypes as C
    taps = _ref_text_pins()["fir_iq_sv"]["default_branch_taps"]
    L = oracle.lib()
    mine = list((C.c_int32 * 33).in_dll(L, "ko_cicf_taps65"))
    assert len(taps) == 33 and mine == taps
    signed = [t - (1 << 18) if t & (1 << 17) else t for t in taps]
    assert abs(2 * sum(signed[:32]) + signed[32] - 2 ** 17) <= 8


def test_sats_table_pinned_against_reference():
    """sats.SATS is the host mirror of Sats[] (gps/sats.cpp:25-142): the active rows (comments
    stripped), in order, with the QZSS G2 initial states read as the octal literals they are."""
    from flydog_sdr_gps_amd import sats
    ref = [tuple(r) for r in _ref_text_pins()["sats_cpp"]]
    assert ref == [tuple(r) for r in sats.SATS]
    assert len(ref) == 32 + 4 + 23 and len(ref) <= sats.MAX_SATS


def test_cpp_example_builds_against_the_header_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/search_dropin.cpp: a C++11 translation unit that includes only include/kiwigpu.h, links
    libkiwigpu.so and runs the SearchInit / Sample / Correlate / ChanStart sequence.  Here (no GPU) it
    must build, start, and stop at kg_ctx_create with the no-device error -- no CPU fallback."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    exe = os.path.join(ROOT, "examples", "search_dropin")
    f = tmp_path / "bits.bin"
    f.write_bytes(bytes(8192))
    out = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    if _have_gpu_count(1):
        assert out.returncode == 0
    else:
        assert out.returncode == 1 and "no HIP device" in out.stderr and "no CPU fallback" in out.stderr


def test_gps_timestamp_host_arithmetic_matches_oracle(oracle):
    """kg_snd_gps_begin / kg_snd_gps_stamp (host functions of libkiwigpu: rx/rx_sound.cpp:557, :636-661)
    against the oracle's restatement over a simulated stream: 170-sample data-pump buffers, the FIR's
    fir_pos sequence, AGC on and off, a week wrap, no clock solution, the first block of a connection."""
    from flydog_sdr_gps_amd import load_library, wire
    lib = load_library()
    rng = np.random.Generator(np.random.PCG64(5))
    for agc_on, clk_ticks, t0 in ((1, 123456, 1000.25), (0, 0, 604799.5), (1, 99, 3.0e5)):
        g, k = wire.GpsState(), oracle.GpsState()
        fir_pos, clk_gps = 0, t0 - 20.0
        adc, decim, nrx = 66.6666e6 + 13.7, 5555, 170
        dticks = 0.0
        for buf in range(60):
            dticks += decim * nrx + float(rng.integers(-2, 3))
            wire.gps_begin(lib, g, clk_gps, dticks + 20.0 * adc, adc, 28926.838 / adc, 1e-7)
            oracle.gps_begin(k, clk_gps, dticks + 20.0 * adc, adc, 28926.838 / adc, 1e-7)
            assert g.gpssec == k.gpssec
            fir_pos += nrx
            if fir_pos >= 512:                       # ProcessData emitted a block
                got = wire.gps_stamp(lib, g, 85, fir_pos - nrx, agc_on, 180, decim, adc, clk_gps, clk_ticks)
                want = oracle.gps_stamp(k, 85, fir_pos - nrx, agc_on, 180, decim, adc, clk_gps, clk_ticks)
                assert got == want and (g.gpssec, g.last_gpssec, g.gps_init) == (k.gpssec, k.last_gpssec, k.gps_init)
                if clk_ticks == 0 and buf > 10:
                    assert got[2] == 255
                fir_pos -= 512
        assert 0.0 <= g.gpssec < 7 * 24 * 3600.0


def test_oracle_is_clean_under_asan_and_ubsan():
    """The GPU box cannot run sanitizers; the oracle can: oracle/asan_main.c walks every family of its
    entry points (both acquisition shapes, waterfall, FIR, both DDCs and the three RX instances, AGC and
    detectors, wire formats, hand-off, GPS stamp) under -fsanitize=address,undefined."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan-run"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "asan driver ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_bench_line_helpers_without_a_gpu():
    """bench.py's round-4 line furniture: the box / build identity record (no GPU: the GPU fields stay None, the hashes are
    those of the files in the tree) and the compact per-workload table kept inside `roofline`."""
    import hashlib
    import bench
    box = bench.box_identity()
    assert set(box) >= {"host", "lib_sha16", "bench_sha16", "gpu_uuid", "gpu_name"}
    assert box["bench_sha16"] == hashlib.sha256(open(os.path.join(ROOT, "bench.py"), "rb").read()).hexdigest()[:16]
    assert box["lib_sha16"] == hashlib.sha256(open(os.path.join(ROOT, "flydog_sdr_gps_amd", "libkiwigpu.so"), "rb").read()).hexdigest()[:16]
    rs = {"acq": {"ms_per_step": 0.8, "roofline": {"frac": 0.4, "bound": "valu", "traffic": 4.0e7, "kernel_ms": 0.78},
                  "hbm": {"algorithmic_bytes_per_launch": 1.1e10}},
          "ddc14": {"ms_per_step": 0.47, "roofline": {"frac": 0.22, "bound": "valu", "traffic": 1.05e9, "kernel_ms": 0.47},
                    "hbm": {"algorithmic_bytes_per_step": 3.0e8}},
          "stub": {"ms_per_step": 1.0}}
    tab = bench.by_workload_table(rs)
    assert tab["_cols"] == ["ms_per_step", "frac", "bound", "hbm_frac_algorithmic", "traffic_over_algorithmic"]
    assert tab["acq"][:3] == [0.8, 0.4, "valu"] and abs(tab["acq"][3] - 1.1e10 / 0.78e-3 / 1e9 / 8000.0) < 1e-3
    assert abs(tab["ddc14"][4] - 3.5) < 1e-9 and tab["stub"] == [1.0, None, None, None, None]
    assert len(json.dumps(bench.by_workload_table({k: rs["acq"] for k in bench.ALL_WORKLOADS}))) < 500
    # the environment bench.py fixes before anything touches the GPU (hardware queues)
    assert os.environ.get("GPU_MAX_HW_QUEUES") is not None


def test_cpp_waterfall_example_builds_and_refuses_without_a_gpu(tmp_path):
    """examples/waterfall_dropin (compiled against include/kiwigpu.h only) parses its inputs and, on a box without a gfx950
    device, stops at kg_ctx_create with the library's no-device error: there is no CPU path behind the C ABI."""
    import struct
    import torch
    exe = os.path.join(ROOT, "examples", "waterfall_dropin")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    tb, ab = tmp_path / "t.bin", tmp_path / "a.bin"
    tb.write_bytes(struct.pack("<i", 0) + bytes(4 * 4 * 8192 + 4 * 8192))
    ab.write_bytes(bytes(2 * 8192))
    r = subprocess.run([exe, str(tb), str(ab), str(tmp_path / "o.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "kg_ctx_create" in r.stderr, r.stdout + r.stderr
    r = subprocess.run([exe, str(tb), str(tmp_path / "missing"), str(tmp_path / "o.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


# ---- round 5: no experiment code in the product, tuning switches gated, the receiver bank's surface -------------------
def test_no_knock_out_code_and_no_four_accumulator_kernel_in_the_product():
    """the knock-out builds (ACQ_KO / E1B_KO / KG_WF_KO: results wrong by construction) are gone from the
    sources, and so are the compile-time A/B switches that kept a superseded form of a kernel next to the shipped one (KG_EXP_*:
    wrong values too).  The superseded four-accumulator correlator is neither in the shipped library -- acq_correlate_kernel
    is built as <4 | 16, STAMPS> and as nothing else -- nor in the source (its template argument NQ)."""
    import glob
    import subprocess
    retired = ("KG_FUSED_TW", "ACQ_X2_SWIZZLE", "KG_DEFER_PLACE", "KG_DEFER_PLACE4", "KG_E1B_HANDOVER", "KG_E1B_EAGER_DESCRIBE",
               "KG_TILE_ST_PAIRED", "KG_WF_FUSED_TW", "KG_DDC_ONE_FORM", "KG_DDC_AHEAD", "KG_EXP_NCO", "KG_EXP_WF_LOG10F", "KG_EXP_")
    sources = glob.glob(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "*.h*"))
    assert sources
    for f in sources:
        text = open(f).read()
        assert "_KO" not in text and "KO_" not in text, f
        for name in retired:
            assert name not in text, (f, name)
    acq = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_acq.hip")).read()
    assert "acq_correlate_kernel" in acq and not re.search(r"\bNQ\b", acq)
    lib = os.path.join(ROOT, "flydog_sdr_gps_amd", "libkiwigpu.so")
    syms = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    kernels = [ln for ln in syms.splitlines() if "acq_correlate_kernel<" in ln]
    assert kernels and all(re.search(r"acq_correlate_kernel<(4|16), (false|true)>", ln) for ln in kernels), kernels[:3]


def test_tuning_variables_are_read_only_behind_kiwigpu_tuning():
    """The library's A/B switches (KIWIGPU_DDC_RUNS ...) are read through kg_tuning_env(), which answers only when
    KIWIGPU_TUNING=1: no other getenv of a KIWIGPU_ variable in the library's sources."""
    import glob
    names = set()
    for f in glob.glob(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "*.h*")):
        text = open(f).read()
        for m in re.finditer(r'(\w+)\("(KIWIGPU_[A-Z0-9_]+)"\)', text):
            fn, var = m.group(1), m.group(2)
            names.add(var)
            assert (fn == "getenv" and var == "KIWIGPU_TUNING") or fn == "kg_tuning_env", (f, fn, var)
    assert "KIWIGPU_TUNING" in names and len(names) >= 5
    common = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_common.h")).read()
    assert 'on[0] == \'1\'' in common and "kg_tuning_env" in common


def test_receiver_bank_needs_a_gpu_and_checks_its_arguments():
    import ctypes as C
    import torch
    from flydog_sdr_gps_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.kg_rxbank_create(0, 0, 1 << 22, 0, C.byref(h)) == -2          # nrx out of range: KG_ERR_INVALID, before any device call
    assert lib.kg_rxbank_create(0, 4, 100, 0, C.byref(h)) == -2              # a step shorter than a frame
    if not torch.cuda.is_available():
        assert lib.kg_rxbank_create(0, 4, 1 << 22, 0, C.byref(h)) == -1      # KG_ERR_NO_DEVICE: no CPU fallback
        assert b"no CPU fallback" in lib.kg_last_error()
    assert not h.value


def test_receiver_mixes_are_the_surveys():
    """flydog_sdr_gps_amd.rxbank.survey_mix = SURVEY.md 8(d) configs[3]: f_k = 100 kHz + k 29 kHz, zoom 8 + (k mod 4); with a
    2^22-sample step zoom 11 (R = 1024) is the overlapped sampler, zooms 8..10 the one-shot."""
    from flydog_sdr_gps_amd.ddc import rx_phase_inc
    from flydog_sdr_gps_amd.rxbank import ADC_CLOCK, UI_SRATE, light_mix, survey_mix
    mix = survey_mix(1024, 0, 1 << 22)
    hz = UI_SRATE / (1024 << 14)
    for k in (0, 1, 2, 3, 127, 128, 1023):
        p, ov, inc = mix[k]
        f = 100.0e3 + 29.0e3 * k
        assert p.zoom == 8 + k % 4 and p.decim == 1 << (p.zoom - 1) and ov == (p.zoom == 11)
        assert inc == rx_phase_inc(f, ADC_CLOCK)
        span = UI_SRATE / (1 << p.zoom)
        assert abs(p.start * hz + span / 2 - f) < 2 * hz or p.start == 0.0       # the waterfall is centred on f_k
    assert survey_mix(128, 128, 1 << 22)[0][0].i_offset == mix[128][0].i_offset  # a rank's slice is a slice of the 1024
    assert sorted(set(p.zoom for p, _, _ in light_mix(128, 0))) == list(range(1, 11))
    assert not any(ov for _, ov, _ in light_mix(128, 0))


def test_bench_summary_line_fits_and_names_every_workload():
    import bench
    r = {"ms_per_step": 1.2345, "roofline": {"frac": 0.4321, "bound": "valu", "traffic": 3.0e8}, "hbm": {"algorithmic_bytes_per_step": 1.0e8},
         "checked": {"x": 1}}
    line = {"workloads": {wl: r for wl in bench.ALL_WORKLOADS}}
    s = bench.summary_line(line)
    assert s.startswith("SUMMARY") and len(s) <= 400
    for wl in bench.ALL_WORKLOADS:
        assert wl.replace("receivers", "rx").replace("cfg2_chain", "chain") + "=1.234/0.432v/3.0x/ok" in s, (wl, s)
    assert bench.acq_flops_per_cell(16384, 4092) == 1257460 and bench.acq_flops_per_cell(16384, 16368) == 1294288


def _c_function_body(text, start):
    """The text of the braced body that opens at or after text[start]."""
    i = text.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return text[i:j]


def test_device_memory_has_one_door_and_every_create_cleans_up_through_its_destroy():
    """DESIGN.md 6.14.  hipMalloc / hipHostMalloc / hipFree / hipHostFree are called by kg_mem_alloc and kg_mem_free
    (kg_ctx.hip) and by nothing else in csrc/; the bank's own failure macros are gone; and every kg_*_create* that news an
    object calls that object's destroy (its one failure exit)."""
    import glob
    calls = re.compile(r"\bhip(?:Host)?(?:Malloc|Free)\s*\(")
    found = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "*.h*"))):
        text = open(f).read()
        assert "BANK_HIP" not in text and "BANK_TRY" not in text, f
        if os.path.basename(f) == "kg_ctx.hip":
            for name in ("kg_mem_alloc", "kg_mem_free"):
                m = re.search(r"^int %s\(" % name, text, re.M)
                assert m, name
                body = _c_function_body(text, m.start())
                assert calls.search(body), name
                text = text.replace(body, "")
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
        assert not calls.search(code), (f, calls.search(code).group(0))
        for m in re.finditer(r"^(?:static )?int (kg_\w+_create\w*)\(", text, re.M):
            body = _c_function_body(text, m.start())
            made = re.search(r"= new \(std::nothrow\) (kg_\w+)\(\)", body)
            if made:
                found += 1
                assert re.search(r"\b%s_destroy\(" % made.group(1), body), (f, m.group(1))
    assert found >= 15, found
