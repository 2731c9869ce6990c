"""The waterfall DDC's push planner (csrc/kg_ddc_plan.h) on the CPU, through tools/ddc_plan_host_driver.cpp: every branch of the
plan both ways, at 256 compute units and at 8 wherever the answer differs.  Every expected value below is worked out in the comment
beside it from the rules of the push as it stood before the planner was cut out of it; none is taken from the planner's output.

The rules, with CU the number of compute units:
  want = CU * 4 * 4 * 64 threads (262144 at 256 CUs, 8192 at 8);  fill = CU * 4 * 2 * 64 (131072; 4096)
  target runs = 8192, or ceil(want / nlist) if that is more, capped by max_runs; KIWIGPU_DDC_RUNS in 64 .. max_runs replaces it
  L = the smallest power of two in 64 .. 8192 with ceil(n_cover / L) <= target  (n_cover: the longest share of an R >= 2 entry, or 1)
  a call with a capture: Lw = the smallest power of two in 64 .. 1024 with sum of shares / Lw <= want; L = max(L, Lw), then doubled
  while ceil(n_cover / L) > max_runs
  pass B: small = 2 <= R <= 8, mid = 16 <= R <= 256, big = R >= 512; rest = mid then big
    beside (small and rest, second stream allowed) | staged (small * nruns >= fill, or KIWIGPU_DDC_STAGED) | one launch (some
    small) | rest;  the rest as NARROW + WIDE launches if each non-empty kind has kind * nruns >= fill, else one launch ALL
"""
import os
import re
import struct
import subprocess

import pytest

from .script_common import ROOT, build_driver

NONE, AGE, OUT_STRIDE, COMB_WGS, NRUNS = range(5)              # DDC_REFUSE_*
B_NONE, B_BESIDE, B_STAGED, B_ONE, B_REST = range(5)           # DDC_B_*
SEL_RUN, SEL_SMALL, SEL_REST = range(3)
ALL, NARROW, WIDE = range(3)


def E(chan, R, cnt=0, age=0, stale=0, max_out=0, out_off=0):
    return (chan, R.bit_length() - 1, cnt, age, stale, max_out, out_off)


def GO(n, cus, max_runs, out_stride=None, plan_pass=0, runs="-", side="-", staged="-"):
    return (n, (n + 8) if out_stride is None else out_stride, cus, max_runs, plan_pass, runs, side, staged)


R7 = [E(i, R, cnt=3) for i, R in enumerate((1, 2, 8, 16, 256, 512, 8192))]
STEP = [E(0, 16, cnt=9, max_out=100, out_off=7), E(1, 8192, cnt=77, max_out=8192), E(2, 4, cnt=1)]
AGES = [E(4, 8, cnt=5, age=5000), E(2, 8, cnt=1, age=1000), E(9, 1, age=3000)]
MIDBIG = lambda nmid, nbig: [E(i, 64) for i in range(nmid)] + [E(nmid + i, 1024) for i in range(nbig)]
CASES = {
    # max_runs is what kg_ddc_create derives: min(ceil(max_samples / 64), 16384)
    "r32x14_256": ([E(i, 32) for i in range(14)], GO(1 << 22, 256, 16384)),
    "r32x14_8": ([E(i, 32) for i in range(14)], GO(1 << 22, 8, 16384)),
    "r32x14_runs4096": ([E(i, 32) for i in range(14)], GO(1 << 22, 256, 16384, runs=4096)),
    "r32x14_runs63": ([E(i, 32) for i in range(14)], GO(1 << 22, 256, 16384, runs=63)),
    "r32x14_runs20000": ([E(i, 32) for i in range(14)], GO(1 << 22, 256, 16384, runs=20000)),
    "bypass_only": ([E(0, 1)], GO(1000, 256, 16384)),
    "r7_256": (R7, GO(65536, 256, 1024)),
    "r7_8": (R7, GO(65536, 8, 1024)),
    "r7_side0": (R7, GO(65536, 256, 1024, side=0)),
    "r7_side0_staged1": (R7, GO(65536, 256, 1024, side=0, staged=1)),
    "r64_long_256": ([E(0, 64)], GO((1 << 24) + 1, 256, 16384)),
    "r64_long_8": ([E(0, 64)], GO((1 << 24) + 1, 8, 16384)),
    "r64_1024_runs": ([E(0, 64)], GO(1 << 24, 256, 16384)),
    "step_256": (STEP, GO(1 << 22, 256, 16384)),
    "step_8": (STEP, GO(1 << 22, 8, 16384)),
    "ch20_fit": ([E(i, 32) for i in range(20)], GO(13108 * 64, 256, 16384)),
    "ch20_over": ([E(i, 32) for i in range(20)], GO(13108 * 64 + 1, 256, 16384)),
    "ch32_fit": ([E(i, 32) for i in range(32)], GO(13108 * 64, 256, 16384)),
    "small4_8": ([E(i, 2) for i in range(4)], GO(65536, 8, 1024)),
    "small3_8": ([E(i, 2) for i in range(3)], GO(65536, 8, 1024)),
    "small4_256": ([E(i, 2) for i in range(4)], GO(65536, 256, 1024)),
    "small4_8_staged0": ([E(i, 2) for i in range(4)], GO(65536, 8, 1024, staged=0)),
    "staged1_no_small": ([E(0, 64)], GO(65536, 8, 1024, staged=1)),
    "mid4_big4_8": (MIDBIG(4, 4), GO(65536, 8, 1024)),
    "mid4_big3_8": (MIDBIG(4, 3), GO(65536, 8, 1024)),
    "mid4_big4_256": (MIDBIG(4, 4), GO(65536, 256, 1024)),
    "cap_maxruns": ([E(0, 16, max_out=4096)], GO(65536, 8, 100)),
    "nocap_maxruns": ([E(0, 16)], GO(65536, 8, 100)),
    "ages": (AGES, GO(4096, 256, 1024)),
    "stale_plan": ([E(4, 8, cnt=5, age=7777, stale=1), E(2, 8, cnt=2, age=100)], GO(4096, 256, 1024, plan_pass=1)),
    "stale_real": ([E(4, 8, cnt=5, age=7777, stale=1), E(2, 8, cnt=2, age=100)], GO(4096, 256, 1024)),
    "stale_after_reset": ([E(4, 8), E(2, 8, cnt=2, age=100)], GO(4096, 256, 1024)),
    "stale_capture": ([E(4, 8, cnt=5, age=7777, stale=1, max_out=10), E(2, 8, cnt=2, age=100)], GO(4096, 256, 1024, plan_pass=1)),
    "n1": ([E(0, 1), E(1, 2, cnt=1), E(2, 2, cnt=0)], GO(1, 256, 1)),
    "age_plan": ([E(0, 2, age=(1 << 62) - 100), E(1, 2)], GO(100, 256, 1024, plan_pass=1)),
    "age_real": ([E(0, 2, age=(1 << 62) - 100), E(1, 2)], GO(100, 256, 1024)),
    "age_below": ([E(0, 2, age=(1 << 62) - 101), E(1, 2)], GO(100, 256, 1024, plan_pass=1)),
    "stride": ([E(0, 2, cnt=1), E(1, 4, out_off=1028), E(2, 1)], GO(4096, 256, 1024, out_stride=2051)),
    "stride_fits": ([E(0, 2, cnt=1), E(1, 4, out_off=2), E(2, 1, out_off=0)], GO(1024, 256, 1024, out_stride=1026)),
    "comb_wgs": ([E(0, 2)], GO(1 << 42, 256, 16384, out_stride=1 << 42)),
    "nruns": ([E(0, 64)], GO((1 << 27) + 1, 256, 16384)),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ddc_plan")
    exe = build_driver(tmp, "ddc_plan_host_driver")
    lines = []
    for entries, go in CASES.values():
        lines += ["e " + " ".join(str(v) for v in e) for e in entries] + ["go " + " ".join(str(v) for v in go)]
    script = os.path.join(str(tmp), "cases.txt")
    open(script, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([exe, script], capture_output=True, text=True, check=True).stdout
    parsed = []
    for ln in out.splitlines():
        name, *vals = ln.split()
        if name == "case":
            parsed.append({"launch": []})
        elif name == "launch":
            parsed[-1]["launch"].append(tuple(int(v) for v in vals))
        elif name == "block":
            parsed[-1]["block"] = bytes.fromhex(vals[0]) if vals else b""
        else:
            parsed[-1][name] = [int(v) for v in vals]
    assert len(parsed) == len(CASES)
    return dict(zip(CASES, parsed))


def runs_of(p):
    """(L, nruns, gx, pass A narrow)"""
    n_cover, L, log2L, nruns = p["runs"]
    assert 1 << log2L == L
    return L, nruns, p["pass_a"][0], p["pass_a"][1]


def test_few_channels_raise_the_target_and_max_runs_caps_it(plans):
    # 14 x R = 32, n = 2^22, 256 CUs: ceil(262144 / 14) = 18725 > 8192, capped by max_runs 16384.  L: 64 -> 65536 runs, 128 -> 32768,
    # 256 -> 16384 <= 16384.  gx = 16384 / 256 = 64.  L <= 1024: pass A narrow.
    p = plans["r32x14_256"]
    assert p["refusal"] == [NONE, -1] and runs_of(p) == (256, 16384, 64, 1) and p["runs"][0] == 1 << 22
    # outputs 2^22 / 32 = 131072 each: 2 planes x 131072 words x 14 = 3670016; 131072 / 1024 = 128 comb workgroups x 14 = 1792
    assert p["nouts"] == [131072] * 14 and p["sizes"] == [14, 0, 3670016, 1792, 0]
    assert p["c0off"] == [262144 * i for i in range(14)] and p["wgoff"] == [128 * i for i in range(15)]
    # all of them mid (16 <= R <= 256), no small: form rest; 14 x 16384 = 229376 >= 131072 and no big: split, one NARROW launch
    assert p["pass_b"] == [B_REST, 1, 1] and p["launch"] == [(SEL_REST, 0, 14, NARROW, 0, 0)]
    assert p["bypass"] == [] and p["small"] == [] and p["run"] == p["rest"] == list(range(14)) and p["bypass_kernel"] == [0, 0]
    # 8 CUs: ceil(8192 / 14) = 586 < 8192: target 8192.  256 -> 16384 > 8192, 512 -> 8192.  gx 32.  fill 4096: still split.
    q = plans["r32x14_8"]
    assert runs_of(q) == (512, 8192, 32, 1) and q["pass_b"] == [B_REST, 1, 1] and q["block"] == p["block"]
    # 20 channels: ceil(262144 / 20) = 13108, under the cap: n = 13108 x 64 fits runs of 64 exactly, one sample more does not
    assert runs_of(plans["ch20_fit"])[:2] == (64, 13108)
    assert runs_of(plans["ch20_over"])[:2] == (128, 6555)              # ceil(838913 / 128)
    # 32 channels: 262144 / 32 = 8192 is not more than 8192: 838912 / 64 = 13108 > 8192, 128 -> 6554
    assert runs_of(plans["ch32_fit"])[:2] == (128, 6554)


def test_the_runs_switch_replaces_the_target_only_inside_its_range(plans):
    assert runs_of(plans["r32x14_runs4096"])[:3] == (1024, 4096, 16)   # 2^22 / 4096
    for name in ("r32x14_runs63", "r32x14_runs20000"):                 # below 64, above max_runs: ignored
        assert runs_of(plans[name])[:2] == (256, 16384)


def test_long_runs_take_the_wide_pass_a(plans):
    # one R = 64, n = 2^24 + 1, 256 CUs: target min(262144, 16384).  1024 -> ceil(16777217 / 1024) = 16385 > 16384, 2048 -> 8193.
    # gx = ceil(8193 / 256) = 33.  L > 1024: every form of pass A.
    assert runs_of(plans["r64_long_256"]) == (2048, 8193, 33, 0)
    # 8 CUs: target 8192: 2048 -> 8193 > 8192, 4096 -> 4097; gx 17
    assert runs_of(plans["r64_long_8"]) == (4096, 4097, 17, 0)
    # the last narrow one: n = 2^24 in 16384 runs of 1024
    assert runs_of(plans["r64_1024_runs"]) == (1024, 16384, 64, 1)
    assert plans["r64_long_256"]["nouts"] == [262144]


def test_bypass_only(plans):
    # no R >= 2 entry: n_cover 1, one run of 64, nothing for pass A or B; ceil(1000 / 4096) = 1 bypass block, in line
    p = plans["bypass_only"]
    assert p["runs"] == [1, 64, 6, 1] and p["pass_a"][0] == 1 and p["pass_b"] == [B_NONE, 1, 0] and p["launch"] == []
    assert p["bypass"] == [0] and p["run"] == [] and p["bypass_kernel"] == [0, 1] and p["nouts"] == [1000]
    assert p["sizes"] == [0, 0, 0, 0, 1000]


def test_seven_rates_beside(plans):
    p = plans["r7_256"]
    # (3 + 65536) >> log2 R
    assert p["nouts"] == [65539, 32769, 8192, 4096, 256, 128, 8]
    # planes of (nouts + 3) & ~3 words, two per R >= 2 entry: 65544, 16384, 8192, 512, 256, 16
    assert p["c0off"] == [0, 0, 65544, 81928, 90120, 90632, 90888] and p["sizes"][2] == 90904
    # ceil(nouts / 1024) comb workgroups: 33, 8, 4, 1, 1, 1
    assert p["wgoff"] == [0, 0, 33, 41, 45, 46, 47, 48] and p["sizes"][3] == 48
    assert p["bypass"] == [0] and p["run"] == [1, 2, 3, 4, 5, 6] and p["small"] == [1, 2] and p["rest"] == [3, 4, 5, 6] and p["sizes"][0] == 2
    # ceil(262144 / 7) = 37450, capped by max_runs 1024; 65536 / 64 = 1024 runs; gx 4
    assert runs_of(p) == (64, 1024, 4, 1)
    # small and rest: beside; 2 x 1024 < 131072: one ALL launch for the rest; 65536 / 4096 = 16 bypass blocks on the second stream
    assert p["pass_b"] == [B_BESIDE, 0, 2] and p["launch"] == [(SEL_SMALL, 0, 2, ALL, 1, 1), (SEL_REST, 0, 4, ALL, 0, 0)]
    assert p["bypass_kernel"] == [1, 16]
    # 8 CUs: target 8192 (not capped: it is not raised), 1024 runs of 64 all the same; 2048 < 4096: no split; 16 <= 32 blocks
    q = plans["r7_8"]
    assert runs_of(q) == (64, 1024, 4, 1) and q["pass_b"] == p["pass_b"] and q["launch"] == p["launch"] and q["bypass_kernel"] == [1, 16]
    # KIWIGPU_DDC_SIDE=0: nothing beside; 2 x 1024 < fill: not staged, a few small entries: everything in one launch
    s = plans["r7_side0"]
    assert s["pass_b"] == [B_ONE, 0, 1] and s["launch"] == [(SEL_RUN, 0, 6, ALL, 0, 0)] and s["bypass_kernel"] == [0, 16]
    # ... and KIWIGPU_DDC_STAGED=1: the staged launch in line, then the rest
    t = plans["r7_side0_staged1"]
    assert t["pass_b"] == [B_STAGED, 0, 2] and t["launch"] == [(SEL_SMALL, 0, 2, ALL, 1, 0), (SEL_REST, 0, 4, ALL, 0, 0)]
    assert p["block"] == q["block"] == s["block"] == t["block"]


def test_staged_by_fill_and_by_switch(plans):
    # R = 2 entries alone, 1024 runs, 8 CUs (fill 4096): 4 x 1024 fills, 3 x 1024 does not; 256 CUs (131072): 4 do not
    assert plans["small4_8"]["pass_b"][0] == B_STAGED and plans["small4_8"]["launch"] == [(SEL_SMALL, 0, 4, ALL, 1, 0)]
    assert plans["small3_8"]["pass_b"][0] == B_ONE and plans["small3_8"]["launch"] == [(SEL_RUN, 0, 3, ALL, 0, 0)]
    assert plans["small4_256"]["pass_b"][0] == B_ONE
    assert plans["small4_8_staged0"]["pass_b"][0] == B_ONE             # the switch says no
    assert plans["staged1_no_small"]["pass_b"][0] == B_REST            # the switch says yes, but there is nothing to stage


def test_the_rest_splits_when_both_kinds_fill(plans):
    # 1024 runs, 8 CUs: 4 x 1024 >= 4096 for both kinds; three big ones do not fill; at 256 CUs nothing does
    assert plans["mid4_big4_8"]["pass_b"] == [B_REST, 1, 2]
    assert plans["mid4_big4_8"]["launch"] == [(SEL_REST, 0, 4, NARROW, 0, 0), (SEL_REST, 4, 4, WIDE, 0, 0)]
    assert plans["mid4_big3_8"]["pass_b"] == [B_REST, 0, 1] and plans["mid4_big3_8"]["launch"] == [(SEL_REST, 0, 7, ALL, 0, 0)]
    assert plans["mid4_big4_256"]["pass_b"] == [B_REST, 0, 1] and plans["mid4_big4_256"]["launch"] == [(SEL_REST, 0, 8, ALL, 0, 0)]
    assert plans["mid4_big4_8"]["sizes"][0] == 4 and plans["mid4_big4_8"]["rest"] == list(range(8))


def test_step_call_with_captures(plans):
    p = plans["step_256"]
    # shares: 100 x 16 = 1600; 8192 x 8192 = 2^26, cut to n; the continuous entry all of n
    assert p["nlim"] == [1600, 4194304, 4194304]
    # a capture counts from zero: 1600 >> 4, 2^22 >> 13; continuous: (1 + 2^22) >> 2
    assert p["nouts"] == [100, 512, 1048576] and p["reset"] == [1, 1, 0] and p["outoff"] == [7, 0, 0] and p["will_reset"] == [0, 0, 0]
    assert p["c0off"] == [0, 200, 1224] and p["wgoff"] == [0, 1, 2, 1026] and p["sizes"] == [1, 1, 2098376, 1026, 0]
    # target min(ceil(262144 / 3), 16384): L 256 for the 2^22 share.  Total work 1600 + 2 x 2^22 = 8390208: / 64 = 131097 <= 262144, Lw 64.
    assert runs_of(p) == (256, 16384, 64, 1)
    # small {2}, rest {0 | 1}: beside; one mid x 16384 < 131072: no split
    assert p["small"] == [2] and p["rest"] == [0, 1] and p["pass_b"] == [B_BESIDE, 0, 2]
    assert p["launch"] == [(SEL_SMALL, 0, 1, ALL, 1, 1), (SEL_REST, 0, 2, ALL, 0, 0)]
    # 8 CUs: target 8192: L 512.  Total work: / 64 = 131097, / 128 = 65548, / 256 = 32774, / 512 = 16387 all > 8192: Lw stops at 1024.
    q = plans["step_8"]
    assert runs_of(q) == (1024, 4096, 16, 1) and q["block"] == p["block"]


def test_capture_sizing_is_capped_by_max_runs(plans):
    # one capture of 4096 x 16 = 65536 samples, 8 CUs, max_runs 100: L 64 by the target (1024 <= 8192), Lw 64 (1024 <= 8192), then
    # doubled while ceil(65536 / L) > 100: 512 -> 128, 1024 -> 64
    assert plans["cap_maxruns"]["refusal"] == [NONE, -1] and runs_of(plans["cap_maxruns"]) == (1024, 64, 1, 1)
    # the same share without a capture has no such rule: 1024 runs > 100 is refused
    assert plans["nocap_maxruns"]["refusal"] == [NRUNS, -1] and plans["nocap_maxruns"]["runs"] == [65536, 64, 6, 1024]


def test_unequal_ages(plans):
    p = plans["ages"]
    # the youngest age, and what each entry has on top of it
    assert p["ages"] == [1000, 0] and p["pdelta"] == [4000, 0, 2000] and p["list"] == [4, 2, 9]
    assert p["nouts"] == [(5 + 4096) >> 3, (1 + 4096) >> 3, 4096]


def test_stale_entry_of_a_continuous_push(plans):
    # PLAN pass: the entry is planned as the reset will leave it: age 0 (so the youngest), counter 0
    p = plans["stale_plan"]
    assert p["will_reset"] == [1, 0] and p["ages"] == [0, 0] and p["pdelta"] == [0, 100] and p["nouts"] == [4096 >> 3, (2 + 4096) >> 3]
    # outside one the push has reset the channel before it plans: the same tables either way
    r, a = plans["stale_real"], plans["stale_after_reset"]
    assert a["will_reset"] == [0, 0] and a["block"] == p["block"] == r["block"] and a["nouts"] == p["nouts"]
    # a capture resets by itself and leaves the reference point alone
    c = plans["stale_capture"]
    assert c["will_reset"] == [0, 0] and c["ages"] == [100, 0] and c["pdelta"] == [7677, 0] and c["nouts"] == [10, (2 + 4096) >> 3]


def test_one_sample(plans):
    p = plans["n1"]
    # R = 1: 1 output; R = 2 at count 1: (1 + 1) >> 1 = 1; at count 0: none
    assert p["nouts"] == [1, 1, 0] and p["runs"] == [1, 64, 6, 1] and p["pass_a"] == [1, 1]
    assert p["c0off"] == [0, 0, 8] and p["wgoff"] == [0, 0, 1, 1] and p["sizes"] == [0, 0, 8, 1, 1]
    assert p["pass_b"] == [B_ONE, 1, 1] and p["launch"] == [(SEL_RUN, 0, 2, ALL, 0, 0)] and p["bypass_kernel"] == [1, 1]


def test_refusals(plans):
    # the oldest age + n reaches 2^62: a PLAN pass cannot rebase
    assert plans["age_plan"]["refusal"] == [AGE, -1]
    assert plans["age_real"]["refusal"] == [NONE, -1] and plans["age_real"]["ages"] == [0, 1]
    assert plans["age_below"]["refusal"] == [NONE, -1] and plans["age_below"]["ages"] == [0, 0]
    # entry 1: 4096 >> 2 = 1024 outputs at offset 1028 > 2051; entry 0 has its count, (1 + 4096) >> 1 = 2048 <= 2051
    assert plans["stride"]["refusal"] == [OUT_STRIDE, 1] and plans["stride"]["nouts"] == [2048, 1024]
    assert plans["stride_fits"]["refusal"] == [NONE, -1] and plans["stride_fits"]["nouts"] == [512, 256, 1024]
    # 2^42 >> 1 = 2^41 outputs = 2^31 comb workgroups
    assert plans["comb_wgs"]["refusal"] == [COMB_WGS, -1] and plans["comb_wgs"]["sizes"][3] == 1 << 31
    # ceil((2^27 + 1) / 8192) = 16385 > 16384
    assert plans["nruns"]["refusal"] == [NRUNS, -1] and plans["nruns"]["runs"] == [(1 << 27) + 1, 8192, 13, 16385]
    # and kg_ddc.hip answers them with the statuses and texts the push has always had, in this order
    text = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_ddc.hip")).read()
    got = re.findall(r'KG_REQUIRE\(P\.refusal != DDC_REFUSE_(\w+), (KG_ERR_\w+),\s*"([^"]*)"', text)
    assert got == [("AGE", "KG_ERR_STATE", "kg_ddc_wf_push_dev: 2^62 samples since a channel was last set"),
                   ("OUT_STRIDE", "KG_ERR_INVALID", "kg_ddc_wf_push_dev: out_stride %zu < %ld outputs of channel %d (at offset %ld)"),
                   ("COMB_WGS", "KG_ERR_INVALID", "kg_ddc_wf_push_dev: too many outputs in one call"),
                   ("NRUNS", "KG_ERR_INVALID", "kg_ddc_wf_push_dev: %d runs > %d")]


def test_the_block_is_the_tables_in_order_at_16_byte_alignment(plans):
    order = (("c0off", "q"), ("nouts", "q"), ("nlim", "q"), ("pdelta", "Q"), ("list", "i"), ("wgoff", "i"), ("bypass", "i"), ("run", "i"),
             ("small", "i"), ("rest", "i"), ("reset", "i"), ("outoff", "q"))
    checked = 0
    for name, p in plans.items():
        if p["refusal"][0] != NONE:
            assert "block" not in p
            continue
        block, offsets = b"", []
        for tab, fmt in order:
            block += b"\0" * (-len(block) % 16)        # (an empty table still moves the end up to the boundary)
            offsets.append(len(block))
            block += struct.pack("<%d%s" % (len(p[tab]), fmt), *p[tab])
        assert p["block"] == block and p["offsets"] == offsets, name
        assert len(p["wgoff"]) == len(p["list"]) + 1
        checked += 1
    assert checked >= 30
    # one R = 1 entry: 8 + 8 pad, 8 + 8, 8 + 8, 8 + 8, 4 + 12, 8 + 8, 4 + 12 (bypass), three empty tables, 4 + 12 (reset), 8 (outoff, unpadded)
    assert plans["bypass_only"]["offsets"] == [0, 16, 32, 48, 64, 80, 96, 112, 112, 112, 112, 128] and len(plans["bypass_only"]["block"]) == 136
