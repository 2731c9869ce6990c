"""Measures kg_eph_sv on the GPU against the reference's records (tests/golden/eph_ref.npz): per scenario the largest difference of
x, y, z (metres and ulp), ct (metres and ulp) and t_k (ulp of t_tx), and the share of snapshots equal in every bit.  The bars the
differences are held to are derived in tests/test_eph_cpu.py, not taken from these figures.  profiles/eph_accuracy.txt keeps the output.
usage: python tools/eph_accuracy.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, eph   # noqa: E402
from tests.test_eph_cpu import check_sv, load_golden   # noqa: E402
from tests.test_eph_gpu import segments   # noqa: E402

ctx = Context(0)
out = {"gpu": ctx.name}
for name, s in load_golden().items():
    e = eph.Ephemerides(ctx, 12)
    for binds, rows, _ in segments(s["ev"]):
        for ch, sat, kind in binds:
            e.set_sat(ch, sat, kind)
        e.push_frames([s["frames"][rows.get(ch, [])] for ch in range(12)])
    st = check_sv(e.sv(s["snaps"]), s, name)
    out[name] = {"snapshots_computed": st["n"], "bit_equal": st["equal"], "bit_equal_share": round(st["equal"] / st["n"], 4),
                 "xyz_max_m": st["xyz_m"], "xyz_max_ulp": st["xyz_ulp"], "ct_max_m": st["ct_m"], "ct_max_ulp": st["ct_ulp"], "t_k_max_ulp_of_t_tx": st["tk_ulp"]}
    e.close()
print(json.dumps(out))
