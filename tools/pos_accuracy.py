"""Measures kg_pos_solve on the GPU against the reference's records (tests/golden/pos_ref.npz): per scenario and output quantity the
largest difference from the reference beside the bar it is held to (where the ratio of the two is largest), and the share of epochs
whose whole record is equal in every bit.  The bars are derived in tests/test_pos_cpu.py from the golden alone (8 x the reference's own
envelope under +-4 ulp of input, floor 2 ulp), not taken from these figures.  profiles/pos_accuracy.txt keeps the output.
usage: python tools/pos_accuracy.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context   # noqa: E402
from tests.test_pos_cpu import discrete_equal, load_golden, same_bits, within_bars   # noqa: E402
from tests.test_pos_gpu import run_device   # noqa: E402

ctx = Context(0)
out = {"gpu": ctx.name}
for name, s in load_golden().items():
    got, _ = run_device(ctx, s, False)
    discrete_equal(got, s["epochs"], name)
    stats = within_bars(got, s, name)
    equal = sum(same_bits(got[e:e + 1], s["epochs"][e:e + 1]) is None for e in range(len(got)))
    out[name] = {"epochs": len(got), "bit_equal_epochs": equal, "envelope": s["env"],
                 "max_error_and_bar": {q: {"error": v[0], "bar": v[1]} for q, v in stats.items()}}
print(json.dumps(out))
