"""The position fix without a GPU: kg_pos.h's host build (tools/pos_host_driver.cpp, plain and under the address / undefined-behaviour
sanitizers, a stand-alone program) against the reference's own records (tests/golden/pos_ref.npz, made by tools/make_ref_pos_golden.py
from gps/PosSolver.cpp, its solver headers, TNT / JAMA and the statements cut from gps/solve.cpp) -- every bit of every output and of the
solvers' state --, what the golden holds, the pinned constants, the scene builder and the exported symbols.

The bars of the DEVICE's continuous outputs (tests/test_pos_gpu.py) are made here, from the golden alone: the generator
reran the reference 16 times per scenario with every finite x, y, z input moved by an independent random -4 .. +4 ulp and recorded, per
output quantity, the largest deviation from the unperturbed run (`env`).  bar = max(8 env, floor), the floor 2 ulp of the reference value:
for t_rx 2 ulp(ct_rx) / c, for osc_corr that over the epoch's dt."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import eph, pos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pos_ref.npz")
POS_SYMBOLS = {"kg_pos_create": 5, "kg_pos_destroy": 1, "kg_pos_set_mode": 3, "kg_pos_reset": 1, "kg_pos_solve_dev": 8, "kg_pos_solve": 8,
               "kg_pos_get_state": 3}
FIX_Q, SAT_Q = ("x", "y", "z", "t_rx", "osc_corr", "lambda", "phi", "alt"), ("elev_deg", "azim_deg")
NROW = 12


def load_golden():
    g = np.load(GOLDEN)
    quant = [str(q) for q in g["quant"]]
    assert tuple(quant) == FIX_Q + SAT_Q
    out = {}
    for name in g["names"]:
        name = str(name)
        ne = len(g[name + "_ticks"])
        out[name] = dict(snaps=g[name + "_snaps"].copy().view(eph.snap_dtype).reshape(ne, NROW), sv=g[name + "_sv"].copy().view(eph.sv_dtype).reshape(ne, NROW),
                         ticks=g[name + "_ticks"].copy(), skip=g[name + "_skip"].copy(), mode=g[name + "_mode"].copy(), reset=g[name + "_reset"].copy(),
                         epochs=g[name + "_epochs"].copy().view(pos.epoch_dtype).reshape(ne), states=g[name + "_states"].copy().view(pos.state_dtype).reshape(ne, 3),
                         env=dict(zip(quant, (float(v) for v in g[name + "_env"]))))
    return out


def segments(s):
    """-> [(reset before, (use_kalman, plot_e1b), first epoch, end)]: runs of epochs one call may take"""
    out, mode = [], (1, 0)
    for e in range(len(s["ticks"])):
        m = tuple(int(v) for v in s["mode"][e])
        if not out or s["reset"][e] or m != mode:
            out.append([bool(s["reset"][e]), m, e, e + 1])
            mode = m
        else:
            out[-1][3] = e + 1
    return [tuple(x) for x in out]


def same_bits(a, b):
    """structured arrays equal in every bit, any NaN equal to any NaN -> None, or the first field that differs"""
    assert a.dtype == b.dtype and a.shape == b.shape
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.names:
            d = same_bits(x, y)
            if d:
                return name + "." + d
        elif x.dtype.kind == "f":
            nan = np.isnan(x)
            if not (np.array_equal(nan, np.isnan(y)) and np.array_equal(x[~nan].view(np.uint64), y[~nan].view(np.uint64))):
                return name
        elif not np.array_equal(x, y):
            return name
    return None


def discrete_equal(got, want, what):
    """flags, ekf_running, nsv, chans, sat, ch, type, week, el, az, grn_yel_red, ch_has_soln and NaN-ness"""
    for n in ("flags", "ekf_running", "nsv"):
        assert np.array_equal(got["fix"][n], want["fix"][n]), (what, n, got["fix"][n].tolist(), want["fix"][n].tolist())
    for n in ("sat", "ch", "type", "week", "el", "az"):
        assert np.array_equal(got["sat"][n], want["sat"][n]), (what, n)
    for n in ("chans", "grn_yel_red", "ch_has_soln"):
        assert np.array_equal(got[n], want[n]), (what, n)
    for n in FIX_Q:
        assert np.array_equal(np.isnan(got["fix"][n]), np.isnan(want["fix"][n])), (what, n)
    for n in SAT_Q:
        assert np.array_equal(np.isnan(got["sat"][n]), np.isnan(want["sat"][n])), (what, n)


def bars(s):
    """per quantity an array shaped like the golden's: max(8 env, 2 ulp floor), from the golden alone"""
    want, env = s["epochs"], s["env"]
    ct_rx = np.abs(want["fix"]["t_rx"]) * pos.C_LIGHT
    with np.errstate(invalid="ignore"):
        floor_t = 2 * np.spacing(ct_rx) / pos.C_LIGHT
    tk = s["ticks"].astype(np.float64)
    dt = np.diff(tk, prepend=tk[0] - pos.F_OSC)
    dt = np.where(dt < 0, dt + 2.0 ** 48, dt) / pos.F_OSC                # the epoch's dt, 48-bit wrap undone
    out = {}
    for q in FIX_Q:
        v = want["fix"][q]
        with np.errstate(invalid="ignore"):
            floor = 2 * np.spacing(np.abs(v))
        if q == "t_rx":
            floor = floor_t
        elif q == "osc_corr":
            floor = np.maximum(floor, floor_t / dt[:, None])
        out[q] = np.maximum(8 * env[q], floor)
    for q in SAT_Q:
        with np.errstate(invalid="ignore"):
            out[q] = np.maximum(8 * env[q], 2 * np.spacing(np.abs(want["sat"][q])))
    return out


def within_bars(got, s, what):
    """the continuous outputs against the golden under bars(s) -> {quantity: (largest error, its bar)}"""
    b, want, stats = bars(s), s["epochs"], {}
    for q in FIX_Q + SAT_Q:
        g, w = (got["sat"][q], want["sat"][q]) if q in SAT_Q else (got["fix"][q], want["fix"][q])
        ok = np.isfinite(w)
        err = np.abs(g[ok] - w[ok])
        over = err > b[q][ok]
        k = int(np.argmax(np.divide(err, b[q][ok], out=np.zeros_like(err), where=b[q][ok] > 0))) if err.size else 0
        stats[q] = (float(err[k]), float(b[q][ok][k])) if err.size else (0.0, 0.0)
        assert not over.any(), (what, q, "error %.3g over its bar %.3g" % (err[over][0], b[q][ok][over][0]))
    return stats


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_golden_holds_what_the_generator_promised(golden):
    m, w, t = golden["main"], golden["week"], golden["step"]
    f0 = m["epochs"]["fix"][:, 0]
    spp, ekf, called = (f0["flags"] & pos.SPP_VALID) != 0, (f0["flags"] & pos.EKF_VALID) != 0, (f0["flags"] & pos.CALLED) != 0
    assert np.any((f0["nsv"] == 4) & spp) and np.any((f0["nsv"] == 3) & ~spp & ekf & called) and np.any((f0["nsv"] == 12) & spp & ekf)
    kinds = pos.kinds_table()
    gated = [e for e in range(len(f0)) if np.any(m["sv"][e]["flags"] & eph.SV_POWER) and not np.all(m["sv"][e]["flags"] & eph.SV_POWER)]
    e = gated[0]                                                        # the index quirk: Galileo rows behind the gated one count as Navstar
    enter = [r for r in range(NROW) if not m["sv"][e][r]["flags"] & (eph.SV_NOT_VALID | eph.SV_POWER)]
    assert sum(kinds[m["snaps"][e][r]["sat"]] == eph.E1B for r in enter) == 4 and m["epochs"]["fix"][e, 2]["nsv"] == 0 and m["epochs"]["fix"][e, 1]["nsv"] == 11
    bad = [e for e in range(len(f0)) if np.any(m["sv"][e]["flags"] & eph.SV_BAD)][0]
    assert ekf[bad - 1] and ekf[bad] and not spp[bad] and np.isnan(m["epochs"]["sat"][bad]["elev_deg"]).sum() == 1
    bad = [e for e in range(len(w["ticks"])) if np.any(w["sv"][e]["flags"] & eph.SV_BAD)][0]
    assert w["epochs"]["fix"][bad, 0]["ekf_running"] == -1 and w["mode"][bad][0] == 0
    run = f0["ekf_running"]
    assert any(run[k - 1] >= 1 and run[k] == -1 and called[k] and run[k + 1] >= 0 for k in range(1, len(run) - 1))       # loss and restart
    none = [k for k in range(1, len(f0)) if m["epochs"]["chans"][k] == 0]
    assert len(none) >= 2 and all(f0["flags"][k] & pos.POS_VALID and not called[k] for k in none)
    f2 = m["epochs"]["fix"][:, 2]
    assert np.any((f2["nsv"] >= 1) & (f2["nsv"] < 4) & ((f2["flags"] & pos.CALLED) != 0))
    sat = m["epochs"]["sat"][ekf | spp]
    live = sat[(sat["elev_deg"] != 0) | (sat["azim_deg"] != 0)]
    rej = live[(live["el"] == 0) & (live["az"] == 0)]
    assert np.any(np.round(rej["azim_deg"]) == 360) and np.any(np.round(rej["elev_deg"]) <= 0) and np.any(np.isnan(rej["elev_deg"])) and np.any(live["el"] > 0)
    tr = w["epochs"]["fix"][:, 0]["t_rx"]
    assert np.any((tr[1:] < 10) & (tr[:-1] > 604790)) and np.any(w["ticks"][1:] < w["ticks"][:-1])                     # the week; the 48-bit wrap
    modes = set(tuple(int(v) for v in md) for md in w["mode"])
    assert {(0, 0), (1, 0), (1, 1), (0, 1)} <= modes and w["reset"].sum() == 1
    assert t["epochs"]["fix"][1, 0]["ekf_running"] == 1 and t["epochs"]["fix"][2, 0]["ekf_running"] == -1 and t["epochs"]["fix"][2, 0]["flags"] & pos.SPP_VALID
    for s in golden.values():
        assert len(s["ticks"]) <= 40 and all(0 < s["env"][q] < 1e-6 for q in ("x", "y", "z", "alt"))
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_the_constants_are_the_reference_text():
    h = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_pos.h")).read()
    for name, text in (("C_LIGHT", "2.99792458e8"), ("OMEGA_E", "7.2921151467e-5"), ("WGS84_A", "6378137.0"), ("WGS84_B", "6356752.31424518"),
                       ("LLH_DH", "1e-3"), ("EKF_Q", "5e-5"), ("EKF_H0", "1.8e-21"), ("EKF_H1", "6.5e-22"), ("EKF_H2", "1.4e-24")):
        assert re.search(r"\b%s = %s\b" % (name, re.escape(text)), h), name
    for gate in ("> 1e-20", "< 1e-30", "< 1e3", "> 1e3", "< 0.001", "> -100", "< 9000", "75e-3", "< 1e-9", "1ULL << 48"):
        assert gate in h, gate
    assert pos.UERE == 6.0 and pos.F_OSC == 124.999900 * 1000000 and pos.C_LIGHT == 2.99792458e8


# ---- kg_pos.h on the host
def build_driver(tmpdir, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/pos_host_driver.cpp"
    exe = os.path.join(str(tmpdir), name)
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tools", "pos_host_driver.cpp")],
                   check=True)
    return exe


def driver_script(s):
    out = [pos.script_head(pos.kinds_table())]
    for reset, mode, a, b in segments(s):
        if reset:
            out.append("X\n")
        out.append("M %d %d\n" % mode)
        for e in range(a, b):
            out.append(pos.script_epoch(s["snaps"][e], s["sv"][e], s["ticks"][e], s["skip"][e]))
    return "".join(out)


def run_driver(exe, text):
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    return pos.parse_records(p.stdout.decode())


def check_driver(exe, golden):
    for name, s in golden.items():
        ep, st = run_driver(exe, driver_script(s))
        assert len(ep) == len(s["epochs"])
        assert same_bits(ep, s["epochs"]) is None, (name, "outputs", same_bits(ep, s["epochs"]))
        assert same_bits(st, s["states"]) is None, (name, "states", same_bits(st, s["states"]))


def test_host_build_equals_the_reference(tmp_path, golden):
    check_driver(build_driver(tmp_path, "pos_host", []), golden)


def test_host_build_under_sanitizers(tmp_path, golden):
    check_driver(build_driver(tmp_path, "pos_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), golden)


def test_scene_builder_round_trips_a_known_position(tmp_path):
    """a noiseless scene solves to the position and clock it was built from.  The bar: ct near 1e14 m has an ulp of 1/64 m, so every
    pseudorange carries up to one ulp of rounding; with a GDOP below 6 for these six directions that is under 0.1 m (1e-6 deg)."""
    exe = build_driver(tmp_path, "pos_host_rt", [])
    llh, t_rx = (-71.06, 42.36, 35.0), 345678.9
    azel = [(20, 70), (100, 25), (190, 40), (250, 15), (310, 55), (355, 30)]
    rows = pos.scene_rows(llh, t_rx, azel)
    sv, sn = np.zeros(6, eph.sv_dtype), np.zeros(6, eph.snap_dtype)
    sv["x"], sv["y"], sv["z"], sv["ct"], sv["week"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], 2200
    sn["sat"], sn["power"] = np.arange(6), 1e6
    ep, st = run_driver(exe, pos.script_head(pos.kinds_table()) + pos.script_epoch(sn, sv, 1000, 0))
    f = ep[0]["fix"][0]
    assert f["flags"] == pos.CALLED | pos.POS_VALID | pos.SPP_VALID and f["nsv"] == 6 and ep[0]["grn_yel_red"] == 1
    want = pos.llh_to_xyz(*llh)
    assert np.linalg.norm(np.array([f["x"], f["y"], f["z"]]) - want) < 0.1 and abs(f["t_rx"] - t_rx) * pos.C_LIGHT < 0.1
    assert abs(np.degrees(f["lambda"]) - llh[0]) < 1e-6 and abs(np.degrees(f["phi"]) - llh[1]) < 1e-6 and abs(f["alt"] - llh[2]) < 0.1
    got = [(int(r["el"]), int(r["az"])) for r in ep[0]["sat"][:6]]
    assert got == [(el, az) for az, el in azel], got
    assert ep[0]["ch_has_soln"] == 0x3F and st[0, 0]["state_spp"].tolist() == [1, 0]


def test_library_exports_the_pos_symbols():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, nargs in POS_SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m and len(m.group(1).split(",")) == nargs, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert getattr(lib, s) is not None
    assert set(s for s in _lib.SYMBOLS if s.startswith("kg_pos_")) == set(POS_SYMBOLS)
    assert not re.search(r"\bvoid\s*\*\s*d_\w+", "".join(re.findall(r"kg_pos_\w+\s*\([^;]*\)\s*;", header))), "every device pointer of kg_pos is typed"
