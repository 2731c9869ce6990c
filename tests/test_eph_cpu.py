"""Ephemeris decode and satellite position without a GPU: the model (tests/eph_model.py) against the reference's own records
(tests/golden/eph_ref.npz, made by tools/make_ref_eph_golden.py), the encoders of flydog_sdr_gps_amd/eph.py through kg_nav's model and
this one, kg_eph.h's host build (tools/eph_host_driver.cpp, plain and under the address / undefined-behaviour sanitizers, a stand-alone
program) against the reference -- decoded state and GetClock bit for bit, position and clock within the derived bars -- and the
exported symbols.

The bars.  Both sides stop E <- M + e sin E at a step below 1e-10, so each lies within 1e-10 e / (1 - e) of the root
and they lie within twice that of each other: dE <= 2e-10 e / (1 - e), a position change of A dE.  For e <= 0.025 and A <= 3.0e7 m that is
1.6e-4 m; with a few ulp of 3e7 m (3.7e-9 m each) from the libraries the bar for x, y, z is 1e-3 m.  The set with e at the field's
maximum (e = (2^32 - 1) 2^-33 = 0.5, A = 2.66e7 m) has A dE = 5.3e-3 m by the same formula; its bar keeps the same ratio to the
formula: 1e-3 * (A dE) / 1.54e-4 = 3.5e-2 m.  The clock correction moves by under 1e-18 s for such a dE, so t_tx differs by at most
one rounding: |ct - ref| <= 2 ulp(ref), |t_k - ref| <= 2 ulp(t_tx)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import eph, nav
from . import eph_model as em
from . import nav_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eph_ref.npz")
C_LIGHT = float.fromhex("0x1.1de784ap+28")
EPH_SYMBOLS = {"kg_eph_create": 3, "kg_eph_destroy": 1, "kg_eph_set_sat": 4, "kg_eph_clear_sat": 2, "kg_eph_clear_chan": 2, "kg_eph_push_frames_dev": 7,
               "kg_eph_push_frames": 7, "kg_eph_get": 3, "kg_eph_get_chan": 4, "kg_eph_get_utc": 2, "kg_eph_sv_dev": 4, "kg_eph_sv": 4, "kg_eph_replica": 3}
REFUSED = eph.SV_NOT_VALID | eph.SV_POWER


def load_golden():
    g = np.load(GOLDEN)
    out = {}
    for name in g["names"]:
        name = str(name)
        out[name] = dict(ev=g[name + "_ev"].copy(), frames=g[name + "_frames"].copy().view(nav.frame_dtype).reshape(-1),
                         eph=g[name + "_eph"].copy().view(eph.ephem_dtype).reshape(-1), chan=g[name + "_chan"].copy(), utc=g[name + "_utc"].copy(),
                         notes=g[name + "_notes"].copy().view(eph.note_dtype).reshape(-1),
                         snaps=g[name + "_snaps"].copy().view(eph.snap_dtype).reshape(-1), svd=g[name + "_svd"].copy(), svi=g[name + "_svi"].copy())
    return out


def final_states(s):
    """-> {sat: the reference's kg_ephem after the scenario's last frame for it}"""
    sat_of, final = {}, {}
    for op, ch, a, b in s["ev"]:
        if op == 0:
            sat_of[ch] = a
        else:
            final[sat_of[ch]] = s["eph"][a]
    return final


def xyz_bar(e):
    """the bar for x, y, z of a satellite with this kg_ephem (see the module's text)"""
    ecc, A = float(e["e"]), float(e["sqrtA"]) ** 2
    if ecc <= 0.025 and A <= 3.0e7:
        return 1e-3
    return 1e-3 * (2e-10 * ecc / (1 - ecc) * A) / (2e-10 * 0.025 / 0.975 * 3.0e7)


def check_sv(got, s, what):
    """got: sv_dtype records (refused rows: only flags looked at) against the scenario's reference records -> the measured maxima"""
    final = final_states(s)
    stats = dict(n=0, equal=0, xyz_m=0.0, xyz_ulp=0.0, ct_ulp=0.0, tk_ulp=0.0, ct_m=0.0)
    assert len(got) == len(s["snaps"])
    for k, (v, o, d, (flags, week)) in enumerate(zip(s["snaps"], got, s["svd"], s["svi"])):
        assert int(o["flags"]) == int(flags), (what, k, int(o["flags"]), int(flags))
        if flags & REFUSED:
            continue
        assert int(o["week"]) == int(week), (what, k)
        ct, t_k, xyz = d[2], d[3], d[4:7]
        if flags & eph.SV_BAD:
            assert all(np.isnan(o[f]) for f in ("x", "y", "z", "ct", "t_k")) and np.isnan(d[2:7]).all(), (what, k)
            continue
        bar = xyz_bar(final[int(v["sat"])])
        same = True
        for f, want in zip("xyz", xyz):
            err = abs(float(o[f]) - want)
            assert err <= bar, (what, k, f, float(o[f]), want, bar)
            stats["xyz_m"] = max(stats["xyz_m"], err)
            stats["xyz_ulp"] = max(stats["xyz_ulp"], err / np.spacing(abs(want)))
            same &= float(o[f]) == want
        assert abs(float(o["ct"]) - ct) <= 2 * np.spacing(abs(ct)), (what, k, float(o["ct"]), ct)
        assert abs(float(o["t_k"]) - t_k) <= 2 * np.spacing(abs(ct / C_LIGHT)), (what, k, float(o["t_k"]), t_k)
        stats["ct_ulp"] = max(stats["ct_ulp"], abs(float(o["ct"]) - ct) / np.spacing(abs(ct)))
        stats["ct_m"] = max(stats["ct_m"], abs(float(o["ct"]) - ct))
        stats["tk_ulp"] = max(stats["tk_ulp"], abs(float(o["t_k"]) - t_k) / np.spacing(abs(ct / C_LIGHT)))
        same &= float(o["ct"]) == ct and float(o["t_k"]) == t_k
        stats["n"] += 1
        stats["equal"] += bool(same)
    return stats


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def model_runs(golden):
    """the model on every golden scenario: computed once"""
    return {name: em.run(s["ev"], s["frames"]) for name, s in golden.items()}


def test_golden_holds_what_the_generator_promised(golden):
    ca, gal = golden["ca"], golden["gal"]
    sub = ca["frames"]["id"][ca["notes"]["applied"] == 1]
    assert all((sub == k).sum() >= 3 for k in (1, 2, 3, 4))
    word = gal["frames"]["id"][gal["notes"]["applied"] == 1]
    assert all((word == k).sum() >= 3 for k in (0, 1, 2, 3, 4, 5, 6, 10))
    assert (gal["notes"]["applied"] == 0).sum() >= 4 and (ca["notes"]["applied"] == 0).sum() >= 3
    fin = list(final_states(ca).values()) + list(final_states(gal).values())
    assert sum(int(e["valid"]) and e["kind"] != eph.E1B for e in fin) >= 4 and sum(int(e["valid"]) and e["kind"] == eph.E1B for e in fin) >= 3
    assert sum(not int(e["valid"]) for e in fin) >= 2
    flags = np.concatenate([ca["svi"][:, 0], gal["svi"][:, 0]])
    assert ((flags & (REFUSED | eph.SV_BAD)) == 0).sum() >= 200
    assert all(((flags & f) != 0).sum() >= n for f, n in ((eph.SV_TOW_DELAYED, 5), (eph.SV_POWER, 5), (eph.SV_BAD, 3), (eph.SV_TOO_OLD, 5)))
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_model_equals_the_reference(golden, model_runs):
    for name, s in golden.items():
        _, out = model_runs[name]
        for a, (e, chan, utc, note) in enumerate(out):
            assert e == s["eph"][a].tobytes(), (name, a, "kg_ephem")
            assert chan == tuple(int(v) for v in s["chan"][a]) and utc == tuple(int(v) for v in s["utc"][a]), (name, a)
            assert note == s["notes"][a].tobytes(), (name, a, "note")


def test_model_clock_equals_the_reference(golden, model_runs):
    n = 0
    for name, s in golden.items():
        m, _ = model_runs[name]
        for v, d, (flags, _) in zip(s["snaps"], s["svd"], s["svi"]):
            if flags & REFUSED:
                continue
            clock, f = m.get_clock(v)
            assert f == flags & (eph.SV_BAD | eph.SV_TOW_DELAYED)
            assert (np.isnan(clock) and np.isnan(d[0])) or em.bits64(clock) == em.bits64(d[0]), (name, v, clock, d[0])
            n += 1
    assert n >= 200


def test_the_constants_are_the_reference_doubles():
    """exact powers of two or pi for Galileo would pass none of the decode tests; the header must carry the reference's doubles"""
    h = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_eph.h")).read()
    for name, text in (("P2_32", "2.328306436538696E-10"), ("P2_33", "1.164153218269348E-10"), ("P2_35", "2.910383045673370E-11"),
                       ("P2_43", "1.136868377216160E-13"), ("P2_46", "1.421085471520200E-14"), ("SC2RAD", "3.1415926535898"), ("MU", "3.986005e14"),
                       ("OMEGA_E", "7.2921151467e-5"), ("C_LIGHT", "2.99792458e8"), ("F_REL", "-4.442807633e-10"), ("CPS", "1.023e6")):
        m = re.search(r"\b%s = (-?0x[0-9a-f.]+p[+-]\d+)" % name, h)
        assert m and float.fromhex(m.group(1)) == float(text), name
    assert float("2.328306436538696E-10") != 2.0 ** -32 and float("1.136868377216160E-13") != 2.0 ** -43


def test_encoders_round_trip():
    rng = np.random.default_rng(21)
    for sub, table in eph.L1_FIELDS.items():
        fields = {k: int(rng.integers(0, 1 << n)) for k, (_, n) in table.items()}
        words = eph.subframe_words(sub, fields, tow=12345, fill=rng.integers(0, 2, 240))
        assert words[0] >> 16 == 0x8B and eph.words_fields(sub, words) == (12345, fields)
        fr, _ = nm.run(nav.L1, nav.l1_subframe(words))                  # through kg_nav's model: the frame as the device leaves it
        assert len(fr) == 1 and fr[0]["err"] == 0 and fr[0]["id"] == sub
        m = em.Model(1)
        m.set_sat(0, 3, eph.NAVSTAR)
        note = m.push(0, fr[0])
        assert note["applied"] == 1 and note["tow"] == 12345 * 6 and note["sub"] == sub
        e = m.slot[3]
        if sub == 2:
            assert e["e"] == fields["e"] * 2.0 ** -33 and e["sqrtA"] == fields["sqrtA"] * 2.0 ** -19 and e["t_oe"] == 16 * fields["t_oe"]
            assert e["M_0"] == em.signed(fields["M_0"], 32) * 2.0 ** -31 * em.PI
        if sub == 3:
            assert e["IDOT"] == em.signed(fields["IDOT"], 14) * 2.0 ** -43 * em.PI and e["IODE3"] == fields["IODE3"]
    for wt, table in eph.INAV_FIELDS.items():
        fields = {k: int(rng.integers(0, 1 << n)) for k, (_, n) in table.items()}
        if wt == 5:
            fields.update(e1bhs=0, e1bdvs=0)
        w = eph.inav_word(wt, fields, fill=rng.integers(0, 2, 128))
        assert eph.inav_fields(w) == (wt, fields)
        fr, _ = nm.run(nav.E1B, nav.e1b_page(w))
        assert len(fr) == 1 and fr[0]["err"] == 0 and fr[0]["id"] == wt
        m = em.Model(1)
        m.set_sat(0, 40, eph.E1B)
        m.chan[0]["week_gst"] = 1300
        assert m.push(0, fr[0])["applied"] == 1
        e = m.slot[40]
        if wt == 1:
            assert e["e"] == fields["e"] * em.P2_33 and m.chan[0]["toes"] == 60 * fields["toes"]
        if wt == 4:
            assert e["a_f"][1] == em.signed(fields["f1"], 21) * em.P2_46
        if wt == 10:
            assert e["WN_0G"] == fields["WN_0G"] and e["t_0G"] == 3600 * fields["t_0G"]


def test_golden_frames_are_what_kg_nav_leaves(golden):
    """the generator builds its frames directly; kg_nav's model turns the same words into the same payload"""
    fr = golden["gal"]["frames"][3]                     # a word 4
    bits = np.unpackbits(fr["data"][:30])
    w = np.concatenate((bits[2:114], bits[122:138]))
    got, _ = nm.run(nav.E1B, nav.e1b_page(w, reserved=bits[138:202], reserved2=bits[226:234]))
    assert got[0]["data"].tobytes() == fr["data"].tobytes() and got[0]["id"] == fr["id"]
    fr = golden["ca"]["frames"][0]
    data = np.unpackbits(fr["data"])[:300].reshape(10, 30)[:, :24]
    words = [int("".join(str(b) for b in row), 2) for row in data]
    got, _ = nm.run(nav.L1, nav.l1_subframe(words))
    assert got[0]["data"].tobytes() == fr["data"].tobytes() and got[0]["id"] == fr["id"]


# ---- kg_eph.h on the host
def build_driver(tmpdir, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tools/eph_host_driver.cpp"
    exe = os.path.join(str(tmpdir), name)
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tools", "eph_host_driver.cpp")],
                   check=True)
    return exe


def driver_script(s):
    lines = []
    for op, ch, a, b in s["ev"]:
        if op == 0:
            lines.append("B %d %d %d" % (ch, a, b))
        else:
            r = s["frames"][a]
            lines.append("F %d %d %d %d %s" % (ch, r["err"], r["bit"], r["consumed"], r["data"].tobytes().hex()))
    for v in s["snaps"]:
        lines.append("V %d %d %d %d %d %d %s" % (v["sat"], v["bits"], v["bits_tow"], v["ms"], v["chips"], v["cg_phase"], float(v["power"]).hex()))
    return "\n".join(lines) + "\n"


def check_driver(exe, golden):
    stats = {}
    for name, s in golden.items():
        p = subprocess.run([exe], input=driver_script(s).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
        lines = [ln.split(" ") for ln in p.stdout.decode().splitlines()]
        E, V = [f for f in lines if f[0] == "E"], [f for f in lines if f[0] == "V"]
        assert len(E) == len(s["frames"]) and len(V) == len(s["snaps"])
        frame_of = [a for op, ch, a, b in s["ev"] if op == 1]
        for a, f in zip(frame_of, E):
            assert tuple(int(v) for v in f[1:4]) == tuple(int(v) for v in s["chan"][a]), (name, a, "channel state")
            assert tuple(int(v) for v in f[4:7]) == tuple(int(v) for v in s["utc"][a]), (name, a, "utc")
            assert bytes.fromhex(f[7]) == s["notes"][a].tobytes(), (name, a, "note")
            assert bytes.fromhex(f[8]) == s["eph"][a].tobytes(), (name, a, "kg_ephem")
        got = np.zeros(len(V), eph.sv_dtype)
        for k, f in enumerate(V):
            got[k]["flags"], got[k]["week"] = int(f[1]), int(f[8])
            clock = float.fromhex(f[2])
            for fld, t in zip(("ct", "t_k", "x", "y", "z"), f[3:8]):
                got[k][fld] = float.fromhex(t)
            if not got[k]["flags"] & REFUSED:                           # GetClock: every bit
                want = s["svd"][k][0]
                assert (np.isnan(clock) and np.isnan(want)) or em.bits64(clock) == em.bits64(want), (name, k, clock, want)
        stats[name] = check_sv(got, s, "host " + name)
    return stats


def test_host_build_equals_the_reference(tmp_path, golden):
    stats = check_driver(build_driver(tmp_path, "eph_host", []), golden)
    print(stats)
    assert sum(st["n"] for st in stats.values()) >= 200


def test_host_build_under_sanitizers(tmp_path, golden):
    exe = build_driver(tmp_path, "eph_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_driver(exe, golden)


def test_replica_word_split(tmp_path):
    """kg_trk's word is {~cg_phase[31], cg_phase[30:26], chips[9:0], chips[11:10]}; LoadAtomic's masks read it as dn[-1] and dn[0]"""
    exe = build_driver(tmp_path, "eph_host_r", [])
    cases = [(0, 0), (4091, 63), (1023, 1), (1024, 32), (2730, 21)]
    script = "".join("R %d\n" % ((cg << 12) | ((chips & 0x3FF) << 2) | (chips >> 10)) for chips, cg in cases)
    p = subprocess.run([exe], input=script.encode(), stdout=subprocess.PIPE, check=True)
    assert [tuple(int(v) for v in ln.split()[1:]) for ln in p.stdout.decode().splitlines()] == cases


def test_library_exports_the_eph_symbols():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, nargs in EPH_SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m and len(m.group(1).split(",")) == nargs, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert getattr(lib, s) is not None
    assert set(s for s in _lib.SYMBOLS if s.startswith("kg_eph_")) == set(EPH_SYMBOLS)
    assert not re.search(r"\bvoid\s*\*\s*d_\w+", "".join(re.findall(r"kg_eph_\w+\s*\([^;]*\)\s*;", header))), "every device pointer of kg_eph is typed"
