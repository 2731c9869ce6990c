"""Generates tests/golden/pos_ref.npz from the REFERENCE ITSELF: gps/PosSolver.cpp with its solver headers and pkgs/TNT_JAMA, compiled from
the reference tree as they are, driven by GNSSDataForEpoch and the SolveTask / update_gps_info_after statements cut from gps/solve.cpp.

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench reads
the reference.  In the manner of tools/make_ref_eph_golden.py it cuts line ranges of the reference into a temporary directory (deleted on
exit), checks the text at both ends of every cut, the text of every statement the harness or csrc/kg_pos.h restates and the decimal text
of every constant, compiles tools/ref/ref_pos_main.cpp around them (once plainly, once with the reference's own DEBUG_POS_SOLVER prints,
which the margin checks read), runs it on seeded scenes (flydog_sdr_gps_amd/pos.py's builder) and keeps only data: the rows, the modes
and the records the reference's code printed.

The bars for the device's continuous outputs come from the reference alone: every scenario is rerun 16 times with every
finite x, y, z input moved by an independent random -4 .. +4 ulp (ct stays: its ulp is 0.03 m); per output quantity the largest deviation
from the unperturbed run over all epochs is the envelope (`env`); the tests' bar is 8 x that, with a floor of 2 ulp.  All reruns must
give the same discrete outputs, and no rounded or gated value may lie within the margins checked at the end; another seed is taken
otherwise.  The conditions at the end keep every later test from passing on an empty set.

    python tools/make_ref_pos_golden.py
"""
import os
import re
import subprocess
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, ROOT  # ref_cut puts the repository root on sys.path
from flydog_sdr_gps_amd import eph, pos  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SOLVE, GPSH, PSC, SPP, EKF, BASE, ELL, CLK, TYPES = ("gps/solve.cpp", "gps/gps.h", "gps/PosSolver.cpp", "gps/SinglePointPositionSolver.h",
                                                     "gps/EKFPositionSolver.h", "gps/PositionSolverBase.h", "gps/Ellipsoid.h", "init/clk.h", "types.h")
LU, UTILS, A2U = "pkgs/TNT_JAMA/jama/lu.h", "pkgs/TNT_JAMA/tnt/utils.h", "pkgs/TNT_JAMA/tnt/array2d_utils.h"

# (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    (GPSH, "POS_CUT_UMS", 289, 296, "struct UMS {", "};"),
    (SOLVE, "POS_CUT_EPOCH", 251, 389, "class GNSSDataForEpoch {", "} ;"),
    (SOLVE, "POS_CUT_GYR", 497, 498, "const int grn_yel_red = (pos_solvers[0]->ekf_valid() ? 0 : (pos_solvers[0]->spp_valid() ? 1 : 2));",
     "GPSstat(STAT_SOLN, 0, grn_yel_red, gnssDataForEpoch.ch_has_soln());"),
    (SOLVE, "POS_CUT_AZEL", 501, 516, "const auto elev_azim = pos_solvers[0]->elev_azim(gnssDataForEpoch.sv());", "continue;"),
    (SOLVE, "POS_CUT_SOLVERS", 571, 578, "std::array<PosSolver::sptr, 3> posSolvers = {", "auto const predOnlyGalileo = [](int type) { return (type == E1B); };"),
    (SOLVE, "POS_CUT_SOLVE", 616, 639, "if (good == 0) continue;", "}"),
]
# what the harness and csrc/kg_pos.h restate: (file, line, text)
PINS = [
    (SOLVE, 38, "#define UERE 6.0"), (CLK, 30, "#define ADC_CLOCK_TYP	    (124.999900*MHz)"), (TYPES, 97, "#define	MHz		1000000"),
    (GPSH, 98, "typedef enum { Navstar, SBAS, QZSS, E1B } sat_e;"), (GPSH, 92, "const double C = 2.99792458e8;"),
    (SOLVE, 327, "_weight[_chans] = replicas[i].power;"), (SOLVE, 330, "if (_weight[_chans] < 1e5 || _weight[_chans] > 5e6)"),
    (SOLVE, 358, "_prn[_chans]  = Sats[_sat[i]].prn;"), (SOLVE, 359, "_type[_chans] = Sats[_sat[i]].type;"),
    (SOLVE, 508, "if (gps.el[gps.last_samp][sat])"), (SOLVE, 511, "const int el = std::round(elev_azim[i].elev_deg);"),
    (SOLVE, 515, "if (az < 0 || az >= 360 || el <= 0 || el > 90)"),
    (SOLVE, 562, "virtual void yield() const {"), (SOLVE, 621, "p->set_use_kalman(use_kalman);"), (SOLVE, 629, "if (plot_E1B) {"),
    (PSC, 75, "weight /= (TNT::mean(weight) * _uere*_uere);"), (PSC, 87, "_state_spp[0] = (status && altitude > -100 && altitude < 9000);"),
    (PSC, 104, "_osc_corr = _spp.mod_gpsweek_rel(_ct_rx[0] - _ct_rx[1]) / _spp.c() / dt_adc_sec;"), (PSC, 109, "if (_use_kalman && _ekf_running == -1) {"),
    (PSC, 128, "_ekf_running  += (_ekf_running < 4);"), (PSC, 153, ", _spp(20, yield)"), (PSC, 157, ", _osc_corr(-1)"),
    (PSC, 171, "return (adc_ticks[0] + (adc_ticks[0] < adc_ticks[1])*(1ULL<<48) - adc_ticks[1])/_fOsc;"),
    (SPP, 29, "double const ct0 = TNT::mean(sv.subarray(3,3, 0,sv.dim2()-1)) + c()*75e-3;"), (SPP, 45, "vec_type dxyzt = cov() * TNT::transpose(h) * weight * drho;"),
    (SPP, 48, "if (TNT::norm(dxyzt.subarray(0,2)) < 0.001)"), (SPP, 57, "mat_type const tmp     = TNT::transpose(h) * weight * h;"),
    (SPP, 59, "if (det > 1e-20 && cov_tmp.dim1() == 4 && cov_tmp.dim2() == 4) {"),
    (EKF, 15, ", _q{{5e-5, 5e-5, 5e-5}}"), (EKF, 16, ", _h{{1.8e-21, 6.5e-22, 1.4e-24}}"), (EKF, 55, "if (std::abs(z-zp) < 1e3) {"),
    (EKF, 60, "w(nsv)   = weight(nsv);"), (EKF, 77, "mat_type const  Pp = Phi * P() * TNT::transpose(Phi) + Q;"),
    (EKF, 78, "mat_type const tmp = h * Pp * TNT::transpose(h) + R;"), (EKF, 82, "if (det < 1e-30)"), (EKF, 84, "mat_type   const G = Pp*TNT::transpose(h) * cov;"),
    (EKF, 92, "if (TNT::norm(dx.subarray(0,2)) > 1e3)"), (EKF, 98, "P().inject((TNT::eye<double>(5) - G * h) * Pp);"), (EKF, 109, "dt = std::max(0.1, dt);"),
    (EKF, 116, "q(3,3)          = c2()*(0.5*_h[0]*dt + 2*_h[1]*dt2 + 2.0/3.0*M_PI*M_PI*_h[2]*dt3);"),
    (EKF, 117, "q(3,4) = q(4,3) = c2()*(               2*_h[1]*dt  +         M_PI*M_PI*_h[2]*dt2);"),
    (EKF, 118, "q(4,4)          = c2()*(0.5*_h[0]/dt + 2*_h[1]     + 8.0/3.0*M_PI*M_PI*_h[2]*dt);"),
    (BASE, 26, ", _omega_e(7.2921151467e-5)"), (BASE, 27, ", _c(2.99792458e8) {}"), (BASE, 75, "double const cws = c()*7*24*3600;"),
    (BASE, 96, "double const theta = -cdt/c()*omega_e();"), (BASE, 115, "for (int i=0; i<5; ++i) {"), (BASE, 119, "if (std::abs(theta-theta_old) < 1e-9)"),
    (BASE, 67, "f(i_sv, elev_rad, azim_rad + (azim_rad < 0)*2*M_PI);"),
    (ELL, 20, "Ellipsoid(double a=6378137.0,"), (ELL, 21, "double b=6356752.31424518,"), (ELL, 22, "int max_iter=10,"), (ELL, 23, "double dh=1e-3)"),
    (ELL, 42, "double const lambda   = 2.0*std::atan2(x(1), x(0)+rho);"), (ELL, 83, "return std::atan(z_by_rho / (1.0 - e2()*nu_ratio));"),
    (ELL, 102, "double e2() const { return 1.0 - b2()/a2(); }"),
    (LU, 100, "int kmax = std::min(i, j);"), (LU, 113, "if (std::abs(LUcolj[i]) > std::abs(LUcolj[p])) {"), (A2U, 246, "sum += A[i][k] * B[k][j];"),
    (UTILS, 109, "return n ? sum/T(n) : T(0);"),
]
# decimal text in csrc/kg_pos.h that must be the reference's: (name in kg_pos.h, text)
HEADER_CONSTS = [("C_LIGHT", "2.99792458e8"), ("OMEGA_E", "7.2921151467e-5"), ("WGS84_A", "6378137.0"), ("WGS84_B", "6356752.31424518"), ("LLH_DH", "1e-3"),
                 ("EKF_Q", "5e-5"), ("EKF_H0", "1.8e-21"), ("EKF_H1", "6.5e-22"), ("EKF_H2", "1.4e-24")]

REF_TYPE = {eph.NAVSTAR: 0, eph.CA: 2, eph.E1B: 3}                     # sat_e: Navstar, SBAS, QZSS, E1B
KIND_OF = {v: k for k, v in REF_TYPE.items()}
CWS = pos.C_LIGHT * 7 * 24 * 3600
QUANT = ("x", "y", "z", "t_rx", "osc_corr", "lambda", "phi", "alt", "elev_deg", "azim_deg")


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    assert pos.UERE == float("6.0") and pos.F_OSC == float("124.999900") * 1000000
    hdr = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_pos.h")).read()
    for name, t in HEADER_CONSTS:
        assert re.search(r"\b%s = %s\b" % (name, re.escape(t)), hdr), ("csrc/kg_pos.h does not carry the reference's text", name, t)
    exes = []
    for name, extra in (("pos_ref", []), ("pos_ref_dbg", ["-DDEBUG_POS_SOLVER"])):
        exe = os.path.join(tmp, name)
        cmd = (["g++", "-O2", "-w", "-std=gnu++14", "-ffp-contract=off", "-I" + tmp, "-I" + os.path.join(R, "gps"), "-I" + os.path.join(R, "pkgs", "TNT_JAMA")] +
               extra + ref_cut.cut_macros(CUTS) + ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_pos_main.cpp")])
        subprocess.run(cmd, check=True)
        exes.append(exe)
    return exes


# ---- scenes
KINDS = pos.kinds_table()
SATS12 = [0, 3, 7, 12, 33, 36, 40, 45, 50, 20, 25, 30]                  # Sats[] indices: Navstar x4, QZSS 33, E1B 36 40 45 50, Navstar x3
AZEL12 = [(10, 60), (80, 30), (150, 45), (220, 20), (300, 70), (350, 15), (45, 80), (120, 10), (200, 55), (260, 35), (330.2, 0.3), (359.7, 25)]
HOME = (16.3, 48.2, 200.0)


def fixed_ct(ct):
    """ct into [0, cws) with C * (ct / C) == ct, as a t_tx times C is"""
    ct = ct % CWS
    for _ in range(8):
        c2 = pos.C_LIGHT * (ct / pos.C_LIGHT)
        if c2 == ct:
            return ct
        ct = c2
    raise AssertionError("no fixed point for ct")


class Scene:
    """accumulates epochs: the script for the harness and the arrays for the golden"""

    def __init__(self, rng):
        self.rng, self.ep, self.mode, self.reset_before = rng, [], (1, 0), False
        self.t, self.ticks = 100000.0, (1 << 47) + 12345

    def set_mode(self, use_kalman, plot):
        self.mode = (int(use_kalman), int(plot))

    def reset(self):
        self.reset_before = True

    def epoch(self, llh=HOME, azel=AZEL12, sat_ids=SATS12, dt=1.0, noise=2.0, err=None, power=None, flags=None, skip=0, nan_rows=(), same_sat=None):
        self.t += dt
        self.ticks = (self.ticks + int(round(dt * pos.F_OSC * (1 + 2e-7)))) % (1 << 48)
        n = len(azel)
        e = self.rng.normal(0, noise, n) + (0 if err is None else np.asarray(err, float))
        rows = pos.scene_rows(llh, self.t % 604800.0 + 0.0123, azel, range_error=e)
        if same_sat is not None:
            rows[:, :3] = rows[same_sat, :3]
        sv, sn = np.zeros(n, eph.sv_dtype), np.zeros(n, eph.snap_dtype)
        for i in range(n):
            sv[i]["x"], sv[i]["y"], sv[i]["z"] = rows[i, :3]
            sv[i]["ct"] = fixed_ct(rows[i, 3])
            sv[i]["week"], sv[i]["t_k"] = 2190 + (self.t >= 604800.0), 100.0
            sn[i]["sat"] = sat_ids[i]
            sn[i]["power"] = (1e6 + 2.5e5 * ((i * 7) % 5)) if power is None else power[i]
            sv[i]["flags"] = 0 if flags is None else flags[i]
            if sn[i]["power"] < 1e5 or sn[i]["power"] > 5e6:
                sv[i]["flags"] |= eph.SV_POWER
            if i in nan_rows:
                sv[i]["flags"] |= eph.SV_BAD
                sv[i]["x"] = sv[i]["y"] = sv[i]["z"] = sv[i]["ct"] = sv[i]["t_k"] = np.nan
        if n < 12:                                                     # one nrow per scenario: the rest are channels that are not ready
            sv, sn = np.concatenate([sv, np.zeros(12 - n, eph.sv_dtype)]), np.concatenate([sn, np.zeros(12 - n, eph.snap_dtype)])
            sv["flags"][n:] = eph.SV_NOT_VALID
        self.ep.append(dict(sv=sv, sn=sn, ticks=self.ticks, skip=skip, mode=self.mode, reset=self.reset_before))
        self.reset_before = False

    def script(self, ref, perturb=None):
        out = [pos.script_head([REF_TYPE[k] for k in KINDS] if ref else KINDS)]
        mode = (1, 0)
        for e in self.ep:
            if e["reset"]:
                out.append("X\n")
            if e["mode"] != mode:
                mode = e["mode"]
                out.append("M %d %d\n" % mode)
            sv = e["sv"]
            if perturb is not None:
                sv = sv.copy()
                for f in "xyz":
                    v = sv[f]
                    ok = np.isfinite(v)
                    k = perturb.integers(-4, 5, v.size)
                    v[ok] = v[ok] + k[ok] * np.spacing(np.abs(v[ok]))
            out.append(pos.script_epoch(e["sn"], sv, e["ticks"], e["skip"]))
        return "".join(out)


def scenario_main(rng):
    """Kalman on, the three solvers; the cases in order"""
    s = Scene(rng)
    s.set_mode(1, 1)
    for _ in range(5):
        s.epoch()                                                      # 12 satellites; the EKF starts and counts to 4
    pw = [1e6] * 12
    pw[2] = 10.0
    s.epoch(power=pw)                                                  # a power-gated row ahead of the E1B rows: the index quirk
    s.epoch(nan_rows=(5,))                                             # a BAD row while the EKF runs
    err = [0] * 12
    err[1] = 5000.0
    s.epoch(err=err)                                                   # an outlier above 1e3 m: the weights shift
    s.epoch(skip=0xFFF & ~((1 << 0) | (1 << 1) | (1 << 4) | (1 << 6)))  # exactly 4
    s.epoch(skip=0xFFF & ~((1 << 0) | (1 << 4) | (1 << 8)))            # 3: SPP false, the EKF coasts
    s.epoch(skip=0xFFF & ~((1 << 5) | (1 << 6) | (1 << 0)))            # only-Galileo set of 2
    s.epoch(flags=[eph.SV_NOT_VALID] * 12)                             # no satellite after a valid epoch: nothing in Replicas
    s.epoch(power=[10.0] * 12)                                         # Replicas, but nothing enters
    s.epoch()
    far = (17.2, 48.9, 300.0)                                          # ~100 km north-east, no satellite square to it: the gate empties
    s.epoch(llh=far)
    for _ in range(4):
        s.epoch(llh=far)                                               # two good SPP fixes restart the EKF
    s.epoch(llh=(17.2, 48.9, 12000.0))                                 # the altitude gate, above
    s.epoch(llh=(17.2, 48.9, -500.0))                                  # and below
    s.epoch(llh=far, azel=AZEL12[:6], sat_ids=SATS12[:6], same_sat=0)  # a degenerate geometry: ComputeCov refuses
    for _ in range(3):
        s.epoch(llh=far)
    return s


def scenario_week(rng):
    """ct_rx crosses the week and the 48-bit tick count wraps; Kalman off, then on; plot_E1B off, then on"""
    s = Scene(rng)
    s.t, s.ticks = 604800.0 - 6.5, (1 << 48) - int(4.5 * pos.F_OSC)
    s.set_mode(0, 0)
    for _ in range(3):
        s.epoch()
    s.epoch(nan_rows=(3,))                                             # a BAD row while no EKF runs
    s.set_mode(1, 0)
    for _ in range(6):
        s.epoch()
    s.set_mode(1, 1)
    for _ in range(4):
        s.epoch()
    s.set_mode(0, 1)
    s.epoch()
    s.set_mode(1, 1)
    for _ in range(3):
        s.epoch()
    s.reset()
    for _ in range(3):
        s.epoch()
    return s


def scenario_step(rng):
    """high satellites, a 2.1 km jump sideways two epochs into the EKF: residuals below the outlier gate, the step above its gate (reached: the generator asserts it)"""
    azel = [(a, 62 + (i % 4) * 6) for i, a in enumerate(range(0, 360, 45))]
    ids = [0, 3, 7, 12, 20, 25, 30, 33]
    s = Scene(rng)
    for _ in range(2):
        s.epoch(azel=azel, sat_ids=ids, noise=0.5)
    for _ in range(5):
        s.epoch(llh=(16.328, 48.2, 200.0), azel=azel, sat_ids=ids, noise=0.5)
    return s


SCENARIOS = (("main", scenario_main), ("week", scenario_week), ("step", scenario_step))


def run(exe, text):
    p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    return p.stdout.decode()


def discrete(ep):
    """the discrete outputs and NaN-ness, as bytes"""
    parts = [ep["fix"][n].tobytes() for n in ("flags", "ekf_running", "nsv")] + [ep["sat"][n].tobytes() for n in ("sat", "ch", "type", "week", "el", "az")]
    parts += [ep[n].tobytes() for n in ("chans", "grn_yel_red", "ch_has_soln")]
    parts += [np.isnan(ep["fix"][n]).tobytes() for n in QUANT[:8]] + [np.isnan(ep["sat"][n]).tobytes() for n in QUANT[8:]]
    return b"".join(parts)


def quantity(ep, q):
    return ep["sat"][q] if q in ("elev_deg", "azim_deg") else ep["fix"][q]


def llh_alt(x, y, z):
    e2 = 1.0 - (pos.WGS84_B ** 2) / (pos.WGS84_A ** 2)
    rho = np.hypot(x, y)
    phi = np.arctan(z / rho / (1 - e2))
    alt = 0.0
    for _ in range(10):
        nu = pos.WGS84_A / np.sqrt(1 - e2 * np.sin(phi) ** 2)
        alt = rho / np.cos(phi) - nu
        phi = np.arctan(z / rho / (1 - e2 * nu / (nu + alt)))
    return alt


def margins_ok(ep, st, dbg):
    """nothing rounded or gated within the margins: az/el 1e-6 deg of a rounding or gate edge; altitude, |z - zp| and the step norm a relative
    1e-6 of their gates (the last two from the reference's DEBUG_POS_SOLVER prints, three decimals: 5e-7 of the gate).  The determinants are
    not printed by the reference: for them the equal discrete outputs of the 16 perturbed reruns stand."""
    for q in ("elev_deg", "azim_deg"):
        v = ep["sat"][q][np.isfinite(ep["sat"][q])]
        if np.any(np.abs((v % 1.0) - 0.5) < 1e-6):
            return False
    for k in range(3):
        x, y, z = (st["spp_state"][:, k, i] for i in range(3))
        with np.errstate(all="ignore"):
            alt = llh_alt(x, y, z)
        alt = alt[np.isfinite(alt)]
        if np.any(np.abs(alt + 100) < 1e-4) or np.any(np.abs(alt - 9000) < 9e-3):
            return False
    for ln in dbg.splitlines():
        f = ln.split()
        if ln.startswith("EKF dx"):
            if abs(float(f[-1]) - 1e3) < 2e-3:
                return False
        elif ln.startswith("EKF") and len(f) == 4 and "nan" not in f[2]:
            if abs(abs(float(f[2])) - 1e3) < 2e-3:
                return False
    return True


def make(exes, name, fn, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    s = fn(rng)
    text = s.script(True)
    ep, st = pos.parse_records(run(exes[0], text), KIND_OF)
    assert len(ep) == len(s.ep)
    dbg = run(exes[1], text)
    plain = "\n".join(ln for ln in dbg.splitlines() if ln[:2] in ("F ", "S ", "G ", "T ")) + "\n"
    ep2, st2 = pos.parse_records(plain, KIND_OF)
    assert ep2.tobytes() == ep.tobytes() and st2.tobytes() == st.tobytes(), "the DEBUG_POS_SOLVER build computes something else"
    if not margins_ok(ep, st, dbg):
        return None
    env = {q: 0.0 for q in QUANT}
    prng = np.random.Generator(np.random.PCG64(seed ^ 0x5EED))
    for _ in range(16):
        pe, _ = pos.parse_records(run(exes[0], s.script(True, perturb=prng)), KIND_OF)
        if discrete(pe) != discrete(ep):
            return None
        for q in QUANT:
            a, b = quantity(ep, q), quantity(pe, q)
            ok = np.isfinite(a)
            if ok.any():
                env[q] = max(env[q], float(np.abs(a[ok] - b[ok]).max()))
    return dict(scene=s, ep=ep, st=st, env=env, dbg=dbg)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exes = build(tmp)
        out, made = {"names": np.array([n for n, _ in SCENARIOS])}, {}
        for k, (name, fn) in enumerate(SCENARIOS):
            for seed in range(0x504F5300 + 64 * k, 0x504F5300 + 64 * k + 32):
                g = make(exes, name, fn, seed)
                if g is not None:
                    break
                print("%s: seed %#x lies on an edge, taking the next" % (name, seed))
            assert g is not None, name
            made[name] = g
            s = g["scene"]
            out[name + "_snaps"] = np.concatenate([e["sn"] for e in s.ep]).view(np.uint8)
            out[name + "_sv"] = np.concatenate([e["sv"] for e in s.ep]).view(np.uint8)
            out[name + "_ticks"] = np.array([e["ticks"] for e in s.ep], np.uint64)
            out[name + "_skip"] = np.array([e["skip"] for e in s.ep], np.uint32)
            out[name + "_mode"] = np.array([e["mode"] for e in s.ep], np.int32)
            out[name + "_reset"] = np.array([e["reset"] for e in s.ep], np.int32)
            out[name + "_epochs"] = g["ep"].view(np.uint8)
            out[name + "_states"] = g["st"].reshape(-1).view(np.uint8)
            out[name + "_env"] = np.array([g["env"][q] for q in QUANT])
            print(name, len(s.ep), "epochs; envelope", {q: "%.3g" % g["env"][q] for q in QUANT})
        promised(made)
        out["quant"] = np.array(QUANT)
        np.savez_compressed(os.path.join(GOLD, "pos_ref.npz"), **out)
        print("wrote pos_ref.npz,", os.path.getsize(os.path.join(GOLD, "pos_ref.npz")), "bytes")


def promised(made):
    """on the reference's records alone: every case the tests rely on is there"""
    m, w, t = made["main"], made["week"], made["step"]
    f0 = m["ep"]["fix"][:, 0]
    spp, ekf, called = (f0["flags"] & pos.SPP_VALID) != 0, (f0["flags"] & pos.EKF_VALID) != 0, (f0["flags"] & pos.CALLED) != 0
    assert np.any((f0["nsv"] == 4) & spp) and np.any((f0["nsv"] == 3) & ~spp & ekf & called) and np.any((f0["nsv"] == 12) & spp & ekf)
    # the index quirk: a power-gated row ahead of an E1B row, and solver 2's set is not the rows whose satellite is Galileo
    quirk = 0
    for e, rec in zip(m["scene"].ep, m["ep"]):
        enter = [i for i in range(len(e["sv"])) if not e["sv"][i]["flags"] & (eph.SV_NOT_VALID | eph.SV_POWER) and not (e["skip"] >> i) & 1]
        true_e1b = sum(KINDS[e["sn"][i]["sat"]] == eph.E1B for i in enter)
        gated = [i for i in range(len(e["sv"])) if e["sv"][i]["flags"] & eph.SV_POWER]
        if gated and any(KINDS[e["sn"][i]["sat"]] == eph.E1B and i > gated[0] for i in enter) and e["mode"][1]:
            assert rec["fix"][2]["nsv"] != true_e1b and rec["fix"][1]["nsv"] + rec["fix"][2]["nsv"] == len(enter)
            quirk += 1
    assert quirk >= 1
    # a BAD row while the EKF runs (it stays valid) and one while it does not
    def bad_epochs(g):
        return [k for k, e in enumerate(g["scene"].ep) if np.any(e["sv"]["flags"] & eph.SV_BAD)]
    k = bad_epochs(m)[0]
    assert ekf[k - 1] and ekf[k] and not spp[k] and np.isnan(m["ep"]["sat"][k]["elev_deg"]).any()
    k = bad_epochs(w)[0]
    assert w["ep"]["fix"][k, 0]["ekf_running"] == -1 and not w["ep"]["fix"][k, 0]["flags"] & pos.SPP_VALID
    # an outlier above 1e3 m with the EKF going on: the reference's own print of z - zp
    blocks = m["dbg"].split("\nG ")
    def resid(b):
        return [abs(float(ln.split()[2])) for ln in b.splitlines() if re.match(r"EKF +\d+ ", ln) and "nan" not in ln.split()[2]]
    assert any(1 <= sum(v > 1e3 for v in resid(b)) <= 3 and sum(v < 1e3 for v in resid(b)) >= 16 for b in blocks)
    # loss and restart
    run_ = f0["ekf_running"]
    lost = [k for k in range(1, len(run_)) if run_[k - 1] >= 1 and run_[k] == -1 and called[k]]
    assert lost and any(run_[k + 1] >= 0 or run_[k + 2] >= 0 for k in lost if k + 2 < len(run_))
    # the altitude gate on both sides, and ComputeCov's refusal
    alts = [llh_alt(*m["st"]["spp_state"][k, 0, :3]) for k in range(len(f0))]
    assert any(a > 9000 and not s_ and n >= 4 for a, s_, n in zip(alts, spp, f0["nsv"])) and any(a < -100 and not s_ and n >= 4 for a, s_, n in zip(alts, spp, f0["nsv"]))
    assert any(n >= 4 and not s_ and c and tuple(m["st"]["spp_state"][k, 0, :3]) == (0.0, 0.0, 0.0) for k, (n, s_, c) in enumerate(zip(f0["nsv"], spp, called)))
    # the EKF's step gate (DEBUG print of the step norm), if a scene reaches it
    steps = [float(ln.split()[-1]) for g in made.values() for ln in g["dbg"].splitlines() if ln.startswith("EKF dx")]
    print("EKF step norms above 1e3:", sum(v > 1e3 for v in steps), "of", len(steps), "(largest %.1f)" % max(steps))
    assert sum(v > 1e3 for v in steps) >= 1 and t["ep"]["fix"][2, 0]["ekf_running"] == -1 and t["ep"]["fix"][1, 0]["ekf_running"] == 1
    # the week and the tick wrap; the modes
    tr = w["ep"]["fix"][:, 0]["t_rx"]
    assert np.any((tr[1:] < 10) & (tr[:-1] > 604790)) and np.all(w["ep"]["fix"][:, 0]["flags"][4:] & pos.POS_VALID)
    tk = np.array([e["ticks"] for e in w["scene"].ep], np.uint64)
    assert np.any(tk[1:] < tk[:-1])
    modes = [e["mode"] for e in w["scene"].ep]
    assert modes[0] == (0, 0) and (1, 0) in modes and (1, 1) in modes and modes.index((1, 0)) > 0
    wf = w["ep"]["fix"]
    assert all(r[0]["ekf_running"] == -1 for md, r in zip(modes, wf) if not md[0]) and any(r[0]["ekf_running"] == 4 for r in wf)
    assert any(md == (1, 1) and r[2]["flags"] & pos.CALLED for md, r in zip(modes, wf)) and not any(r[1]["flags"] & pos.CALLED for md, r in zip(modes, wf) if not md[1])
    # an only-Galileo set below 4, an epoch with nothing after a valid one
    f2 = m["ep"]["fix"][:, 2]
    assert np.any((f2["nsv"] >= 1) & (f2["nsv"] < 4) & ((f2["flags"] & pos.CALLED) != 0))
    none = [k for k in range(1, len(f0)) if m["ep"]["chans"][k] == 0]
    assert len(none) >= 2 and all(f0["flags"][k] & pos.POS_VALID and not called[k] for k in none)
    # the az/el rule: az >= 360, el <= 0 and a NaN (az < 0 on the reference's host); el > 90 cannot be reached (asin)
    sat = m["ep"]["sat"][ekf | spp]
    live = sat[(sat["elev_deg"] != 0) | (sat["azim_deg"] != 0)]
    rej = live[(live["el"] == 0) & (live["az"] == 0)]
    assert np.any(np.round(rej["azim_deg"]) == 360) and np.any(np.round(rej["elev_deg"]) <= 0) and np.any(np.isnan(rej["elev_deg"]))
    assert np.any(live["el"] > 0)
    assert len(t["ep"]) >= 6


if __name__ == "__main__":
    main()
