"""The position fix over the C ABI (kg_pos): what turns the rows of Ephemerides.sv_dev into a position.

Reference                                                                          here
  GNSSDataForEpoch::LoadFromReplicas' compaction   gps/solve.cpp:319-364            -> (inside the kernel)
  SolveTask's three solvers, per-epoch statements  gps/solve.cpp:571-578, :616-639  -> PositionSolver.solve / solve_dev, set_mode
  PosSolverImpl, SPP and EKF solvers, Ellipsoid    gps/PosSolver.cpp, gps/*.h       -> (inside the kernel); PositionSolver.state
  grn_yel_red, ch_has_soln, the az/el rule         gps/solve.cpp:497-516            -> the epoch record

Not here: clock_correction, tod_correction, the gps.* tables, the glitch counters, compute_dop.

scene_rows() is a SCENE BUILDER (receiver position and satellite directions in, sv rows out) and script() / parse_records() are the text
format of tools/pos_host_driver.cpp: input generators and readers for tests and tools, not part of the measured path.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr  # noqa: F401
from . import eph, sats

MAX_CHANS = 12
CALLED, POS_VALID, SPP_VALID, EKF_VALID = 1, 2, 4, 8
UERE, F_OSC = 6.0, 124.999900 * 1000000                 # solve.cpp:38; init/clk.h:30 with types.h:97's MHz
C_LIGHT, OMEGA_E = 2.99792458e8, 7.2921151467e-5
WGS84_A, WGS84_B = 6378137.0, 6356752.31424518

fix_dtype = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("t_rx", "<f8"), ("osc_corr", "<f8"), ("lambda", "<f8"), ("phi", "<f8"), ("alt", "<f8"),
                      ("flags", "<i4"), ("ekf_running", "<i4"), ("nsv", "<i4"), ("pad", "<i4")])
sat_dtype = np.dtype([("elev_deg", "<f8"), ("azim_deg", "<f8"), ("sat", "<i4"), ("ch", "<i4"), ("type", "<i4"), ("week", "<i4"), ("el", "<i4"), ("az", "<i4")])
epoch_dtype = np.dtype([("fix", fix_dtype, (3,)), ("sat", sat_dtype, (12,)), ("chans", "<i4"), ("grn_yel_red", "<i4"), ("ch_has_soln", "<u4"), ("pad", "<u4")])
state_dtype = np.dtype([("spp_state", "<f8", (4,)), ("spp_cov", "<f8", (16,)), ("ekf_state", "<f8", (5,)), ("ekf_P", "<f8", (25,)),
                        ("pos", "<f8", (3,)), ("t_rx", "<f8"), ("osc_corr", "<f8"), ("lambda", "<f8"), ("phi", "<f8"), ("alt", "<f8"), ("ct_rx", "<f8", (2,)),
                        ("ticks_spp", "<u8", (2,)), ("ticks_ekf", "<u8", (2,)),
                        ("pos_valid", "<i4"), ("ekf_running", "<i4"), ("state_spp", "<i4", (2,)), ("ekf_valid", "<i4"), ("pad", "<i4")])
assert (fix_dtype.itemsize, sat_dtype.itemsize, epoch_dtype.itemsize, state_dtype.itemsize) == (80, 40, 736, 536)

_KIND = {sats.NAVSTAR: eph.NAVSTAR, sats.QZSS: eph.CA, sats.E1B: eph.E1B}


def kinds_table():
    """the 64-entry kinds table of the reference's Sats[] (flydog_sdr_gps_amd/sats.py); unused slots Navstar"""
    k = np.zeros(eph.MAX_SATS, np.int32)
    for i, row in enumerate(sats.SATS):
        k[i] = _KIND[row[3]]
    return k


class PositionSolver:
    """SolveTask's three position solvers on the GPU (kg_pos)"""

    def __init__(self, ctx=None, kinds=None, uere=UERE, f_osc=F_OSC, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        k = np.ascontiguousarray(kinds_table() if kinds is None else kinds, np.int32).reshape(-1)
        if k.size != eph.MAX_SATS:
            raise ValueError("kinds: %d entries, not %d" % (k.size, eph.MAX_SATS))
        h = C.c_void_p()
        check(self.lib.kg_pos_create(self.ctx.h, ptr(k), float(uere), float(f_osc), C.byref(h)), "kg_pos_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.lib.kg_pos_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mode(self, use_kalman=True, plot_e1b=False):
        """admcfg's use_kalman_position_solver and plot_E1B; in stream order"""
        check(self.lib.kg_pos_set_mode(self.h, int(use_kalman), int(plot_e1b)), "kg_pos_set_mode")

    def reset(self):
        """three fresh solvers, the mode stays; in stream order"""
        check(self.lib.kg_pos_reset(self.h), "kg_pos_reset")

    def solve_dev(self, d_snaps, d_sv, nrow, nepoch, d_ticks, d_skip, d_out):
        """enqueue only: device addresses (d_skip may be 0 / None)"""
        check(self.lib.kg_pos_solve_dev(self.h, C.c_void_p(int(d_snaps)), C.c_void_p(int(d_sv)), int(nrow), int(nepoch), C.c_void_p(int(d_ticks)),
                                        C.c_void_p(int(d_skip)) if d_skip else None, C.c_void_p(int(d_out))), "kg_pos_solve_dev")

    def solve(self, snaps, sv, ticks, skip=None):
        """snaps (eph.snap_dtype) and sv (eph.sv_dtype): (nepoch, nrow); ticks, skip: (nepoch,) -> epoch_dtype array; synchronises"""
        s = np.ascontiguousarray(snaps, eph.snap_dtype)
        v = np.ascontiguousarray(sv, eph.sv_dtype)
        assert s.ndim == 2 and s.shape == v.shape
        t = np.ascontiguousarray(ticks, np.uint64).reshape(-1)
        k = None if skip is None else np.ascontiguousarray(skip, np.uint32).reshape(-1)
        assert t.size == s.shape[0] and (k is None or k.size == t.size)
        out = np.zeros(s.shape[0], epoch_dtype)
        check(self.lib.kg_pos_solve(self.h, ptr(s), ptr(v), s.shape[1], s.shape[0], ptr(t), ptr(k), ptr(out)), "kg_pos_solve")
        return out

    def state(self, solver=0):
        """-> the solver's kg_pos_state (a 0-d state_dtype array); synchronises"""
        out = np.zeros((), state_dtype)
        check(self.lib.kg_pos_get_state(self.h, int(solver), ptr(out)), "kg_pos_get_state")
        return out


# ---- the scene builder
def llh_to_xyz(lon_deg, lat_deg, alt):
    lam, phi = np.radians(lon_deg), np.radians(lat_deg)
    e2 = 1.0 - (WGS84_B * WGS84_B) / (WGS84_A * WGS84_A)
    nu = WGS84_A / np.sqrt(1.0 - e2 * np.sin(phi) ** 2)
    return np.array([(nu + alt) * np.cos(phi) * np.cos(lam), (nu + alt) * np.cos(phi) * np.sin(lam), ((1 - e2) * nu + alt) * np.sin(phi)])


def enu_basis(lon_deg, lat_deg):
    """columns east, north, up in ECEF (Ellipsoid::dXYZdENU)"""
    lam, phi = np.radians(lon_deg), np.radians(lat_deg)
    cp, sp, cl, sl = np.cos(phi), np.sin(phi), np.cos(lam), np.sin(lam)
    return np.array([[-sl, -sp * cl, cp * cl], [cl, -sp * sl, cp * sl], [0.0, cp, sp]])


def scene_rows(llh, t_rx, azel, radius=26.56e6, range_error=None):
    """Receiver at llh = (lon deg, lat deg, alt m) whose clock reads t_rx [s of week] at reception; one satellite per (az deg, el deg) at
    `radius` from the Earth's centre.  -> (x, y, z, ct) rows, float64 (n, 4): the satellite in the ECEF frame of its transmit time and
    ct = C (t_rx) - range - range_error, the pseudorange model of PositionSolverBase::Iter (the frame turns by omega_e range / c)."""
    p = llh_to_xyz(*llh)
    m = enu_basis(llh[0], llh[1])
    out = np.zeros((len(azel), 4))
    ct_rx = C_LIGHT * t_rx
    for i, (az, el) in enumerate(azel):
        a, e = np.radians(az), np.radians(el)
        u = m @ np.array([np.sin(a) * np.cos(e), np.cos(a) * np.cos(e), np.sin(e)])
        b = p @ u                                       # |p + d u| = radius
        d = -b + np.sqrt(b * b - (p @ p - radius * radius))
        s = p + d * u                                   # in the frame of reception
        th = d / C_LIGHT * OMEGA_E                      # back to the frame of transmission: RotZ(-theta), theta = -d / c * omega_e
        ct, st = np.cos(th), np.sin(th)
        out[i, :3] = [ct * s[0] - st * s[1], st * s[0] + ct * s[1], s[2]]
        out[i, 3] = ct_rx - d - (0.0 if range_error is None else range_error[i])
    return out


# ---- the text format of tools/pos_host_driver.cpp
def script_head(kinds, uere=UERE, f_osc=F_OSC):
    return "K " + " ".join(str(int(k)) for k in kinds) + "\nC %s %s\n" % (float(uere).hex(), float(f_osc).hex())


def script_epoch(snaps, sv, ticks, skip=0):
    """one epoch: snaps (eph.snap_dtype) and sv (eph.sv_dtype) of nrow rows"""
    lines = ["E %d %d %d" % (len(snaps), int(ticks), int(skip))]
    for s, v in zip(snaps, sv):
        lines.append("R %d %d %d %s %s %s %s %s" % (s["sat"], v["flags"], v["week"], float(s["power"]).hex(), float(v["x"]).hex(), float(v["y"]).hex(),
                                                    float(v["z"]).hex(), float(v["ct"]).hex()))
    return "\n".join(lines) + "\n"


def _f(t):
    return float("nan") if "nan" in t else float.fromhex(t)


def parse_records(text, type_map=None):
    """the driver's (or the reference harness') output -> (epoch_dtype array, state_dtype array (nepoch, 3)); type_map: S's type -> kind"""
    epochs, states = [], []
    ep, st = np.zeros((), epoch_dtype), np.zeros(3, state_dtype)
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "F":
            r = ep["fix"][int(f[1])]
            r["flags"], r["ekf_running"], r["nsv"] = int(f[2]), int(f[3]), int(f[4])
            for name, t in zip(("x", "y", "z", "t_rx", "osc_corr", "lambda", "phi", "alt"), f[5:13]):
                r[name] = _f(t)
        elif f[0] == "S":
            r = ep["sat"][int(f[1])]
            r["sat"], r["ch"], r["week"], r["el"], r["az"] = int(f[2]), int(f[3]), int(f[5]), int(f[6]), int(f[7])
            r["type"] = int(f[4]) if type_map is None else type_map[int(f[4])]
            r["elev_deg"], r["azim_deg"] = _f(f[8]), _f(f[9])
        elif f[0] == "G":
            ep["chans"], ep["grn_yel_red"], ep["ch_has_soln"] = int(f[1]), int(f[2]), int(f[3])
        elif f[0] == "T":
            k = int(f[1])
            r = st[k]
            r["pos_valid"], r["state_spp"], r["ekf_valid"] = int(f[2]), (int(f[3]), int(f[4])), int(f[5])
            r["ticks_spp"], r["ticks_ekf"] = (int(f[6]), int(f[7])), (int(f[8]), int(f[9]))
            d = [_f(t) for t in f[10:]]
            assert len(d) == 52, len(d)
            r["ct_rx"], r["spp_state"], r["spp_cov"], r["ekf_state"], r["ekf_P"] = d[0:2], d[2:6], d[6:22], d[22:27], d[27:52]
            fx = ep["fix"][k]
            r["pos"] = (fx["x"], fx["y"], fx["z"])
            for name in ("t_rx", "osc_corr", "lambda", "phi", "alt", "ekf_running"):
                r[name] = fx[name]
            if k == 2:
                epochs.append(ep.copy())
                states.append(st.copy())
                ep, st = np.zeros((), epoch_dtype), np.zeros(3, state_dtype)
        else:
            raise ValueError("unknown record " + ln[:40])
    return (np.array(epochs, epoch_dtype).reshape(-1), np.array(states, state_dtype).reshape(-1, 3))
