"""The position fix on the GPU (kg_pos) against the reference's own records (tests/golden/pos_ref.npz): the discrete outputs -- flags,
ekf_running, nsv, chans, sat, ch, type, week, el, az, grn_yel_red, ch_has_soln, NaN-ness -- equal, the continuous ones under the bars
tests/test_pos_cpu.py derives from the golden (8 x the reference's own envelope under +-4 ulp of input, floor 2 ulp),
one call of many epochs equal in every bit to a call per epoch, reset and mode in stream order, the refusals, and the chain
kg_eph_sv_dev -> kg_pos_solve_dev with no host copy between."""
import os
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import eph, pos
from flydog_sdr_gps_amd._lib import KiwiGpuError
from .test_pos_cpu import NROW, discrete_equal, load_golden, same_bits, segments, within_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def run_device(ctx, s, single):
    """-> (epoch records, the three final states)"""
    p = pos.PositionSolver(ctx)
    try:
        out = []
        for reset, mode, a, b in segments(s):
            if reset:
                p.reset()
            p.set_mode(*mode)
            for lo, hi in ([(e, e + 1) for e in range(a, b)] if single else [(a, b)]):
                out.append(p.solve(s["snaps"][lo:hi], s["sv"][lo:hi], s["ticks"][lo:hi], s["skip"][lo:hi]))
        return np.concatenate(out), np.array([p.state(k) for k in range(3)], pos.state_dtype)
    finally:
        p.close()


@pytest.mark.parametrize("name", ("main", "week", "step"))
def test_golden_scenarios(gpu_ctx, golden, name):
    s = golden[name]
    whole, st_whole = run_device(gpu_ctx, s, False)
    each, st_each = run_device(gpu_ctx, s, True)
    assert whole.tobytes() == each.tobytes(), (name, "one call against a call per epoch", same_bits(whole, each))
    assert st_whole.tobytes() == st_each.tobytes(), (name, "kg_pos_get_state", same_bits(st_whole, st_each))
    discrete_equal(whole, s["epochs"], name)
    stats = within_bars(whole, s, name)
    print(name, {q: "%.3g / %.3g" % v for q, v in stats.items()})
    want = s["states"][-1]
    for n in ("pos_valid", "ekf_running", "state_spp", "ekf_valid", "ticks_spp", "ticks_ekf"):
        assert np.array_equal(st_whole[n], want[n]), (name, n)
    assert np.all(whole["pad"] == 0) and np.all(whole["fix"]["pad"] == 0)


def test_reset_and_mode_in_stream_order(gpu_ctx, golden):
    """three enqueued calls with a mode change and a reset between them and ONE wait at the end, against the same with a wait after each"""
    s = golden["main"]
    cuts = ((0, 4), (4, 9), (9, 14))
    p = pos.PositionSolver(gpu_ctx)
    ref = pos.PositionSolver(gpu_ctx)
    bufs = []
    try:
        def dev(a):
            d = gpu_ctx.alloc(max(a.nbytes, 8))
            bufs.append(d)
            gpu_ctx.upload(d, a)
            return d
        d_out = gpu_ctx.alloc(14 * pos.epoch_dtype.itemsize)
        bufs.append(d_out)
        d_sn, d_sv, d_tk, d_sk = dev(s["snaps"][:14]), dev(s["sv"][:14]), dev(s["ticks"][:14]), dev(s["skip"][:14])
        gpu_ctx.sync()
        for k, (a, b) in enumerate(cuts):
            if k == 1:
                p.set_mode(0, 1)
            if k == 2:
                p.reset()
                p.set_mode(1, 1)
            p.solve_dev(d_sn + a * NROW * eph.snap_dtype.itemsize, d_sv + a * NROW * eph.sv_dtype.itemsize, NROW, b - a, d_tk + 8 * a, d_sk + 4 * a,
                        d_out + a * pos.epoch_dtype.itemsize)
        got = np.zeros(14, pos.epoch_dtype)
        gpu_ctx.download(d_out, got)                                    # the one wait
        want = []
        for k, (a, b) in enumerate(cuts):
            if k == 1:
                ref.set_mode(0, 1)
            if k == 2:
                ref.reset()
                ref.set_mode(1, 1)
            want.append(ref.solve(s["snaps"][a:b], s["sv"][a:b], s["ticks"][a:b], s["skip"][a:b]))
            gpu_ctx.sync()
        want = np.concatenate(want)
        assert got.tobytes() == want.tobytes(), same_bits(got, want)
        assert np.all(got["fix"][4:9, 0]["ekf_running"] == -1) and not np.any(got["fix"][:4, 1]["flags"] & pos.CALLED)   # Kalman off; plot_e1b off at first
        assert not np.any(got["fix"][9:13, 0]["flags"] & pos.POS_VALID)                                  # fresh solvers after the reset: below 4 satellites
        assert got["fix"][13, 0]["flags"] == pos.CALLED | pos.POS_VALID | pos.SPP_VALID and got["fix"][13, 0]["ekf_running"] == -1
        assert [p.state(k).tobytes() for k in range(3)] == [ref.state(k).tobytes() for k in range(3)]
    finally:
        gpu_ctx.sync()
        for d in bufs:
            gpu_ctx.free(d)
        p.close()
        ref.close()


def test_invalid_arguments_are_refused(gpu_ctx, golden):
    s = golden["main"]
    kinds = pos.kinds_table()
    bad = kinds.copy()
    bad[5] = 3
    for make in (lambda: pos.PositionSolver(gpu_ctx, bad), lambda: pos.PositionSolver(gpu_ctx, kinds[:63]), lambda: pos.PositionSolver(gpu_ctx, kinds, uere=0.0),
                 lambda: pos.PositionSolver(gpu_ctx, kinds, f_osc=float("nan")), lambda: pos.PositionSolver(gpu_ctx, kinds, f_osc=float("inf"))):
        with pytest.raises((KiwiGpuError, ValueError)):
            make()
    p = pos.PositionSolver(gpu_ctx)
    bufs = []
    try:
        p.solve(s["snaps"][:3], s["sv"][:3], s["ticks"][:3], s["skip"][:3])
        before = [p.state(k).tobytes() for k in range(3)]
        d = gpu_ctx.alloc(1 << 16)
        bufs.append(d)
        image = np.full(1 << 16, 0x5A, np.uint8)
        gpu_ctx.upload(d, image)
        sn, sv, tk, sk, out = d, d + 4096, d + 8192, d + 12288, d + 16384
        calls = [lambda: p.solve_dev(sn, sv, 0, 1, tk, sk, out), lambda: p.solve_dev(sn, sv, 13, 1, tk, sk, out), lambda: p.solve_dev(sn, sv, 12, 0, tk, sk, out),
                 lambda: p.solve_dev(sn, sv, 12, 65537, tk, sk, out), lambda: p.solve_dev(0, sv, 12, 1, tk, sk, out), lambda: p.solve_dev(sn, 0, 12, 1, tk, sk, out),
                 lambda: p.solve_dev(sn, sv, 12, 1, 0, sk, out), lambda: p.solve_dev(sn, sv, 12, 1, tk, sk, 0), lambda: p.solve_dev(sn + 2, sv, 12, 1, tk, sk, out),
                 lambda: p.solve_dev(sn, sv + 4, 12, 1, tk, sk, out), lambda: p.solve_dev(sn, sv, 12, 1, tk + 4, sk, out),
                 lambda: p.solve_dev(sn, sv, 12, 1, tk, sk + 2, out), lambda: p.solve_dev(sn, sv, 12, 1, tk, sk, out + 4),
                 lambda: p.set_mode(2, 0), lambda: p.set_mode(1, -1), lambda: p.state(3), lambda: p.state(-1)]
        for k, call in enumerate(calls):
            with pytest.raises(KiwiGpuError):
                call()
        gpu_ctx.sync()
        got = np.zeros(1 << 16, np.uint8)
        gpu_ctx.download(d, got)
        assert np.array_equal(got, image) and [p.state(k).tobytes() for k in range(3)] == before       # nothing touched
    finally:
        for d in bufs:
            gpu_ctx.free(d)
        p.close()


def test_chained_from_kg_eph_on_the_device(gpu_ctx):
    """kg_eph_sv_dev's rows straight into kg_pos_solve_dev, against kg_pos_solve on the same rows copied back: strides, flags, layout"""
    from .test_eph_cpu import load_golden as load_eph_golden
    from .test_eph_gpu import run_scenario
    s = load_eph_golden()["ca"]
    nepoch = 4
    snaps = s["snaps"][:NROW * nepoch].copy()
    flags = s["svi"][:NROW * nepoch, 0]
    assert ((flags & (eph.SV_NOT_VALID | eph.SV_POWER)) == 0).reshape(nepoch, NROW).sum(1).min() >= 4 and np.any(flags & eph.SV_POWER)
    e = run_scenario(gpu_ctx, s, False, "ca", 0, eph.Ephemerides(gpu_ctx, 12))
    p, q = pos.PositionSolver(gpu_ctx), pos.PositionSolver(gpu_ctx)
    bufs = []
    try:
        p.set_mode(1, 1)
        q.set_mode(1, 1)
        ticks = (np.arange(nepoch, dtype=np.uint64) + 5) * np.uint64(pos.F_OSC)
        sv0 = np.zeros(NROW * nepoch, eph.sv_dtype)
        d_sn, d_sv, d_tk, d_out = (gpu_ctx.alloc(n) for n in (snaps.nbytes, sv0.nbytes, ticks.nbytes, nepoch * pos.epoch_dtype.itemsize))
        bufs += [d_sn, d_sv, d_tk, d_out]
        gpu_ctx.upload(d_sn, snaps)
        gpu_ctx.upload(d_sv, sv0)
        gpu_ctx.upload(d_tk, ticks)
        e.sv_dev(d_sn, NROW * nepoch, d_sv)
        p.solve_dev(d_sn, d_sv, NROW, nepoch, d_tk, None, d_out)
        got, sv = np.zeros(nepoch, pos.epoch_dtype), np.zeros(NROW * nepoch, eph.sv_dtype)
        gpu_ctx.download(d_out, got)
        gpu_ctx.download(d_sv, sv)
        assert np.array_equal(sv["flags"], flags)
        want = q.solve(snaps.reshape(nepoch, NROW), sv.reshape(nepoch, NROW), ticks)
        assert got.tobytes() == want.tobytes(), same_bits(got, want)
        enter = ((flags & (eph.SV_NOT_VALID | eph.SV_POWER)) == 0).reshape(nepoch, NROW)
        assert np.array_equal(got["chans"], enter.sum(1)) and np.all(got["fix"][:, 0]["flags"] & pos.CALLED)
        for k in range(nepoch):
            rows = np.flatnonzero(enter[k])
            assert np.array_equal(got["sat"][k]["ch"][:len(rows)], rows) and np.array_equal(got["sat"][k]["sat"][:len(rows)], snaps["sat"].reshape(nepoch, NROW)[k][rows])
            assert got["ch_has_soln"][k] == sum(1 << int(r) for r in rows)
    finally:
        gpu_ctx.sync()
        for d in bufs:
            gpu_ctx.free(d)
        p.close()
        q.close()
        e.close()


def test_cpp_caller_fixes_the_position_it_built(gpu_ctx):
    """examples/fix_dropin.cpp: kg_pos_create / set_mode / solve / get_state through include/kiwigpu.h alone; it checks its own fix"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fix_dropin")
    assert os.path.exists(exe), "examples/fix_dropin is not built (run __graft_entry__.build())"
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert lines[0].startswith("fix 7 ekf -1 nsv 6 lat 48.2000000 lon 16.3000000") and lines[3].startswith("fix 15 ekf 3 nsv 6")
    assert lines[4:10] == ["ch 0 sat 1 el 70 az 20", "ch 1 sat 7 el 25 az 100", "ch 2 sat 12 el 40 az 190", "ch 3 sat 20 el 15 az 250", "ch 4 sat 40 el 55 az 310",
                           "ch 5 sat 45 el 30 az 355"]
