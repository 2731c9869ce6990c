"""Containment of kg_pos_solve_dev on the guarded layouts of tests/guarded.py (the four properties of tests/test_containment_gpu.py):
exactly nepoch records are written and nothing else; the nrow * nepoch snapshots and rows, the nepoch tick counts and skip words are only
read; the result does not depend on what lies around them or on what the output held; the result is the host call's."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import eph, pos
from tests.guarded import contain
from .test_pos_cpu import NROW, load_golden

pytestmark = pytest.mark.gpu

SNAP, SV, EPOCH = eph.snap_dtype.itemsize, eph.sv_dtype.itemsize, pos.epoch_dtype.itemsize


@pytest.mark.parametrize("nrow,nepoch", [(1, 1), (4, 1), (12, 1), (1, 3), (4, 3), (12, 3)])
def test_pos_solve(gpu_ctx, nrow, nepoch):
    s = load_golden()["main"]
    first = 5                                                           # the power-gated, the NaN and the outlier epoch
    snaps = np.ascontiguousarray(s["snaps"][first:first + nepoch, NROW - nrow:])
    sv = np.ascontiguousarray(s["sv"][first:first + nepoch, NROW - nrow:])
    ticks = s["ticks"][first:first + nepoch].copy()
    skip = np.array([0, 1, 0x802][:nepoch], np.uint32)
    assert snaps.shape == (nepoch, nrow)

    def case(lay):
        p = pos.PositionSolver(gpu_ctx)
        try:
            p.set_mode(1, 1)
            g_sn, _ = lay.inp([snaps], 4, elem=SNAP)
            g_sv, _ = lay.inp([sv], 8, elem=SV)
            g_tk, _ = lay.inp([ticks], 8)
            g_sk, _ = lay.inp([skip], 4)
            g_out, _ = lay.out(1, nepoch, EPOCH, 8)
            p.solve_dev(g_sn.ptr, g_sv.ptr, nrow, nepoch, g_tk.ptr, g_sk.ptr, g_out.ptr)
            gpu_ctx.sync()
            return lay.take(g_out, [nepoch * EPOCH]), [p.state(k) for k in range(3)]
        finally:
            p.close()

    res = contain(gpu_ctx, case)
    p = pos.PositionSolver(gpu_ctx)                                     # the same through the host call
    try:
        p.set_mode(1, 1)
        host = p.solve(snaps, sv, ticks, skip)
        assert res[0][0][2] == host.tobytes()
        assert [r[2] for r in res[1]] == [p.state(k).tobytes() for k in range(3)]
        assert host["chans"].max() >= min(nrow, 1) and np.all(host["chans"] <= nrow)
    finally:
        p.close()
