"""Containment of kg_eph_push_frames_dev and kg_eph_sv_dev on the guarded layouts of tests/guarded.py (the four properties of
tests/test_containment_gpu.py): exactly d_counts[ch] notes per row are written and nothing else; the counted frames, the counts and the
snapshots are only read; of a refused snapshot's record only `flags` is written; the result is the host call's."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import eph, nav
from tests.guarded import contain
from .test_eph_cpu import REFUSED, load_golden
from .test_eph_gpu import segments

pytestmark = pytest.mark.gpu

NOTE, FRAME, SNAP, SV = eph.note_dtype.itemsize, nav.frame_dtype.itemsize, eph.snap_dtype.itemsize, eph.sv_dtype.itemsize


def bind(e, binds):
    for ch, sat, kind in binds:
        e.set_sat(ch, sat, kind)


def test_eph_push_frames(gpu_ctx):
    g = load_golden()["gal"]
    binds, rows, _ = segments(g["ev"])[0]
    binds = binds[:3]
    calls = ((9, 0, 8), (14, 11, 0), (0, 0, 0))                                 # frames per channel and call; zeros among them; 23, 11 and 8 in all
    cap = 14

    def case(lay):
        e = eph.Ephemerides(gpu_ctx, 3)
        try:
            bind(e, binds)
            out, at = [], [0, 0, 0]
            for counts in calls:
                fr = [g["frames"][rows[ch][at[ch]:at[ch] + n]] for ch, n in enumerate(counts)]
                at = [a + n for a, n in zip(at, counts)]
                g_fr, fstride = lay.inp(fr, 8, elem=FRAME, stride=cap + (0 if lay.tight else 3))
                g_cnt, _ = lay.inp([np.array(counts, np.int32)], 4)
                g_no, nstride = lay.out(3, cap, NOTE, 8)
                e.push_frames_dev(g_fr.ptr, fstride, g_cnt.ptr, cap, g_no.ptr, nstride)
                gpu_ctx.sync()
                out.append([n.view(eph.note_dtype).copy() for n in lay.take(g_no, [c * NOTE for c in counts])])
            return out, [e.get(sat) for _, sat, _ in binds], [tuple(sorted(e.chan(ch).items())) for ch in range(3)], tuple(sorted(e.utc().items()))
        finally:
            e.close()

    res = contain(gpu_ctx, case)
    e = eph.Ephemerides(gpu_ctx, 3)                                             # the same through the host call
    try:
        bind(e, binds)
        at, total = [0, 0, 0], 0
        for k, counts in enumerate(calls):
            host = e.push_frames([g["frames"][rows[ch][at[ch]:at[ch] + n]] for ch, n in enumerate(counts)])
            at = [a + n for a, n in zip(at, counts)]
            for ch in range(3):
                assert res[0][k][ch][2] == host[ch].tobytes(), (k, ch)
                total += len(host[ch])
        assert total == 42
        for k, (_, sat, _) in enumerate(binds):
            assert res[1][k][2] == e.get(sat).tobytes() == g["eph"][rows[k][-1]].tobytes(), sat
    finally:
        e.close()


def test_eph_sv(gpu_ctx):
    s = load_golden()["ca"]
    snaps = s["snaps"][:130]
    refused = (s["svi"][:130, 0] & REFUSED) != 0
    assert refused.sum() >= 20 and (~refused).sum() >= 60
    used = [(44, 48) if r else (0, SV) for r in refused]                        # of a refused snapshot only `flags`

    def case(lay):
        e = eph.Ephemerides(gpu_ctx, 12)
        try:
            for binds, rows, _ in segments(s["ev"]):
                bind(e, binds)
                e.push_frames([s["frames"][rows.get(ch, [])] for ch in range(12)])
            g_in, _ = lay.inp([snaps], 4)
            g_out, _ = lay.out(len(snaps), 1, SV, 8, stride=1)                  # one row per record, rows back to back
            e.sv_dev(g_in.ptr, len(snaps), g_out.ptr)
            gpu_ctx.sync()
            return lay.take(g_out, used), e.get(0)
        finally:
            e.close()

    res = contain(gpu_ctx, case)
    e = eph.Ephemerides(gpu_ctx, 12)
    try:
        for binds, rows, _ in segments(s["ev"]):
            bind(e, binds)
            e.push_frames([s["frames"][rows.get(ch, [])] for ch in range(12)])
        host = e.sv(snaps)
        for k, r in enumerate(refused):
            want = host[k:k + 1].tobytes()
            assert res[0][k][2] == (want[44:48] if r else want), k
    finally:
        e.close()
