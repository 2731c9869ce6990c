"""Containment of kg_iqd_process_dev on the guarded layouts of tests/guarded.py: the call writes only the row bytes its map names and
the status records of its blocks, leaves its input alone, and reads only the samples it was given (the results do not change with what
surrounds them, nor with what the outputs held before)."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import iqd

from . import iqd_common as ic
from .guarded import contain

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("draw", [iqd.POINTS, iqd.DENSITY])
def test_iqd_process(gpu_ctx, draw):
    """two channels, entries of three, two and one block of 170 samples (a row of d_iq is used in part), rows of 4 * 77 and 2 * 33 bytes
    whose places are 2 bytes apart from a multiple of 16, a second call on the carried state"""
    pool = ic.pool()
    NS = 170
    chans, nblk, inst = [1, 0, 1], [3, 2, 1], [0, 0, 1]
    x = [[np.ascontiguousarray(pool[ic.AT[seg] + 1000 * c:ic.AT[seg] + 1000 * c + NS * n]) for seg, n in zip(("bpsk", "noise", "cw"), nblk)] for c in range(2)]
    cap = (NS * sum(nblk) + 2 * ic.RING) * 4

    def case(lay):
        q = iqd.IqDisplay(gpu_ctx, nchan=2)
        try:
            for ch, cmds in ((0, ["M 0 0", "P 33", "D %d" % draw]), (1, ["M 1 2", "P 77", "G 55", "D %d" % draw])):
                for l in ic.HEAD + cmds:
                    ic.apply_command(q, ch, l)
            res = []
            for call in range(2):
                g_in, s_in = lay.inp(x[call], 8)
                g_rows, _ = lay.out(1, cap, 1, 16)
                g_st, _ = lay.out(1, sum(nblk), 24, 8)
                m, sent = q.process_dev(chans, nblk, inst, NS, g_in.ptr, s_in, g_rows.ptr, cap, g_st.ptr, sum(nblk), NS * sum(nblk))
                gpu_ctx.sync()
                used = int(m["off"][-1] + m["len"][-1])
                assert m.size >= 8 and (np.diff(m["off"]) == m["len"][:-1]).all() and m["off"][0] == 0
                res.append((lay.take(g_rows, [used]), lay.take(g_st, [24 * sum(nblk)]), m.view(np.uint8), sent))
            res.append([ic.state_of(q, ch) for ch in range(2)])
            return res
        finally:
            q.close()

    res = contain(gpu_ctx, case)
    assert len(res) == 3
