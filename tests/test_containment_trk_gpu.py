"""Containment of kg_trk_process_bits_dev on the guarded layouts of tests/guarded.py (the four properties of
tests/test_containment_gpu.py): it writes exactly d_counts[ch] records per row and nchan counts, reads exactly
ceil((bit offset + nclocks) / 8) bytes of the stream -- and of the last byte only the bits below the end -- and gives the host call's
result."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import trk
from tests.guarded import contain
from . import trk_common as tc

pytestmark = pytest.mark.gpu

NCHAN = 3
CALLS = (8191 + 3, 2 * tc.CA_EPOCH + 5)         # the second call starts 2 bits into a byte and ends 7 bits into one
REC = trk.epoch_dtype.itemsize


def new_tracker(ctx):
    t = trk.Tracker(ctx, NCHAN)
    for ch, (w, cg) in enumerate(((tc.CA1, tc.NOM), (tc.QZ, tc.NOM + 3000), (tc.E1, tc.RATE_MAX))):
        t.set_sat(ch, w)
        if w & trk.E1B_MODE:
            t.set_e1b_code(ch, tc.e1b_code(3))
        t.set_rate_cg(ch, cg)
        t.set_rate_lo(ch, tc.LO_NOM + 1000 * ch)
        t.set_gain_lo(ch, 20, 7)
        t.set_gain_cg(ch, 11, 12)
    t.sampler_reset()
    return t


def test_trk_process_bits(gpu_ctx):
    rng = np.random.default_rng(91)
    total = sum(CALLS)
    stream = rng.integers(0, 256, (total + 7) // 8).astype(np.uint8)
    spare = (1 << (total % 8)) - 1                                  # the bits of the last byte that belong to the stream
    results = []
    for beyond in (0x00, 0xFF):                                     # what the last byte holds above the stream's end
        s = stream.copy()
        s[-1] = (s[-1] & spare) | (beyond & ~spare & 0xFF)

        def case(lay):
            t = new_tracker(gpu_ctx)
            try:
                out, clock = [], 0
                for n in CALLS:
                    first, nbytes = clock // 8, (clock % 8 + n + 7) // 8
                    g_bits, _ = lay.inp([s[first:first + nbytes]], 1)
                    cap = trk.cap_for(n) + 1
                    g_ep, stride = lay.out(NCHAN, cap, REC, 8)
                    g_cnt, _ = lay.out(1, NCHAN, 4, 4)
                    t.process_dev(g_bits.ptr, n, g_ep.ptr, stride, cap, g_cnt.ptr)
                    gpu_ctx.sync()
                    counts = lay.take(g_cnt, 4 * NCHAN)[0].view(np.int32)
                    rows = lay.take(g_ep, [int(c) * REC for c in counts])
                    out.append((counts.copy(), [r.view(trk.epoch_dtype).copy() for r in rows]))
                    clock += n
                return out, [t.get_chan(ch).tobytes() for ch in range(NCHAN)], t.get_clocks()[1]
            finally:
                t.close()

        results.append(contain(gpu_ctx, case))
    assert results[0] == results[1], "bits above the stream's end in its last byte were read"
    # the same stream through the host call
    t = new_tracker(gpu_ctx)
    try:
        clock, host = 0, []
        for n in CALLS:
            host.append(t.process(stream[clock // 8:], n))
            clock += n
        first_run = results[0][0]
        for k in range(len(CALLS)):
            counts = np.frombuffer(first_run[k][0][2], np.int32)
            assert counts.tolist() == [len(e) for e in host[k]] and counts.sum() >= 2
            for ch in range(NCHAN):
                assert first_run[k][1][ch][2] == host[k][ch].tobytes(), (k, ch)
    finally:
        t.close()
