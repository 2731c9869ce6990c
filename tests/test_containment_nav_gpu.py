"""Containment of kg_nav_push_bits_dev and kg_nav_push_epochs_dev on the guarded layouts of tests/guarded.py (the four properties of
tests/test_containment_gpu.py): exactly d_counts[ch] records per row and nchan counts are written; exactly nbits[ch] bytes of row ch --
of each byte only bit 0 -- or the counted records are read; the result is the host call's (for the epoch rows: the model's)."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import nav, trk
from tests.guarded import contain
from . import nav_model as nm
from .test_nav_cpu import load_golden

pytestmark = pytest.mark.gpu

MODES = (nav.L1, nav.E1B, nav.L1)
REC = nav.frame_dtype.itemsize


def streams():
    g = load_golden()
    return [g["ca_back_to_back_preambles"]["bits"], g["e1b_odd_start"]["bits"], g["ca_bit_error_w5"]["bits"]]


def test_nav_push_bits(gpu_ctx):
    bits = streams()
    calls = ((700, 1100, 0), (500, 700, 611), (0, 0, 592))                     # nbits per channel and call; zeros among them
    rng = np.random.default_rng(4)
    results = []
    for upper in (0x00, 0xFE):                                                  # what the bytes hold above bit 0
        noisy = [b | (rng.integers(0, 256, b.size).astype(np.uint8) & upper) for b in bits]

        def case(lay):
            ns = nav.NavSync(gpu_ctx, 3, MODES)
            try:
                out, at = [], [0, 0, 0]
                for nb in calls:
                    rows = [noisy[ch][at[ch]:at[ch] + n] for ch, n in enumerate(nb)]
                    at = [a + n for a, n in zip(at, nb)]
                    g_bits, stride = lay.inp(rows, 1)
                    cap = nav.cap_for(MODES, nb) + 1
                    g_fr, fstride = lay.out(3, cap, REC, 8)
                    g_cnt, _ = lay.out(1, 3, 4, 4)
                    ns.push_dev(g_bits.ptr, stride, nb, g_fr.ptr, fstride, cap, g_cnt.ptr)
                    gpu_ctx.sync()
                    counts = lay.take(g_cnt, 4 * 3)[0].view(np.int32)
                    frames = lay.take(g_fr, [int(c) * REC for c in counts])
                    out.append((counts.copy(), [f.view(nav.frame_dtype).copy() for f in frames]))
                states = [ns.state(ch) for ch in range(3)]
                return out, [(s["holding"], s["bit0"], s["pushed"], s["held"]) for s in states]
            finally:
                ns.close()

        results.append(contain(gpu_ctx, case))
    assert results[0] == results[1], "bits above bit 0 of an input byte were read"
    ns = nav.NavSync(gpu_ctx, 3, MODES)                                         # the same stream through the host call
    try:
        at, total = [0, 0, 0], 0
        for k, nb in enumerate(calls):
            host = ns.push([bits[ch][at[ch]:at[ch] + n] for ch, n in enumerate(nb)])
            at = [a + n for a, n in zip(at, nb)]
            counts = np.frombuffer(results[0][0][k][0][2], np.int32)
            assert counts.tolist() == [len(h) for h in host]
            for ch in range(3):
                assert results[0][0][k][1][ch][2] == host[ch].tobytes(), (k, ch)
            total += int(counts.sum())
        assert total >= 30
    finally:
        ns.close()


def test_nav_push_epochs(gpu_ctx):
    bits = streams()
    flags = [np.repeat(bits[0], 20), bits[1], np.repeat(bits[2], 20)]
    calls = ((14000, 1100, 0), (10000, 700, -1 - 12220), (0, 0, 11840))       # records per channel and call; a stopped channel's count
    epoch_cap = 14001
    cap = nav.cap_for_epochs(MODES, epoch_cap)
    rng = np.random.default_rng(6)
    noise = rng.integers(0, 256, (3, epoch_cap * trk.epoch_dtype.itemsize), dtype=np.uint8)

    def case(lay):
        ns = nav.NavSync(gpu_ctx, 3, MODES)
        try:
            out, at = [], [0, 0, 0]
            for counts_in in calls:
                rows = []
                for ch, c in enumerate(counts_in):
                    n = c if c >= 0 else -1 - c
                    r = noise[ch].view(trk.epoch_dtype)[:n].copy()
                    r["flags"] = (r["flags"] & ~np.uint32(trk.INAV)) | flags[ch][at[ch]:at[ch] + n].astype(np.uint32) * trk.INAV
                    at[ch] += n
                    rows.append(r)
                g_ep, stride = lay.inp(rows, 8, stride=epoch_cap + (0 if lay.tight else 3), elem=trk.epoch_dtype.itemsize)
                g_in, _ = lay.inp([np.array(counts_in, np.int32)], 4)
                g_fr, fstride = lay.out(3, cap, REC, 8)
                g_cnt, _ = lay.out(1, 3, 4, 4)
                ns.push_epochs_dev(g_ep.ptr, stride, g_in.ptr, epoch_cap, g_fr.ptr, fstride, cap, g_cnt.ptr)
                gpu_ctx.sync()
                counts = lay.take(g_cnt, 4 * 3)[0].view(np.int32)
                frames = lay.take(g_fr, [int(c) * REC for c in counts])
                out.append((counts.copy(), [f.view(nav.frame_dtype).copy() for f in frames]))
            states = [ns.state(ch) for ch in range(3)]
            return out, [(s["holding"], s["bit0"], s["pushed"], s["held"], s["nav_ms"], s["nav_prev"], s["nav_glitch"]) for s in states]
        finally:
            ns.close()

    res = contain(gpu_ctx, case)
    models = [nm.Channel(m) for m in MODES]                                     # the same through the model
    at, total = [0, 0, 0], 0
    for k, counts_in in enumerate(calls):
        for ch, c in enumerate(counts_in):
            n = c if c >= 0 else -1 - c
            want = nm.frames(models[ch].push(models[ch].nav_bits(flags[ch][at[ch]:at[ch] + n])))
            at[ch] += n
            assert res[0][k][1][ch][2] == want.tobytes(), (k, ch)
            total += len(want)
    assert total >= 15
    for ch, c in enumerate(models):
        s = c.state()
        assert res[1][ch][0] == s["holding"] and res[1][ch][1] == s["bit0"] and res[1][ch][2] == s["pushed"]
