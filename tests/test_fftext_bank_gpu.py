"""The receiver bank's FFT extension (kg_rxbank_fftext_*; extensions/FFT/FFT.cpp) against a standalone chain over a short script of
commands: rx0 integrates from the start, leaves and joins again; rx1 walks `SET run=` / `SET mod=` into and out of SAM and channel-null
SAM (the instance and the boost are those of the mode AT THE COMMAND; spec chosen in SAM listens to the second filter, which is fed in
channel-null SAM only), then integrates, with itime and clear on the way; rx2 is never switched on.  The standalone chain: a
kg_fir_process_taps_dev on the bank's own rx_in records, a second filter on the bank's own agc pairs, and a kg_fftext of its own told
the same commands -- rows, map, bins and final sums equal byte for byte.  Everything else the bank hands out is byte-identical to a
second bank that is stepped the same and never told about the extension, which holds nothing for it."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import fftext, post, snd
from flydog_sdr_gps_amd._lib import check, ptr

from . import fftext_common as fc

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
SAM, USB, QAM = post.MODE_SAM, post.MODE_SSB, post.MODE_QAM
# before step k: (receiver, what, value).  A step yields about 0.8 sound blocks.
SCRIPT = {0: [(0, "itime", 0.1), (0, "run", fc.INTEG), (1, "run", fc.SPEC)],       # rx1: spec chosen in USB: the passband, boost 1e6
          3: [(1, "mode", (SAM, 0))],                                              # ... which a later `SET mod=` does not move
          5: [(1, "run", fc.SPEC)],                                                # chosen again in SAM: the second filter, boost 100; plain SAM feeds none
          8: [(1, "mode", (SAM, post.CHAN_NULL_LSB)),                              # now it is fed
              (0, "mode", (SAM, post.CHAN_NULL_USB))],                             # rx0 too (its integ stays on the passband): rx1 is entry 1 of the second filter's list
          12: [(1, "mode", (USB, 0))],                                             # out of SAM: still listening to the second filter
          14: [(1, "itime", 0.2), (1, "run", fc.INTEG), (0, "clear", None)],
          17: [(0, "leave", None)],
          19: [(0, "join", None), (1, "clear", None)],
          20: [(0, "run", fc.WF), (1, "mode", (QAM, 0))],
          22: [(1, "run", fc.SPEC)]}                                               # QAM: the second filter again (never fed), boost 100
STEPS = 25


def _bank():
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, N)
    bank.configure(mix)
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=USB)
    return bank


def _outputs(bank):
    return [np.array(m).copy() for m in bank.audio_map()], {k: bank.fetch(k, list(range(NR))) for k in ("xin", "firo", "s16", "pay", "agc", "iq_pay")}


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import live_allocs, synth
    ctx = gpu_ctx
    plain, told = _bank(), _bank()
    fs = told.fs
    pb, nf = snd.FastFir(ctx, nchan=NR, max_in=4096), snd.FastFir(ctx, nchan=1, max_in=512)
    sx = fftext.FftExt(ctx, nchan=NR, sample_rate=fs)
    bufs = []
    try:
        lo, hi = told.audio[0][1:3]
        for rx in range(NR):
            assert pb.setup(rx, lo, hi, 0.0, fs)
        assert nf.setup(0, lo, hi, 0.0, fs)
        adc = synth.adc_stream(N, 0x5EED0F17)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        stride, MAXB = int(told.bufs.rx_stride), 8
        d_in, d_out, d_post = ctx.alloc(NR * stride * 8), ctx.alloc(NR * (stride + 512) * 8), ctx.alloc(NR * MAXB * 8192)
        d_nin, d_nout, d_npost, d_rows = ctx.alloc(512 * 8), ctx.alloc(512 * 8), ctx.alloc(MAXB * 8192), ctx.alloc(MAXB * 1024)
        bufs = [d_in, d_out, d_post, d_nin, d_nout, d_npost, d_rows]
        assert told.fftext is None and plain.fftext is None
        told.fftext_set_rate(fs)
        held = live_allocs()
        mode = {rx: (USB, 0) for rx in range(NR)}                       # the test's own view of the modes, from the script alone
        on = {rx: False for rx in range(NR)}
        live = {rx: True for rx in range(NR)}
        seen = {"integ0": 0, "pb1": 0, "null1": 0, "silent1": 0, "integ1": 0, "wf0": 0}
        for step in range(STEPS):
            for rx, what, v in SCRIPT.get(step, []):
                if what == "mode":
                    for b in (told, plain):
                        b.post.set_sam_mparam(rx, v[1])
                        b.post.set_mode(rx, v[0])
                    mode[rx] = v
                elif what == "run":
                    told.fftext_set_run(rx, v)
                    sx.set_run(rx, v, mode[rx][0] in post.SAM_MODES, mode[rx][0] == QAM)
                    on[rx] = v != fc.OFF
                elif what == "itime":
                    told.fftext_set_itime(rx, v)
                    sx.set_itime(rx, v)
                elif what == "clear":
                    told.fftext_clear(rx)
                    sx.clear(rx)
                elif what == "leave":
                    for b in (told, plain):
                        b.leave(rx)
                    sx.restart(rx)
                    on[rx], live[rx] = False, False
                elif what == "join":
                    for b in (told, plain):
                        b.join(rx, None, None)
                        b.set_wf(rx, b.params[rx], b.overlapped[rx])
                        b.set_audio(rx, b.rx_inc[rx], LO, HI, mode=USB)
                    pb.reset(rx)
                    sx.restart(rx)
                    mode[rx], on[rx], live[rx] = (USB, 0), False, True
            if step == 0:                                               # the first command made the object: its sums, the spectra, the rows
                assert live_allocs() - held == 3 and told.fftext is not None
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            maps, out = _outputs(told)
            maps2, out2 = _outputs(plain)
            # 1. nothing else changes
            for a, b in zip(maps, maps2):
                assert np.array_equal(a, b), step
            nrec, nfir = maps[0], maps[1]
            for rx in range(NR):
                n = int(nfir[rx])
                for k, per in (("firo", 1), ("s16", 1), ("agc", 1), ("pay", 0.5), ("iq_pay", 4)):
                    m = int(n * per)
                    assert np.array_equal(np.ascontiguousarray(out[k][rx, :m]).view(np.uint8), np.ascontiguousarray(out2[k][rx, :m]).view(np.uint8)), (step, rx, k)
            # 2. the standalone chain on the bank's own records
            act = np.array([rx for rx in range(NR) if live[rx]], np.int32)
            xin = np.ascontiguousarray(out["xin"]).view(np.complex64).reshape(NR, stride)
            ctx.upload(d_in, np.ascontiguousarray(xin[act]))
            nout = np.zeros(act.size, np.int32)
            each = np.ascontiguousarray(nrec[act], np.int32)
            # (kg_fir_process_taps_dev takes one n for all entries: one call per receiver)
            for i, rx in enumerate(act):
                one = np.zeros(1, np.int32)
                check(pb.lib.kg_fir_process_taps_dev(pb.h, ptr(np.array([rx], np.int32)), 1, ptr(int(d_in + i * stride * 8)), stride, int(each[i]),
                                                     ptr(int(d_out)), stride + 512, ptr(one), None, ptr(int(d_post + int(rx) * MAXB * 8192)), MAXB * 1024),
                      "kg_fir_process_taps_dev")
                nout[i] = one[0]
            ctx.sync()
            assert np.array_equal(nout, nfir[act]), (step, nout, nfir)
            agc = np.ascontiguousarray(out["agc"]).view(np.complex64).reshape(NR, -1)
            want_map, want_rows = [], []
            for rx in act:
                nblk = int(nfir[rx]) // 512
                sam_null = mode[rx][0] == SAM and bool(mode[rx][1] & 3)
                if rx == 1 and sam_null:                                # the second filter is fed whether anyone listens or not
                    for blk in range(nblk):
                        ctx.upload(d_nin, np.ascontiguousarray(agc[1, 512 * blk:512 * (blk + 1)]))
                        one = np.zeros(1, np.int32)
                        check(nf.lib.kg_fir_process_taps_dev(nf.h, ptr(np.zeros(1, np.int32)), 1, ptr(int(d_nin)), 512, 512, ptr(int(d_nout)), 512, ptr(one),
                                                             None, ptr(int(d_npost + blk * 8192)), 1024), "kg_fir_process_taps_dev")
                        ctx.sync()
                        assert one[0] == 512
                if not on[rx] or nblk == 0:
                    continue
                for inst, d_sp in ((fc.PASSBAND, d_post + int(rx) * MAXB * 8192),) + (((fc.CHAN_NULL, d_npost),) if sam_null else ()):
                    m = sx.process_dev([rx], [nblk], [inst], d_sp, MAXB * 1024, d_rows, 1024, MAXB)
                    ctx.sync()
                    r = np.zeros((MAXB, 1024), np.uint8)
                    ctx.download(d_rows, r)
                    for j, (ch, ent, blk, b) in enumerate(m.tolist()):
                        want_map.append((ch, blk, b))
                        want_rows.append(r[j].copy())
                        info = sx.state(rx)[0]
                        key = {(0, fc.INTEG): "integ0", (0, fc.WF): "wf0", (1, fc.INTEG): "integ1"}.get((int(rx), int(info["run"])))
                        seen[key or ("null1" if inst == fc.CHAN_NULL else "pb1")] += 1
                if rx == 1 and int(sx.state(1)[0]["run"]) == fc.SPEC and int(sx.state(1)[0]["instance"]) == fc.CHAN_NULL and not sam_null:
                    seen["silent1"] += nblk
            rx_of, blk_of, bin_of = told.fftext_map()
            rows = told.fftext_rows()
            got_map = [(int(a), int(b), int(c)) for a, b, c in zip(rx_of, blk_of, bin_of)]
            assert got_map == want_map, (step, got_map, want_map)
            for r, w in enumerate(want_rows):
                bad = np.flatnonzero(rows[r] != w)
                assert bad.size == 0, (step, want_map[r], "first differing byte", int(bad[0]), int(rows[r, bad[0]]), int(w[bad[0]]))
            assert 2 not in rx_of
            if step in (16, 18, STEPS - 1):                             # the sums: before the leave, while rx0 is away, at the end
                for rx in range(NR):
                    a, b = told.fftext.state(rx, sums=True), sx.state(rx, sums=True)
                    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), (step, rx)
        # the walk met every case
        assert seen["integ0"] >= 8 and seen["pb1"] >= 3 and seen["null1"] >= 2 and seen["silent1"] >= 3 and seen["integ1"] >= 3 and seen["wf0"] >= 2, seen
        assert int(told.fftext.state(0)[0]["run"]) == fc.WF and float(told.fftext.state(0)[0]["time"]) == 0.0          # the joined receiver started afresh
        # 3. the bank that was never told holds nothing for the extension
        assert plain.fftext is None and plain.fftext_map()[0].size == 0
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        for d in bufs:
            ctx.free(d)
        pb.close()
        nf.close()
        sx.close()
        told.close()
        plain.close()
