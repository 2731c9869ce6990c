"""The receiver bank's audio spectrum rows (`SET spc_=2`): rx0 is USB with its rows on from the start, rx1 is SAM and walks the
reference's emission script (tests/golden/spec_ref.npz, Pin 3: USB -> SAM -> channel-null LSB -> the n == 5 re-send with mparam 0 ->
channel-null USB -> AM -> channel-null LSB, rows on / off / on on the way), rx2 has its rows off throughout.  Rows and map equal a
standalone chain byte for byte and in order: kg_fir_process_spec_dev on the bank's own rx_in records, and a standalone channel-null
kg_fir on the bank's own agc pairs.  Everything else the bank hands out is byte-identical to a second bank that is stepped the same
and never told about the rows."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import post, snd

from . import spec_common as sc

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
SAM, USB, AM = post.MODE_SAM, post.MODE_SSB, post.MODE_AM
# before step k: (receiver, what, value).  A step yields about 0.8 sound blocks, so changes three steps apart are at least two blocks
# apart (the rows-off stretch: two steps, at least one block).
SCRIPT = {0: [(1, "mode", (USB, 0))],
          3: [(1, "mode", (SAM, 0))],
          6: [(1, "mode", (SAM, post.CHAN_NULL_LSB))],
          9: [(1, "spec", 0)],
          11: [(1, "spec", 2)],
          12: [(1, "mode", (SAM, 0))],
          15: [(1, "mode", (SAM, post.CHAN_NULL_USB))],
          18: [(1, "mode", (AM, 0))],
          21: [(1, "mode", (SAM, post.CHAN_NULL_LSB))]}
STEPS = 24


def _bank(told):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, N)
    bank.configure(mix)
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=USB)
    if told:
        bank.set_spec(0, 2)
        bank.set_spec(1, 2)
        bank.set_spec(2, 1)                                             # not SPEC_SND_AF: off
    return bank, mix


def _apply(bank, step, told):
    for rx, what, v in SCRIPT.get(step, []):
        if what == "spec":
            if told:
                bank.set_spec(rx, v)
        else:                                                           # the mode command with n == 5 (rx_sound_cmd.cpp:202-230)
            bank.post.set_sam_mparam(rx, v[1])
            bank.post.set_mode(rx, v[0])


def _step_outputs(bank):
    maps = bank.audio_map()
    live = list(range(NR))
    return [np.array(m).copy() for m in maps], {k: bank.fetch(k, live) for k in ("xin", "firo", "s16", "pay", "agc", "iq_pay")}


def test_bank_rows_equal_a_standalone_chain(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    ctx = gpu_ctx
    told, plain = _bank(True)[0], _bank(False)[0]
    fs = told.fs
    # the standalone chain: a passband filter per receiver and a channel-null filter for rx1
    pb = snd.FastFir(ctx, nchan=NR, max_in=4096)
    nf = snd.FastFir(ctx, nchan=1, max_in=512)
    bufs = []
    try:
        lo, hi = told.audio[0][1:3]                                     # set_audio clamps the cuts to the bank's rate first
        for rx in range(NR):
            assert pb.setup(rx, lo, hi, 0.0, fs)
        assert nf.setup(0, lo, hi, 0.0, fs)
        adc = synth.adc_stream(N, 0x5EED0059)
        d_adc = told.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        d_adc2 = plain.ctx.alloc(adc.nbytes)
        plain.ctx.upload(d_adc2, adc)
        stride = int(told.bufs.rx_stride)
        d_in, d_out, d_rows = ctx.alloc(NR * stride * 8), ctx.alloc(NR * (stride + 512) * 8), ctx.alloc(NR * 8 * 1024)
        d_nin, d_nrows = ctx.alloc(512 * 8), ctx.alloc(1024)
        bufs = [d_in, d_out, d_rows, d_nin, d_nrows]
        mirror_null = False                                             # the test's own walk of rx1's rule, from the script alone
        spec1, mode1, seen = 2, (USB, 0), {"P0": 0, "P1": 0, "N1": 0, "PN": 0, "null_fed_rows_off": 0}
        for step in range(STEPS):
            _apply(told, step, True)
            _apply(plain, step, False)
            for rx, what, v in SCRIPT.get(step, []):
                if what == "spec":
                    spec1 = v
                else:
                    mode1, mirror_null = v, False
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            maps, out = _step_outputs(told)
            maps2, out2 = _step_outputs(plain)
            # 1. nothing else changes: every audio output byte-identical to the bank that was never told
            for a, b in zip(maps, maps2):
                assert np.array_equal(a, b), step
            nrec, nfir = maps[0], maps[1]
            for rx in range(NR):
                n = int(nfir[rx])
                for k, per in (("firo", 1), ("s16", 1), ("agc", 1), ("pay", 0.5), ("iq_pay", 4)):
                    m = int(n * per)
                    assert np.array_equal(np.ascontiguousarray(out[k][rx, :m]).view(np.uint8), np.ascontiguousarray(out2[k][rx, :m]).view(np.uint8)), (step, rx, k)
            # 2. the standalone chain on the bank's own records
            xin = np.ascontiguousarray(out["xin"]).view(np.complex64).reshape(NR, stride)
            ctx.upload(d_in, xin)
            nout = pb.process_spec_dev(np.arange(NR), d_in, stride, nrec, d_out, stride + 512, d_rows, 8 * 1024, [0] * NR)
            ctx.sync()
            assert np.array_equal(nout, nfir), (step, nout, nfir)
            pb_rows = np.zeros((NR, 8, 1024), np.uint8)
            ctx.download(d_rows, pb_rows)
            agc = np.ascontiguousarray(out["agc"]).view(np.complex64).reshape(NR, -1)
            want = []                                                   # (rx, inst, blk, row) in emission order per receiver
            for rx in range(NR):
                for blk in range(int(nfir[rx]) // 512):
                    if rx == 0:
                        want.append((0, sc.PASSBAND, blk, pb_rows[0, blk]))
                        seen["P0"] += 1
                    if rx == 1:
                        sam_null = mode1[0] == SAM and bool(mode1[1] & 3)
                        emitted_p = spec1 == 2 and not mirror_null
                        if emitted_p:
                            want.append((1, sc.PASSBAND, blk, pb_rows[1, blk]))
                            seen["P1"] += 1
                        if mode1[0] in post.SAM_MODES:
                            mirror_null = sam_null
                        if sam_null:                                    # fed whether the rows are on or not
                            ctx.upload(d_nin, np.ascontiguousarray(agc[1, 512 * blk:512 * (blk + 1)]))
                            n1 = nf.process_spec_dev([0], d_nin, 512, [512], None, 0, d_nrows, 1024, [sc.CHAN_NULL])
                            ctx.sync()
                            assert n1[0] == 512
                            row = np.zeros(1024, np.uint8)
                            ctx.download(d_nrows, row)
                            if spec1 == 2:
                                want.append((1, sc.CHAN_NULL, blk, row))
                                seen["N1"] += 1
                                seen["PN"] += emitted_p
                            else:
                                seen["null_fed_rows_off"] += 1
            rx_of, inst_of, blk_of = told.spec_map()
            rows = told.spec_rows()
            assert [(int(a), int(b), int(c)) for a, b, c in zip(rx_of, inst_of, blk_of)] == [w[:3] for w in want], (step, list(zip(rx_of, inst_of, blk_of)), [w[:3] for w in want])
            for r, w in enumerate(want):
                bad = np.flatnonzero(rows[r] != w[3])
                assert bad.size == 0, (step, w[:3], "first differing byte", int(bad[0]), int(rows[r, bad[0]]), int(w[3][bad[0]]))
            assert 2 not in rx_of                                       # rx2 yields no rows
            assert plain.spec_map()[0].size == 0
        # the walk met every case of the rule
        assert seen["P0"] >= 16 and seen["P1"] >= 6 and seen["N1"] >= 5 and seen["PN"] == 3 and seen["null_fed_rows_off"] >= 1, seen
        # 3. a joined receiver starts with its rows off and a reset channel-null filter
        assert told.null_fir.pos(1) == 0
        told.join(1, None, None)
        told.set_wf(1, told.params[1], told.overlapped[1])
        told.set_audio(1, told.rx_inc[1], LO, HI, mode=SAM, sam_mparam=post.CHAN_NULL_LSB)
        nf.reset(0)                                                     # the standalone twin of the reset filter

        def null_rows_of_step():
            _, o = _step_outputs(told)
            a = np.ascontiguousarray(o["agc"]).view(np.complex64).reshape(NR, -1)
            got = []
            for blk in range(int(told.audio_map()[1][1]) // 512):
                ctx.upload(d_nin, np.ascontiguousarray(a[1, 512 * blk:512 * (blk + 1)]))
                nf.process_spec_dev([0], d_nin, 512, [512], None, 0, d_nrows, 1024, [sc.CHAN_NULL])
                ctx.sync()
                row = np.zeros(1024, np.uint8)
                ctx.download(d_nrows, row)
                got.append(row)
            return got

        for _ in range(2):
            told.step(d_adc)
            told.sync()
            rx_of, _, _ = told.spec_map()
            assert 1 not in rx_of and 0 in rx_of
            null_rows_of_step()
        told.set_spec(1, 2)
        told.step(d_adc)
        told.sync()
        rx_of, inst_of, _ = told.spec_map()
        mine = [r for r in range(rx_of.size) if rx_of[r] == 1]
        want = null_rows_of_step()
        assert mine and [int(inst_of[r]) for r in mine] == [sc.CHAN_NULL] * len(want)           # the mirror already says channel null
        rows = told.spec_rows()
        for r, w in zip(mine, want):
            assert np.array_equal(rows[r], w), "the joined receiver's channel-null filter did not start from zero history"
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        for d in bufs:
            ctx.free(d)
        pb.close()
        nf.close()
        told.close()
        plain.close()
