"""Long steps equal short steps, byte for byte.  kg_rxbank_step can complete several 512-sample sound blocks per receiver in one step, and
everything the bank gained since its first demodulators is indexed by sound block inside the step: the per-block channel lists, null_row,
the FFT extension's spectra, pb_n / pb_base, the offsets into s16 / pay / iq_pay / agc, the per-block kg_post calls.  Behind the DDC the
audio side is a stream machine (the DDC, the blanker, CFastFIR's block positions, and every stage behind them advance per sample or per
512-sample block, whatever call the samples arrived in), so the truth for a long-step bank is a second bank stepped over the same stream
in short steps with the same commands at the same sample positions (tests/rxbank_stepsize.py) -- the regime the rest of the suite holds
to the oracle and to standalone chains.  Equality; no tolerance; nothing left out.

(a) every feature at 3 to 4 blocks a step against single-block steps; (b) the largest step there is, 2^27 samples of the rx3 instance (42
to 43 blocks, blocks_max = 43), against 5 to 6 blocks a step; (c) the create-time boundary."""
import numpy as np
import pytest

from . import rxbank_stepsize as ss

pytestmark = pytest.mark.gpu

KG_ERR_INVALID = -2
L = ss.BLOCK


@pytest.fixture(scope="module")
def stream():
    return ss.stream_blocks()


def _equalities(long, short, ratio, nrx):
    """every collected stream, row sequence and end state; the info / nrec / nfir sums over the matching steps"""
    diff = ss.first_difference(long, short, nrx)
    assert diff is None, ("(receiver, what, ...) of the first difference, long bank then short bank", diff)
    for k, rec in enumerate(long["steps"]):
        sh = short["steps"][ratio * k:ratio * (k + 1)]
        for f in ("nrec", "nfir"):
            assert rec["info"][f] == sum(s["info"][f] for s in sh), (k, "info", f)
            assert np.array_equal(rec[f], sum(s[f] for s in sh)), (k, f, rec[f], [s[f] for s in sh])
        assert np.array_equal(rec["seq0"], sh[0]["seq0"]), (k, "snd_seq before the step")
        assert rec["info"]["snd_seq"] == sh[0]["info"]["snd_seq"] and rec["info"]["fir_pos"] == sh[-1]["info"]["fir_pos"], k
        assert rec["info"]["nframes"] == sh[0]["info"]["nframes"] and rec["info"]["nmoves"] == 0, k


def _waterfall(long, short, ratio):
    """A one-shot frame of long step k starts on the sample short step ratio * k starts on, with the same NCO phase and snd_seq: the same
    row and the same packet.  Nothing else of the waterfall is compared: a frame per step depends on the step size by definition.  (The
    waterfall's NB_STD blanker carries its magnitude average from frame to frame, rx_waterfall.cpp:1098, so the start of a blanked
    receiver's frame is judged against another past in the two banks; the blanker only ever passes a sample or zeroes it, and over this
    stream it decides the same in both: the blanked receiver is held like the others.)"""
    for k, rec in enumerate(long["steps"]):
        sh = short["steps"][ratio * k]
        assert sorted(rec["frames"]) == sorted(sh["frames"]), k
        for rx, (row, pkt) in rec["frames"].items():
            assert row == sh["frames"][rx][0], (k, rx, "waterfall row")
            assert pkt == sh["frames"][rx][1], (k, rx, "waterfall packet")


def test_every_feature_several_blocks_a_step(stream):
    """Eight receivers in the default 12 kHz mode, eight steps of 2^24 samples against thirty-two of 2^22 over two alternating blocks:

      rx  mode                       with
      0   AM, de-emphasis            NB_STD on audio and waterfall; `SET mod=` to SSB before long step 5
      1   SSB                        `SET spc_=2`, NB_WILD
      2   NBFM, squelch 80
      3   SAM, channel null (LSB)    `SET spc_=2`; the extension's spectrum, chosen in SAM
      4   IQ, little-endian          the extension's waterfall
      5   QAM, big-endian            leaves before long step 2, joins before long step 4
      6   SSB                        NR (WDSP LMS, denoise + auto-notch); `SET nr algo=3` (NR_SPECTRAL) before long step 4
      7   SAS                        the extension's integrator, itime 0.1; `SET clear` before long step 5
    """
    from flydog_sdr_gps_amd import fftext, post
    table = ss.features()
    nrx = len(table)
    script = {2 * L: [(5, "leave", None)],
              4 * L: [(5, "join", None), (6, "nr", ss.NR_SPECTRAL)],
              5 * L: [(0, "audio", dict(lo=300.0, hi=2700.0, mode=post.MODE_SSB)), (7, "fx_clear", None)]}
    long = ss.run(L, 8, stream, script, table=table)
    short = ss.run(L >> 2, 32, stream, script, table=table)
    # the test cannot pass without reaching what it is for
    per_step = [ss.blocks(rec) for rec in long["steps"]]
    print("sound blocks per receiver, long steps:", per_step)
    assert all(max(b[rx] for b in per_step) >= 3 for rx in range(nrx)), per_step
    assert any(len({n for n in b if n > 0}) >= 2 for b in per_step), ("no step with two block counts", per_step)
    seen = set()
    for rec in long["steps"]:
        seen |= {("spec", inst) for _, inst, blk in rec["blk_spec"] if blk >= 1}
        seen |= {("fx", rx) for rx, blk in rec["blk_fx"] if blk >= 1}
        for rx, nblk in enumerate(ss.blocks(rec)):
            if nblk >= 2:
                seen.add("adpcm" if not rec["stereo"][rx] else ("iq_le" if rec["le"][rx] else "iq_be"))
    want = {("spec", fftext.CHAN_NULL), ("spec", fftext.PASSBAND), ("fx", 3), ("fx", 4), ("fx", 7), "adpcm", "iq_le", "iq_be"}
    assert want <= seen, sorted(map(str, want - seen))
    assert max(max(ss.blocks(rec)) for rec in short["steps"]) == 1, "a short step with two blocks"
    assert any(rec["blk_spec"] for rec in short["steps"]) and any(rec["blk_fx"] for rec in short["steps"])
    _equalities(long, short, 4, nrx)
    _waterfall(long, short, 4)


def test_the_largest_step(stream):
    """RX_WIDE at n = 2^27: 21746 records, 42 to 43 sound blocks a step (blocks_max = 43, the most kg_rxbank_create accepts in any mode),
    with every per-block table kind staged in every block: SSB + NB_STD, channel-null SAM with rows and the extension's spectrum, IQ
    little-endian, QAM big-endian.  THREE long steps against twenty-four of 2^24 (5 to 6 blocks each, which (a) ties to single-block
    steps) over one 2^24-sample block tiled eight times: 42.47 blocks a step leave FirPos() at 242 and 484 after two steps of 42
    blocks, and only the third step has all 43 (16 + 5 * 43 = 231 of the 244 table entries).  A step that did not fit its table slot
    or staged another number of tables than it planned would refuse (KG_ERR_NOMEM / KG_ERR_STATE): RxBank.step raises on anything
    but KG_OK."""
    from flydog_sdr_gps_amd.ddc import RX_WIDE
    table = ss.largest()
    adc = [stream[0]] * 8
    long = ss.run(1 << 27, 3, adc, {}, rx_mode=RX_WIDE, table=table)
    short = ss.run(L, 24, adc, {}, rx_mode=RX_WIDE, table=table)
    per_step = [ss.blocks(rec) for rec in long["steps"]]
    print("sound blocks per receiver, long steps:", per_step, "table bytes:", [rec["info"]["table_bytes"] for rec in long["steps"]])
    assert all(rec["info"]["table_bytes"] > 0 for rec in long["steps"])
    assert all(42 <= n <= 43 for b in per_step for n in b) and any(n == 43 for b in per_step for n in b), per_step
    assert all(5 <= n <= 6 for rec in short["steps"] for n in ss.blocks(rec))
    for rec in long["steps"]:                               # rows of both kinds and of the extension up to the last block
        assert max(blk for _, inst, blk in rec["blk_spec"] if inst == 1) >= 41 and max(blk for _, blk in rec["blk_fx"]) >= 41
    _equalities(long, short, 8, len(table))
    _waterfall(long, short, 8)


@pytest.mark.parametrize("wide", [False, True])
def test_create_time_boundary(wide):
    """kg_rxbank_create's two rules for the step.  Its table rule, 16 + 5 * blocks_max <= KG_ARENA_MAX_ENTRIES (244), allows 45 sound
    blocks: a step of (45 - 1) * 512 * decim_rx samples.  Its first rule allows 2^27 samples, and in BOTH instances that is the smaller
    one (44 * 512 * 10416 and 44 * 512 * 6172 are 1.75 and 1.04 times 2^27; 2^27 samples are 26 and 43 blocks): the largest accepted
    step, n_max, is the smaller of the two.  A bank created with n_max steps; the first n whose blocks_max is 46 is refused at create
    with KG_ERR_INVALID and nothing is left allocated."""
    from flydog_sdr_gps_amd import KiwiGpuError, live_allocs, post
    from flydog_sdr_gps_amd.ddc import RX_DECIM, RX_DECIM_WIDE, RX_STD, RX_WIDE
    from flydog_sdr_gps_amd.rxbank import RxBank
    decim, mode = (RX_DECIM_WIDE, RX_WIDE) if wide else (RX_DECIM, RX_STD)
    blocks_max = lambda n: (n // decim + 2) // 512 + 1     # kg_rxbank_create's own arithmetic
    n_max = min((45 - 1) * 512 * decim // 8192 * 8192, 1 << 27)
    assert blocks_max(n_max) <= 45
    held = live_allocs()
    table = [dict(zoom=8, audio=dict(lo=300.0, hi=2700.0, mode=post.MODE_SSB)),
             dict(zoom=9, audio=dict(lo=-4900.0, hi=4900.0, mode=post.MODE_SAM, sam_mparam=post.CHAN_NULL_LSB), spec=2)]
    mix = ss._mix(table, n_max)
    bank = RxBank(2, n_max, rx_mode=mode)
    try:
        assert bank.rxddc.decim == decim
        bank.wf.set_tables()
        for rx, row in enumerate(table):
            ss._connect(bank, rx, row, mix, join=False)
        zeros = np.zeros(1 << 22, np.int16)
        d_adc = bank.ctx.alloc(2 * n_max)
        for at in range(0, n_max, zeros.size):
            bank.ctx.upload(d_adc + 2 * at, zeros[:min(zeros.size, n_max - at)])
        info = bank.step(d_adc)
        bank.sync()
        nrec, nfir, _, _ = bank.audio_map()
        print("n_max", n_max, "blocks_max", blocks_max(n_max), "records", nrec.tolist(), "blocks", (nfir // 512).tolist(), "table bytes", info.table_bytes)
        assert info.table_bytes > 0 and (nrec >= n_max // decim - 1).all() and (nfir // 512 >= blocks_max(n_max) - 2).all()
        rx_of, inst, blk = bank.spec_map()
        assert (inst == 1).any() and blk.max() == nfir[1] // 512 - 1      # the channel null's rows up to the step's last block
        bank.ctx.free(d_adc)
    finally:
        bank.close()
    assert live_allocs() == held
    n46 = next(n for n in range((45 * 512 - 2) * decim // 8192 * 8192, 1 << 62, 8192) if blocks_max(n) == 46)
    assert blocks_max(n46 - 8192) <= 45
    with pytest.raises(KiwiGpuError) as e:
        RxBank(2, n46, rx_mode=mode)
    assert e.value.status == KG_ERR_INVALID
    assert live_allocs() == held
