"""The receiver bank's IQ display (kg_rxbank_iqd_*; extensions/IQ_display/iq_display.cpp) against a standalone kg_iqd fed the bank's own
CFastFIR output, over a short script of commands: rx0 recovers a carrier in points mode, passes through NBFM (where it gets nothing),
is cleared, leaves and joins again; rx1 runs the MSK pair in density mode and is switched off and on; rx2 is never switched on.  Rows,
row map, status records, status map and the whole end state are equal byte for byte.  Everything else the bank hands out is
byte-identical to a second bank that is stepped the same and never told about the extension, which holds nothing for it; and a bank
of twice the step gives the same rows as the short steps."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import iqd, post

from . import iqd_common as ic

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB, NBFM = post.MODE_SSB, post.MODE_NBFM
# before step k: (receiver, command line of tests/iqd_common.py, or mode / leave / join).  A step yields about 0.8 sound blocks.
SCRIPT = {0: [(0, "N"), (0, "R 1 RATE"), (0, "M 1 1"), (0, "P 300"), (0, "G 60"), (1, "N"), (1, "M 2 200"), (1, "D 1"), (1, "P 100"), (1, "R 1 RATE")],
          4: [(0, "mode", NBFM)],
          7: [(0, "mode", USB), (1, "R 0 RATE")],
          9: [(1, "R 1 RATE"), (0, "C"), (0, "P 77")],
          12: [(0, "leave")],
          14: [(0, "join")],
          15: [(0, "N"), (0, "D 1"), (0, "R 1 RATE"), (1, "Y 1")]}
STEPS = 19


def _bank(n=N):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, n)
    bank.configure(MIXES["light"](NR, 0, n))
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=USB)
    return bank


def _outputs(bank):
    return [np.array(m).copy() for m in bank.audio_map()], {k: bank.fetch(k, list(range(NR))) for k in ("xin", "firo", "s16", "pay", "agc", "iq_pay")}


def _tell(bank, rx, line, fs):
    op, a = line[0], line[2:].split()
    {"N": lambda: bank.iqd_init(rx), "R": lambda: bank.iqd_set_run(rx, int(a[0]), fs), "G": lambda: bank.iqd_set_gain(rx, int(a[0])),
     "P": lambda: bank.iqd_set_points(rx, int(a[0])), "M": lambda: bank.iqd_set_pll_mode(rx, int(a[0]), int(a[1])),
     "W": lambda: bank.iqd_set_pll_bandwidth(rx, float(a[0])), "D": lambda: bank.iqd_set_draw(rx, int(a[0])),
     "Y": lambda: bank.iqd_set_display_mode(rx, int(a[0])), "C": lambda: bank.iqd_clear(rx)}[op]()


def _state_equal(a, b, where):
    for k in ("ints", "floats", "pll", "iq", "plot", "map"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (where, k)


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import live_allocs, synth
    ctx = gpu_ctx
    plain, told = _bank(), _bank()
    fs = told.fs
    sx = iqd.IqDisplay(ctx, nchan=NR)
    bufs = []
    try:
        adc = synth.adc_stream(N, 0x5EED0F18)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        MAXB = 8
        cap = NR * (512 * MAXB + ic.RING) * 4
        d_in, d_rows, d_st = ctx.alloc(NR * MAXB * 512 * 8), ctx.alloc(cap), ctx.alloc(24 * NR * MAXB)
        bufs = [d_in, d_rows, d_st]
        assert told.iqd is None and plain.iqd is None
        held = live_allocs()
        mode = {rx: USB for rx in range(NR)}
        on = {rx: False for rx in range(NR)}
        live = {rx: True for rx in range(NR)}
        seen = {"rows0": 0, "rows1": 0, "nbfm0": 0, "off1": 0, "sent": 0, "after_join": 0}
        for step in range(STEPS):
            for rx, what, *v in SCRIPT.get(step, []):
                if what == "mode":
                    for b in (told, plain):
                        b.post.set_mode(rx, v[0])
                    mode[rx] = v[0]
                elif what == "leave":
                    for b in (told, plain):
                        b.leave(rx)
                    sx.init(rx)
                    on[rx], live[rx] = False, False
                elif what == "join":
                    for b in (told, plain):
                        b.join(rx, None, None)
                        b.set_wf(rx, b.params[rx], b.overlapped[rx])
                        b.set_audio(rx, b.rx_inc[rx], LO, HI, mode=USB)
                    sx.init(rx)
                    mode[rx], on[rx], live[rx] = USB, False, True
                else:
                    line = what.replace("RATE", repr(float(fs)))
                    _tell(told, rx, line, fs)
                    r = ic.apply_command(sx, rx, line)
                    if r is not None:
                        on[rx] = r
            if step == 0:                                               # the first command made the object: its state, the rows, the status records
                assert live_allocs() - held == 3 and told.iqd is not None
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            maps, out = _outputs(told)
            maps2, out2 = _outputs(plain)
            # 1. nothing else changes
            for a, b in zip(maps, maps2):
                assert np.array_equal(a, b), step
            nfir = maps[1]
            for rx in range(NR):
                n = int(nfir[rx])
                for k, per in (("firo", 1), ("s16", 1), ("agc", 1), ("pay", 0.5), ("iq_pay", 4)):
                    m = int(n * per)
                    assert np.array_equal(np.ascontiguousarray(out[k][rx, :m]).view(np.uint8), np.ascontiguousarray(out2[k][rx, :m]).view(np.uint8)), (step, rx, k)
            # 2. the standalone object on the bank's own filter output
            firo = np.ascontiguousarray(out["firo"]).view(np.complex64).reshape(NR, -1)
            fed = [rx for rx in range(NR) if live[rx] and on[rx] and mode[rx] != NBFM and int(nfir[rx]) >= 512]
            seen["nbfm0"] += int(live[0] and on[0] and mode[0] == NBFM and int(nfir[0]) >= 512)
            seen["off1"] += int(not on[1] and int(nfir[1]) >= 512)
            m_got, rows_got = told.iqd_rows()
            st_got, rx_of, blk_of, sent_got = told.iqd_status()
            if not fed:
                assert m_got.size == 0 and st_got.size == 0, step
                continue
            nblk = [int(nfir[rx]) // 512 for rx in fed]
            host = np.zeros((len(fed), MAXB * 512), np.complex64)
            for i, rx in enumerate(fed):
                host[i, :512 * nblk[i]] = firo[rx, :512 * nblk[i]]
            ctx.upload(d_in, host)
            m, sent = sx.process_dev(fed, nblk, [0] * len(fed), 512, d_in, MAXB * 512, d_rows, cap, d_st, NR * MAXB, 512 * NR * MAXB)
            ctx.sync()
            used = int(m["off"][-1] + m["len"][-1]) if m.size else 0
            rows, st = np.zeros(max(used, 1), np.uint8), np.zeros(sum(nblk), iqd.status_dtype)
            ctx.download(d_rows, rows)
            ctx.download(d_st, st)
            for f in ("ch", "blk", "samp", "cmd", "len", "off"):
                assert np.array_equal(m_got[f], m[f]), (step, f, m_got[f], m[f])
            assert np.array_equal(rows_got, rows[:used]), step
            assert st_got.tobytes() == st.tobytes() and np.array_equal(sent_got, sent), step
            assert rx_of.tolist() == [rx for i, rx in enumerate(fed) for _ in range(nblk[i])] and blk_of.tolist() == [b for n in nblk for b in range(n)]
            assert 2 not in m_got["ch"]
            seen["rows0"] += int((m["ch"] == 0).sum())
            seen["rows1"] += int((m["ch"] == 1).sum())
            seen["sent"] += int(sent.sum())
            seen["after_join"] += int(step >= 15 and (m["ch"] == 0).any())
            if step in (11, 13, STEPS - 1):                             # before the leave, while rx0 is away, at the end
                for rx in range(2):
                    _state_equal(ic.state_of(told.iqd, rx), ic.state_of(sx, rx), (step, rx))
        # the walk met every case
        assert seen["rows0"] >= 5 and seen["rows1"] >= 20 and seen["nbfm0"] >= 1 and seen["off1"] >= 1 and seen["sent"] >= 1 and seen["after_join"] >= 1, seen
        assert int(told.iqd.state(0)[0]["draw"]) == iqd.DENSITY and int(told.iqd.state(0)[0]["points"]) == 1024      # the joined receiver started afresh
        # 3. the bank that was never told holds nothing for the extension
        assert plain.iqd is None and plain.iqd_rows()[0].size == 0 and plain.iqd_status()[0].size == 0
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        for d in bufs:
            ctx.free(d)
        sx.close()
        told.close()
        plain.close()


def test_a_long_step_equals_the_same_blocks_as_short_steps(gpu_ctx):
    """a bank of 2 N samples a step against one of N over the same stream: the rows of each receiver, concatenated, and the end state"""
    from flydog_sdr_gps_amd import synth
    short, long_ = _bank(N), _bank(2 * N)
    try:
        adc = synth.adc_stream(2 * N, 0x5EED0F19)
        half = adc.nbytes // 2
        d_s, d_l = short.ctx.alloc(adc.nbytes), long_.ctx.alloc(adc.nbytes)
        short.ctx.upload(d_s, adc)
        long_.ctx.upload(d_l, adc)
        for b in (short, long_):
            for rx, lines in ((0, ["N", "R 1 12000", "M 1 2", "P 300", "G 60"]), (2, ["N", "R 1 12000", "M 0 0", "P 33", "D 1"])):
                for l in lines:
                    _tell(b, rx, l, b.fs)
        got = {id(short): {0: [], 2: []}, id(long_): {0: [], 2: []}}
        sent = {id(short): [], id(long_): []}

        def take(b):
            b.sync()
            m, rows = b.iqd_rows()
            for r in m:
                got[id(b)][int(r["ch"])].append((int(r["cmd"]), rows[r["off"]:r["off"] + r["len"]].tobytes()))
            st, rx_of, _, snt = b.iqd_status()
            sent[id(b)] += sorted((int(rx), st[k].tobytes()) for k, rx in enumerate(rx_of) if snt[k])

        for _ in range(6):
            long_.step(d_l)
            take(long_)
            for k in range(2):
                short.step(d_s + k * half)
                take(short)
        for rx in (0, 2):
            assert len(got[id(long_)][rx]) >= 8 and got[id(long_)][rx] == got[id(short)][rx], rx
            _state_equal(ic.state_of(long_.iqd, rx), ic.state_of(short.iqd, rx), rx)
        assert len(sent[id(long_)]) >= 2 and sorted(sent[id(long_)]) == sorted(sent[id(short)])
        short.ctx.free(d_s)
        long_.ctx.free(d_l)
    finally:
        short.close()
        long_.close()
