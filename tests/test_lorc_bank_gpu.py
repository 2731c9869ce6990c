"""The receiver bank's Loran-C extension (kg_rxbank_lorc_*; extensions/Loran_C/loran_c.cpp) against a standalone kg_lorc fed the bank's own
CFastFIR output, over a short script of commands: rx0 averages two chains under CMA and EMA, passes through NBFM (where it gets
nothing), has an offset moved, leaves and joins again; rx1 runs IIR under a fixed gain and is stopped and started; rx2 is never started.
Rows, row map and the whole end state are equal byte for byte.  Everything else the bank hands out is byte-identical to a second bank
that is stepped the same and never told about the extension, which holds nothing for it; a bank of twice the step gives the same rows
as the short steps; ten steps enqueued with no wait give what ten awaited steps give; the tap's one callback goes to the IQ display or
to Loran-C, never to both."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, lorc, post
from flydog_sdr_gps_amd._lib import ptr

from . import lorc_common as lc

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB, NBFM = post.MODE_SSB, post.MODE_NBFM
I_SRATE = 600                                   # a row behind every 601 samples: a step yields about 0.8 sound blocks
# before step k: (receiver, command line of tests/lorc_common.py with RATE for the bank's audio rate, or mode / leave / join)
SCRIPT = {0: [(0, "N RATE %d" % I_SRATE), (0, "I 0 2990"), (0, "I 1 4970"), (0, "A 1 1"), (0, "P 0 1"), (0, "P 1 6"), (0, "S"),
              (1, "N RATE %d" % I_SRATE), (1, "I 0 3970"), (1, "I 1 2990"), (1, "A 0 2"), (1, "A 1 2"), (1, "P 0 0.0005"), (1, "P 1 0.002"), (1, "G 0 -33"), (1, "S"),
              (2, "N RATE %d" % I_SRATE), (2, "I 0 2990"), (2, "I 1 2990")],
          4: [(0, "mode", NBFM)],
          7: [(0, "mode", USB), (1, "T")],
          9: [(1, "S"), (0, "O 0 77"), (0, "O 1 -5")],
          12: [(0, "leave")],
          14: [(0, "join")],
          15: [(0, "N RATE %d" % I_SRATE), (0, "I 0 4970"), (0, "I 1 2990"), (0, "A 0 1"), (0, "P 0 3"), (0, "P 1 1"), (0, "S")]}
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


def _tell(bank, rx, line):
    op, a = line[0], line[2:].split()
    {"N": lambda: bank.lorc_init(rx, float(a[0]), int(a[1])), "I": lambda: bank.lorc_set_gri(rx, int(a[0]), int(a[1])),
     "O": lambda: bank.lorc_set_offset(rx, int(a[0]), int(a[1])), "G": lambda: bank.lorc_set_gain(rx, int(a[0]), int(a[1])),
     "A": lambda: bank.lorc_set_avg_algo(rx, int(a[0]), int(a[1])), "P": lambda: bank.lorc_set_avg_param(rx, int(a[0]), float(a[1])),
     "S": lambda: bank.lorc_start(rx), "T": lambda: bank.lorc_stop(rx)}[op]()


def _state_equal(a, b, where):
    assert a["scalars"].tobytes() == b["scalars"].tobytes(), (where, a["scalars"], b["scalars"])
    assert a["avg"].tobytes() == b["avg"].tobytes(), where


def _rows_of(m, rows):
    return [(int(r["conn"]), int(r["ch"]), int(r["cmd"]), rows[int(r["off"]):int(r["off"]) + int(r["len"])].tobytes()) for r in m]


def test_a_bank_that_was_never_told_and_one_that_was(gpu_ctx):
    from flydog_sdr_gps_amd import live_allocs, synth
    ctx = gpu_ctx
    plain, told = _bank(), _bank()
    fs = told.fs
    sx = lorc.LoranC(ctx, nconn=NR)
    try:
        adc = synth.adc_stream(N, 0x5EED0F1A)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        assert told.lorc is None and plain.lorc is None
        held = live_allocs()
        mode = {rx: USB for rx in range(NR)}
        on = {rx: False for rx in range(NR)}
        seen = {"rows0": 0, "rows1": 0, "nbfm0": 0, "off1": 0, "reset": 0, "after_join": 0}
        for step in range(STEPS):
            for rx, what, *v in SCRIPT.get(step, []):
                if what == "mode":
                    for b in (told, plain):
                        b.post.set_mode(rx, v[0])
                    mode[rx] = v[0]
                elif what == "leave":
                    for b in (told, plain):
                        b.leave(rx)
                    on[rx] = False
                elif what == "join":
                    for b in (told, plain):
                        b.join(rx, None, None)
                        b.set_wf(rx, b.params[rx], b.overlapped[rx])
                        b.set_audio(rx, b.rx_inc[rx], LO, HI, mode=USB)
                    info, avg = told.lorc.state(rx)                      # a fresh object: all zero, stopped, waiting for its ext_server_init
                    assert not info["inited"] and not info["started"] and not avg.any() and not info["ch"]["nbucket"].any()
                    mode[rx], on[rx] = USB, False
                else:
                    line = what.replace("RATE", repr(float(fs)))
                    _tell(told, rx, line)
                    if line[0] == "N" and sx.state(rx)[0]["started"]:     # the standalone object's registration outlives the memset; a join ended it
                        sx.stop(rx)
                    lc.apply_command(sx, rx, line)
                    on[rx] = {"S": True, "T": False}.get(line[0], on[rx])
            if step == 0:                                               # the first command made the object and the rows; the slots were exchanged
                assert live_allocs() - held == 2 and told.lorc is not None
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
            fed = [rx for rx in range(NR) if on[rx] and mode[rx] != NBFM and int(nfir[rx]) >= 512]
            seen["nbfm0"] += int(on[0] and mode[0] == NBFM and int(nfir[0]) >= 512)
            seen["off1"] += int(not on[1] and int(nfir[1]) >= 512)
            m_got, rows_got = told.lorc_rows()
            if not fed:
                assert m_got.size == 0, step
                continue
            nblk = [int(nfir[rx]) // 512 for rx in fed]
            host = np.zeros((len(fed), max(nblk), 512), np.complex64)
            for i, rx in enumerate(fed):
                host[i, :nblk[i]] = firo[rx, :512 * nblk[i]].reshape(-1, 512)
            rows, m = sx.process(fed, host, nblk=nblk)
            for f in ("conn", "blk", "samp", "ch", "cmd", "len", "off"):
                assert np.array_equal(m_got[f], m[f]), (step, f, m_got[f], m[f])
            assert _rows_of(m_got, rows_got) == _rows_of(m, rows), step
            assert 2 not in m_got["conn"]
            seen["rows0"] += int((m["conn"] == 0).sum())
            seen["rows1"] += int((m["conn"] == 1).sum())
            seen["reset"] += int((m["cmd"] == lorc.SCOPE_RESET).sum())
            seen["after_join"] += int(step >= 15 and (m["conn"] == 0).any())
            if step in (11, 13, STEPS - 1):                             # before the leave, while rx0 is away, at the end
                for rx in range(NR):
                    if step != 13 or rx != 0:
                        _state_equal(lc.state_of(told.lorc, rx), lc.state_of(sx, rx), (step, rx))
        # the walk met every case
        assert seen["rows0"] >= 6 and seen["rows1"] >= 6 and seen["nbfm0"] >= 1 and seen["off1"] >= 1 and seen["reset"] >= 3 and seen["after_join"] >= 1, seen
        assert int(told.lorc.state(0)[0]["ch"][0]["gri"]) == 4970                  # the joined receiver started afresh
        # 3. the bank that was never told holds nothing for the extension
        assert plain.lorc is None and plain.lorc_rows()[0].size == 0
        # 4. the tap holds one callback: the IQ display or Loran-C
        told.iqd_init(2)
        told.iqd_set_run(2, 1, fs)
        with pytest.raises(KiwiGpuError):
            told.lorc_start(2)
        assert not told.lorc.state(2)[0]["started"]
        told.iqd_set_run(2, 0, fs)
        told.lorc_start(2)
        with pytest.raises(KiwiGpuError):
            told.iqd_set_run(2, 1, fs)
        assert not told.iqd.state(2)[0]["run"] and told.lorc.state(2)[0]["started"]
        told.lorc_stop(2)
        told.iqd_set_run(2, 1, fs)
        # 5. what a bank refuses beyond kg_lorc: a GRI of fewer than 128 samples
        before = lc.state_of(told.lorc, 1)
        with pytest.raises(KiwiGpuError):
            told.lorc_set_gri(1, 0, 900)
        _state_equal(lc.state_of(told.lorc, 1), before, "refused gri")
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def _start(b):
    for rx, lines in ((0, ["N RATE %d" % I_SRATE, "I 0 2990", "I 1 4970", "P 0 2", "P 1 2", "O 1 100", "S"]),
                      (2, ["N RATE %d" % I_SRATE, "I 0 3970", "I 1 3970", "A 0 1", "A 1 2", "P 0 5", "P 1 0.001", "G 1 -34", "S"])):
        for l in lines:
            _tell(b, rx, l.replace("RATE", repr(float(b.fs))))


def test_a_long_step_equals_the_same_blocks_as_short_steps(gpu_ctx):
    """a bank of 2 N samples a step against one of N over the same stream: the rows of each receiver, concatenated, and the end state"""
    from flydog_sdr_gps_amd import synth
    short, long_ = _bank(N), _bank(2 * N)
    try:
        adc = synth.adc_stream(2 * N, 0x5EED0F1B)
        half = adc.nbytes // 2
        d_s, d_l = short.ctx.alloc(adc.nbytes), long_.ctx.alloc(adc.nbytes)
        short.ctx.upload(d_s, adc)
        long_.ctx.upload(d_l, adc)
        got = {id(short): {0: [], 2: []}, id(long_): {0: [], 2: []}}
        for b in (short, long_):
            _start(b)

        def take(b):
            b.sync()
            m, rows = b.lorc_rows()
            for r in _rows_of(m, rows):
                got[id(b)][r[0]].append(r[1:])

        for _ in range(6):
            long_.step(d_l)
            take(long_)
            for k in range(2):
                short.step(d_s + k * half)
                take(short)
        for rx in (0, 2):
            assert len(got[id(long_)][rx]) >= 6 and got[id(long_)][rx] == got[id(short)][rx], rx
            _state_equal(lc.state_of(long_.lorc, rx), lc.state_of(short.lorc, rx), rx)
        short.ctx.free(d_s)
        long_.ctx.free(d_l)
    finally:
        short.close()
        long_.close()


def test_ten_steps_enqueued_with_no_wait_equal_the_stepwise_ones(gpu_ctx):
    """the host runs ahead: ten steps and a command between them with no wait against the same steps awaited one by one -- every step's
    row map (the host's), the last step's rows and the end state"""
    from flydog_sdr_gps_amd import synth
    wait, deep = _bank(), _bank()
    try:
        adc = synth.adc_stream(N, 0x5EED0F1C)
        d_w, d_d = wait.ctx.alloc(adc.nbytes), deep.ctx.alloc(adc.nbytes)
        wait.ctx.upload(d_w, adc)
        deep.ctx.upload(d_d, adc)
        maps = {id(wait): [], id(deep): []}
        for b, d, awaited in ((wait, d_w, True), (deep, d_d, False)):
            _start(b)
            b.step(d)                                                     # the first step of a bank drains by design
            b.sync()
            for k in range(10):
                if k == 5:
                    b.lorc_set_offset(0, 0, 33)                           # a command between two enqueued steps: host state only
                b.step(d)
                if awaited:
                    b.sync()
                m = np.zeros(64, lorc.row_dtype)
                n = b.lib.kg_rxbank_lorc_map(b.h, ptr(m), 64)
                assert n >= 0
                maps[id(b)].append(m[:n].tobytes())
            b.sync()
        assert maps[id(wait)] == maps[id(deep)] and sum(len(m) for m in maps[id(wait)]) >= 8 * 32
        mw, rw = wait.lorc_rows()
        md, rd = deep.lorc_rows()
        assert _rows_of(mw, rw) == _rows_of(md, rd)
        for rx in (0, 2):
            _state_equal(lc.state_of(wait.lorc, rx), lc.state_of(deep.lorc, rx), rx)
        wait.ctx.free(d_w)
        deep.ctx.free(d_d)
    finally:
        wait.close()
        deep.close()
