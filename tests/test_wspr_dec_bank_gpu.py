"""Stage 2 of the WSPR extension in the receiver bank (kg_rxbank_wspr_set_metric_table / _set_decode / _dec_out): with decode on, the step
that holds a receiver's cycle end enqueues pass 0 behind the cycle-end launch and announces it by KG_WSPR_EV_DECODES.  The bank's records
equal a standalone kg_wspr with set_decode on, fed the bank's own CFastFIR output, over the steps around the cycle ends of two
receivers; every other output of every step is byte-identical to a bank never told; a later pass by the host on the bank's object equals
the standalone one; long steps equal short ones; steps enqueued with no wait equal awaited ones; leave and join clear records, held
candidates and ignore."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import post, wspr

from . import wspr_dec_common as W

pytestmark = pytest.mark.gpu

N = 1 << 22
NR = 3
LO, HI = -4900.0, 4900.0
USB = post.MODE_SSB
STEPS = 18                                      # of 8 N: 6.4 sound blocks a step; group 85 is due in the 87th block


def _bank(n):
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, n)
    bank.configure(MIXES["light"](NR, 0, n))
    for rx in range(NR):
        bank.set_audio(rx, mix[rx][2], LO, HI, mode=USB)
    return bank


def test_the_banks_pass_0_equals_the_standalone_objects(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    g = W.load()
    n = 8 * N
    plain, told = _bank(n), _bank(n)
    sx = wspr.Wspr(gpu_ctx, nconn=NR)
    try:
        adc = synth.adc_stream(n, 0x5EED0F3A)
        d_adc, d_adc2 = told.ctx.alloc(adc.nbytes), plain.ctx.alloc(adc.nbytes)
        told.ctx.upload(d_adc, adc)
        plain.ctx.upload(d_adc2, adc)
        assert told.wspr_dec_out() == {} and told.wspr is None                    # asking does not make the object
        told.wspr_set_metric_table(g["mettab"])
        sx.set_metric_table(g["mettab"])
        for who in (lambda f: getattr(told, "wspr_" + f), lambda f: getattr(sx, f)):
            who("init")(0, 375.0)
            who("set_capture")(0, 1)
            who("set_decode")(0, 1)
        on = {0: True, 1: False, 2: False}
        ends, clock = [], (0, 0)
        for step in range(STEPS):
            if step == 1:
                clock = (1, 7)
            if step == 2:                                                          # rx1 joins the capture later, free running: its cycle ends two steps behind rx0's
                for who in (lambda f: getattr(told, "wspr_" + f), lambda f: getattr(sx, f)):
                    who("init")(1, 375.0)
                    who("set_capture")(1, 1)
                    who("set_decode")(1, 1)
                on[1] = True
            told.wspr_set_now(*clock)
            told.step(d_adc)
            plain.step(d_adc2)
            told.sync()
            plain.sync()
            maps, maps2 = [np.array(m).copy() for m in told.audio_map()], [np.array(m).copy() for m in plain.audio_map()]
            for a, b in zip(maps, maps2):                                          # every other output: the bank never told
                assert np.array_equal(a, b), step
            nfir = maps[1]
            out, out2 = ({k: b.fetch(k, list(range(NR))) for k in ("firo", "s16")} for b in (told, plain))
            for rx in range(NR):
                for k in ("firo", "s16"):
                    m = int(nfir[rx])
                    assert np.array_equal(np.ascontiguousarray(out[k][rx, :m]).view(np.uint8), np.ascontiguousarray(out2[k][rx, :m]).view(np.uint8)), (step, rx, k)
            firo = np.ascontiguousarray(out["firo"]).view(np.complex64).reshape(NR, -1)
            fed = [rx for rx in range(NR) if on[rx] and int(nfir[rx]) >= 512]
            rows_got, m_got, ev_got, cyc_got, cnt_got = told.wspr_out()
            nblk = [int(nfir[rx]) // 512 for rx in fed]
            host = np.zeros((len(fed), max(nblk), 512), np.complex64)
            for i, rx in enumerate(fed):
                host[i, :nblk[i]] = firo[rx, :512 * nblk[i]].reshape(-1, 512)
            rows, m, ev, cyc, counts = sx.push(fed, host, clock[0], clock[1], nblk=nblk)
            assert ev_got.tobytes() == ev.tobytes(), (step, ev_got, ev)
            decs = told.wspr_dec_out()
            due = [rx for i, rx in enumerate(fed) if cyc[i]["due"]]
            assert sorted(decs) == due == sorted(int(e["conn"]) for e in ev if e["kind"] == wspr.EV_DECODES), step
            for rx in due:                                                         # a step without a cycle end announces and hands out nothing
                want = sx.decodes(rx)
                assert want.size == cyc_got[rx]["npk"] >= 1 and decs[rx].tobytes() == want.tobytes(), (step, rx)
                ends.append((step, rx))
        assert [rx for _, rx in ends] == [0, 1] and ends[0][0] < ends[1][0], ends
        # a later pass is the host's, between steps, on the bank's own object: equal to the standalone one, ignore carried from pass 0
        for rx in (0, 1):
            a, na = told.wspr.decode([rx], 1000, 1)
            b, nb = sx.decode([rx], 1000, 1)
            assert na[0] == nb[0] >= 1 and a.tobytes() == b.tobytes(), rx
            assert (a[0][:na[0]]["result"][sx.decodes(rx)["ignore"] == 1] == wspr.SKIPPED).all()
        assert plain.wspr is None and plain.wspr_dec_out() == {}
        # leave and join: no records, no held candidates, no ignore, decode off
        assert told.wspr.decodes(1).size >= 1
        told.leave(1)
        told.join(1, None, None)
        assert told.wspr.decodes(1).size == 0
        told.wspr_init(1, 375.0)
        out, nc = told.wspr.decode([1], 200, 2)
        assert nc[0] == 0 and not out.tobytes().strip(b"\0")
        told.ctx.free(d_adc)
        plain.ctx.free(d_adc2)
    finally:
        sx.close()
        told.close()
        plain.close()


def test_long_steps_short_steps_and_steps_with_no_wait_give_the_same_records(gpu_ctx):
    """one stream through a bank of 8 N samples a step awaited step by step, through one of 4 N, and through one of 8 N whose steps are
    enqueued with no wait: the events of all steps and the records of pass 0 are the same"""
    from flydog_sdr_gps_amd import synth
    g = W.load()
    banks = {"long": _bank(8 * N), "short": _bank(4 * N), "deep": _bank(8 * N)}
    try:
        adc = synth.adc_stream(8 * N, 0x5EED0F3B)
        half = adc.nbytes // 2
        evs, recs, d = {}, {}, {}
        for name, b in banks.items():
            d[name] = b.ctx.alloc(adc.nbytes)
            b.ctx.upload(d[name], adc)
            b.wspr_set_metric_table(g["mettab"])
            b.wspr_init(0, 375.0)
            b.wspr_set_capture(0, 1)
            b.wspr_set_decode(0, 1)
            evs[name] = []

        def take(b, name):
            import ctypes as C
            ev, ne = np.zeros(64, wspr.ev_dtype), C.c_int32()
            b.lib.kg_rxbank_wspr_out(b.h, None, None, None, None, 0, None, ev.ctypes.data_as(C.c_void_p), 64, C.byref(ne), None, 0)       # the host's part: no wait
            evs[name] += [(int(e["conn"]), int(e["kind"]), int(e["a"]), int(e["b"])) for e in ev[:ne.value]]

        for k in range(16):
            for name, b in banks.items():
                b.wspr_set_now(*((0, 0) if k == 0 else (1, 30)))
                for h in range(2 if name == "short" else 1):
                    b.step(d[name] + h * half)
                    if name != "deep" or k == 0:                               # the first step of a bank drains by design
                        b.sync()
                    take(b, name)
        for name, b in banks.items():
            b.sync()
            recs[name] = b.wspr.decodes(0)
        assert recs["long"].size >= 1 and recs["long"].tobytes() == recs["short"].tobytes() == recs["deep"].tobytes()
        assert sum(e[1] == wspr.EV_DECODES for e in evs["long"]) == 1
        assert evs["long"] == evs["deep"] and sorted(evs["long"]) == sorted(evs["short"])
        for name, b in banks.items():
            b.ctx.free(d[name])
    finally:
        for b in banks.values():
            b.close()
