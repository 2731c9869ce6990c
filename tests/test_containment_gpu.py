"""Containment of the device entry points of include/kiwigpu.h, part 1: the wire formats, the data-pump unpack, CFastFIR, the audio
spectrum rows, the noise blanker and the libm arrays.  (Part 2: tests/test_containment_post_gpu.py, kg_post; part 3:
tests/test_containment_ddc_gpu.py, the DDCs, the waterfall and the input-only entry points; tests/test_containment_bank_gpu.py: the
receiver bank's buffers.)

Every case runs through tests/guarded.py's contain(): the same call from a fresh object on three layouts -- guard bands and row gaps
of the inputs filled with 0x00 (the output buffers with 0xFF), with 0xFF (outputs 0x00), and the tight layout of the parity tests --
and asserts, bit for bit,
  W  nothing outside the stated extent of an output row is written, and no input byte changes;
  R  no byte outside the stated input extents reaches an output, a count or the object's state (0x00 against 0xFF: as float NaN,
     as int16 -1, as a record byte 255);
  P  no output depends on what its row held before the call;
  E  the guarded layout gives what the tight layout gives.
Strides are the used size plus an odd number of elements, row 0 sits at the smallest alignment the header allows, and the channel
lists are out of order."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import FastFir, snd, wire
from flydog_sdr_gps_amd._lib import check, ptr
from flydog_sdr_gps_amd.nb import NoiseBlanker
from flydog_sdr_gps_amd.wire import Adpcm
from tests.guarded import contain

pytestmark = pytest.mark.gpu

KG_ERR_INVALID = -2


def c64(rng, n, amp=1000.0):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp).astype(np.complex64)


def i16(rng, n):
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    x[:min(n, 4)] = [-32768, 32767, -1, 0][:min(n, 4)]
    return x


# ---------------------------------------------------------------------------------------------------------------- wire formats
@pytest.mark.parametrize("nsamps", [2, 130, 512])
def test_adpcm_encode(gpu_ctx, oracle, nsamps):
    chans = [2, 0, 1]
    rng = np.random.default_rng(nsamps)
    x = [i16(rng, nsamps) // 4 for _ in chans]

    def case(lay):
        a = Adpcm(gpu_ctx, nchan=4)
        try:
            a.set_state(0, 17, -300)
            g_in, s_in = lay.inp(x, 2)
            g_out, s_out = lay.out(len(chans), nsamps // 2, 1, 1)
            a.encode_dev(chans, g_in.ptr, s_in, nsamps, g_out.ptr, s_out)
            gpu_ctx.sync()
            return lay.take(g_out, nsamps // 2), [a.get_state(c) for c in range(4)]
        finally:
            a.close()

    rows, _ = contain(gpu_ctx, case)
    for i, ch in enumerate(chans):
        st = oracle.adpcm_encode_i16(x[i], state=oracle.AdpcmState(17, -300) if ch == 0 else None)
        want = st[0]
        assert rows[i][2] == np.asarray(want, np.uint8).tobytes(), ch


@pytest.mark.parametrize("little_endian", [0, 1])
@pytest.mark.parametrize("nsamps", [1, 65, 512])
def test_snd_payload(gpu_ctx, nsamps, little_endian):
    rng = np.random.default_rng(nsamps)
    x = [i16(rng, nsamps) for _ in range(3)]

    def case(lay):
        g_in, s_in = lay.inp(x, 2)
        g_out, s_out = lay.out(3, 2 * nsamps, 1, 2, pad=6, mult=2)                     # out_stride: bytes, even
        check(gpu_ctx.lib.kg_snd_payload_dev(gpu_ctx.h, ptr(g_in.ptr), s_in, 3, nsamps, little_endian, ptr(g_out.ptr), s_out),
              "kg_snd_payload_dev")
        gpu_ctx.sync()
        return lay.take(g_out, 2 * nsamps)

    rows = contain(gpu_ctx, case)
    for i in range(3):
        assert rows[i][2] == (x[i] if little_endian else x[i].byteswap()).tobytes()


@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("little_endian", [0, 1])
@pytest.mark.parametrize("nsamps", [1, 65, 512])
def test_snd_iq_payload(gpu_ctx, oracle, nsamps, little_endian, with_list):
    rng = np.random.default_rng(nsamps)
    x = [c64(rng, nsamps, 20000.0) for _ in range(3)]                                  # some samples leave the int16 range
    lst = np.array([2, 0, 1], np.int32)

    def case(lay):
        g_in, s_in = lay.inp(x, 8)
        g_out, s_out = lay.out(3, 4 * nsamps, 1, 2, pad=6, mult=2)
        check(gpu_ctx.lib.kg_snd_iq_payload_dev(gpu_ctx.h, ptr(lst) if with_list else None, 3, ptr(g_in.ptr), s_in, nsamps, little_endian,
                                                ptr(g_out.ptr), s_out), "kg_snd_iq_payload_dev")
        gpu_ctx.sync()
        return lay.take(g_out, 4 * nsamps)

    rows = contain(gpu_ctx, case)
    for i in range(3):                                     # on a context of its own the rows go by position, with a list or without
        assert rows[i][2] == np.asarray(oracle.snd_iq_payload(x[i], little_endian)).tobytes()


def test_wf_packets(gpu_ctx, oracle):
    rng = np.random.default_rng(5)
    rows_in = [rng.integers(0, 256, 1024).astype(np.uint8) for _ in range(3)]
    infos = [(100, 0, 7, 1), (2000, 3, 8, 1), (30000, 3, 9, 0)]        # zoom 0 with compression asked (never compressed), zoom 3 both ways

    def case(lay):
        g_in, s_in = lay.inp(rows_in, 1)
        g_out, s_out = lay.out(3, wire.WF_PKT_MAX, 1, 1, pad=6)
        nb = wire.wf_packets_dev(gpu_ctx, g_in.ptr, s_in, infos, g_out.ptr, s_out)
        gpu_ctx.sync()
        return lay.take(g_out, [int(b) for b in nb]), nb

    pk, nb = contain(gpu_ctx, case)
    assert np.frombuffer(nb[2], np.int32).tolist() == [16 + 1024, 16 + 517, 16 + 1024]
    for i, (xb, zoom, seq, comp) in enumerate(infos):
        want = np.asarray(oracle.wf_packet(rows_in[i], xb, zoom, seq, comp), np.uint8)
        assert pk[i][2] == want.tobytes(), i


# ------------------------------------------------------------------------------------------------------------ data-pump unpack
@pytest.mark.parametrize("rows_layout", [False, True])
@pytest.mark.parametrize("nsamps", [1, 85, 173])
def test_dpump_unpack(gpu_ctx, oracle, nsamps, rows_layout):
    nchans = 3
    rng = np.random.default_rng(nsamps)
    spi = snd.pack_rx_iq(rng.integers(-2 ** 23, 2 ** 23, (nsamps, nchans)), rng.integers(-2 ** 23, 2 ** 23, (nsamps, nchans)))
    spi = np.ascontiguousarray(spi, np.uint8).reshape(nsamps, nchans, 6)
    en = np.array([1, 0, 1], np.uint8)                                               # channel 1 is disabled: its row stays untouched
    used = [8 * nsamps if e else 0 for e in en]

    def case(lay):
        g_out, s_out = lay.out(nchans, nsamps, 8, 8)
        if rows_layout:
            g_in, s_in = lay.inp([spi[:, ch].copy() for ch in range(nchans)], 2, elem=6)
            snd.unpack_rows_dev(gpu_ctx, g_in.ptr, s_in, nsamps, nchans, g_out.ptr, s_out, enabled=en, dc_i=0.25, dc_q=-1.5)
        else:
            g_in, _ = lay.inp([spi], 2, elem=6)
            check(gpu_ctx.lib.kg_dpump_unpack_dev(gpu_ctx.h, ptr(g_in.ptr), nsamps, nchans, ptr(en), snd.RESCALE, 0.25, -1.5, 0,
                                                  ptr(g_out.ptr), s_out), "kg_dpump_unpack_dev")
        gpu_ctx.sync()
        return lay.take(g_out, used)

    rows = contain(gpu_ctx, case)
    want = oracle.dpump_unpack(spi.reshape(-1), nsamps, nchans, enabled=np.ones(nchans, np.uint8), dc_i=0.25, dc_q=-1.5)
    for ch in range(nchans):
        assert rows[ch][2] == (want[ch].tobytes() if en[ch] else b""), ch


# -------------------------------------------------------------------------------------------------------------------- CFastFIR
def new_fir(ctx, nchan, max_in):
    f = FastFir(ctx, nchan=nchan, max_in=max_in)
    for ch in range(nchan):
        f.setup(ch, 100.0 + 50 * ch, 2500.0 + 50 * ch, 0.0, 12000.0, do_cic_comp=bool(ch & 1))
    return f


def nout_of(f, chans, n_each):
    return [(f.pos(c) + n) // 512 * 512 for c, n in zip(chans, n_each)]


@pytest.mark.parametrize("each", [False, True])
def test_fir_process(gpu_ctx, each):
    """kg_fir_process_dev (one n) and kg_fir_process_each_dev (n_each with a row of 0 and of 1 sample); a second call on the carried
    history, so that what the first call appended is part of the check"""
    chans = [4, 0, 5, 1, 3] if each else [2, 0, 1]
    n_each = [0, 1, 170, 513, 1024] if each else [700] * 3
    rng = np.random.default_rng(21)
    x = [[c64(rng, n) for n in n_each] for _ in range(2)]
    lst, cnt = np.array(chans, np.int32), np.array(n_each, np.int32)

    def case(lay):
        f = new_fir(gpu_ctx, 6, 1024)
        try:
            res = []
            for call in range(2):
                want = nout_of(f, chans, n_each)
                g_in, s_in = lay.inp(x[call], 8)
                g_out, s_out = lay.out(len(chans), max(want), 8, 8)
                nout = np.zeros(len(chans), np.int32)
                if each:
                    check(gpu_ctx.lib.kg_fir_process_each_dev(f.h, ptr(lst), len(chans), ptr(g_in.ptr), s_in, ptr(cnt), ptr(g_out.ptr), s_out,
                                                              ptr(nout)), "kg_fir_process_each_dev")
                else:
                    nout = f.process_dev(chans, g_in.ptr, s_in, n_each[0], g_out.ptr, s_out)
                gpu_ctx.sync()
                assert nout.tolist() == want
                res.append((lay.take(g_out, [8 * int(k) for k in nout]), nout, [f.pos(c) for c in range(6)]))
            return res
        finally:
            f.close()

    res = contain(gpu_ctx, case)
    assert sum(len(r[2]) for r in res[1][0]) > 0                       # the second call produced output from the carried history


@pytest.mark.parametrize("taps", ["pre", "post", "both"])
def test_fir_process_taps(gpu_ctx, taps):
    chans, n = [2, 0, 1], 1500
    rng = np.random.default_rng(22)
    x = [c64(rng, n) for _ in chans]

    def case(lay):
        f = new_fir(gpu_ctx, 3, n)
        try:
            g_in, s_in = lay.inp(x, 8)
            g_out, s_out = lay.out(3, 1024, 8, 8)
            g_pre, s_tap = lay.out(3, 2048, 8, 8)
            g_post, _ = lay.out(3, 2048, 8, 8)
            nout = np.zeros(3, np.int32)
            lst = np.array(chans, np.int32)
            check(gpu_ctx.lib.kg_fir_process_taps_dev(f.h, ptr(lst), 3, ptr(g_in.ptr), s_in, n, ptr(g_out.ptr), s_out, ptr(nout),
                                                      ptr(g_pre.ptr) if taps != "post" else None, ptr(g_post.ptr) if taps != "pre" else None,
                                                      s_tap), "kg_fir_process_taps_dev")
            gpu_ctx.sync()
            assert nout.tolist() == [1024] * 3
            return (lay.take(g_out, 8 * 1024), lay.take(g_pre, 8 * 2048 if taps != "post" else 0),
                    lay.take(g_post, 8 * 2048 if taps != "pre" else 0), [f.pos(c) for c in range(3)])
        finally:
            f.close()

    contain(gpu_ctx, case)


def test_fir_refilter(gpu_ctx):
    chans, nblk = [2, 0, 1], [0, 1, 2]
    rng = np.random.default_rng(23)
    pre = [c64(rng, 1024 * k) for k in nblk]

    def case(lay):
        f = new_fir(gpu_ctx, 3, 1024)
        try:
            g_pre, s_tap = lay.inp(pre, 8)
            g_out, s_out = lay.out(3, 1024, 8, 8)
            check(gpu_ctx.lib.kg_fir_refilter_dev(f.h, ptr(np.array(chans, np.int32)), 3, ptr(np.array(nblk, np.int32)), ptr(g_pre.ptr), s_tap,
                                                  ptr(g_out.ptr), s_out), "kg_fir_refilter_dev")
            gpu_ctx.sync()
            return lay.take(g_out, [8 * 512 * k for k in nblk])
        finally:
            f.close()

    contain(gpu_ctx, case)


@pytest.mark.parametrize("variant", ["all", "no_out", "no_post"])
def test_fir_process_spec(gpu_ctx, variant):
    chans, n_each, inst = [2, 0, 1], [0, 512, 1100], [0, 1, 0]
    rng = np.random.default_rng(24)
    x = [c64(rng, n) for n in n_each]

    def case(lay):
        f = new_fir(gpu_ctx, 3, 1100)
        try:
            g_in, s_in = lay.inp(x, 8)
            g_out, s_out = lay.out(3, 1024, 8, 8)
            g_rows, s_rows = lay.out(3, 2048, 1, 4, mult=4)                      # d_rows and row_stride: multiples of 4 bytes
            g_post, s_tap = lay.out(3, 2048, 8, 8)
            nout = f.process_spec_dev(chans, g_in.ptr, s_in, n_each, g_out.ptr if variant != "no_out" else None, s_out, g_rows.ptr, s_rows,
                                      inst, g_post.ptr if variant != "no_post" else None, s_tap if variant != "no_post" else 0)
            gpu_ctx.sync()
            assert nout.tolist() == [0, 512, 1024]
            return (lay.take(g_out, [8 * int(k) if variant != "no_out" else 0 for k in nout]), lay.take(g_rows, [2 * int(k) for k in nout]),
                    lay.take(g_post, [16 * int(k) if variant != "no_post" else 0 for k in nout]), [f.pos(c) for c in range(3)])
        finally:
            f.close()

    contain(gpu_ctx, case)


@pytest.mark.parametrize("nrows", [1, 3])
def test_snd_spec_rows(gpu_ctx, nrows):
    rng = np.random.default_rng(25)
    spec = [c64(rng, 1024, 3.0e4) for _ in range(nrows)]
    inst = [1, 0, 1][:nrows]

    def case(lay):
        g_in, s_in = lay.inp(spec, 8)
        g_rows, s_rows = lay.out(nrows, 1024, 1, 4, mult=4)
        snd.spec_rows_dev(gpu_ctx, g_in.ptr, s_in, inst, g_rows.ptr, s_rows)
        gpu_ctx.sync()
        return lay.take(g_rows, 1024)

    rows = contain(gpu_ctx, case)
    tight = snd.spec_rows(gpu_ctx, np.stack(spec), inst)
    for r in range(nrows):
        assert rows[r][2] == tight[r].tobytes()


def test_fir_refuses_misaligned_buffers(gpu_ctx):
    """every CFastFIR buffer is read and written as complex floats: 8-byte pointers, refused on the host otherwise (nothing launched)"""
    f = new_fir(gpu_ctx, 1, 512)
    d = gpu_ctx.alloc(1 << 16)
    try:
        lst, cnt, nout = np.zeros(1, np.int32), np.full(1, 512, np.int32), np.zeros(1, np.int32)
        L = gpu_ctx.lib
        said = lambda: L.kg_last_error().decode()                      # the refusal names the entry point and the pointer
        for d_in, d_out, which in ((d + 4, d + 8192, "d_in"), (d, d + 8192 + 4, "d_out")):
            assert L.kg_fir_process_dev(f.h, ptr(lst), 1, ptr(d_in), 512, 512, ptr(d_out), 512, ptr(nout)) == KG_ERR_INVALID
            assert said().startswith("kg_fir_process_dev: " + which + " "), said()
            assert L.kg_fir_process_each_dev(f.h, ptr(lst), 1, ptr(d_in), 512, ptr(cnt), ptr(d_out), 512, ptr(nout)) == KG_ERR_INVALID
            assert said().startswith("kg_fir_process_each_dev: " + which + " "), said()
            assert L.kg_fir_refilter_dev(f.h, ptr(lst), 1, ptr(np.ones(1, np.int32)), ptr(d_in), 1024, ptr(d_out), 512) == KG_ERR_INVALID
        assert L.kg_fir_process_taps_dev(f.h, ptr(lst), 1, ptr(d), 512, 512, ptr(d + 8192), 512, ptr(nout), ptr(d + 16384 + 4), None,
                                         1024) == KG_ERR_INVALID
        assert said().startswith("kg_fir_process_taps_dev: d_pre "), said()
        assert L.kg_fir_process_taps_dev(f.h, ptr(lst), 1, ptr(d), 512, 512, ptr(d + 8192), 512, ptr(nout), None, ptr(d + 16384 + 4),
                                         1024) == KG_ERR_INVALID
        assert said().startswith("kg_fir_process_taps_dev: d_post "), said()
        inst = np.zeros(1, np.int32)
        assert L.kg_fir_process_spec_dev(f.h, ptr(lst), 1, ptr(d + 4), 512, ptr(cnt), ptr(d + 8192), 512, ptr(nout), ptr(d + 32768), 1024,
                                         ptr(inst), None, 0) == KG_ERR_INVALID
        assert said().startswith("kg_fir_process_spec_dev: d_in "), said()
        assert f.pos(0) == 0                                           # a refused call leaves the object where it was
    finally:
        gpu_ctx.free(d)
        f.close()


# ---------------------------------------------------------------------------------------------------------- NB_STD, audio side
def nb_input(rng, n):
    x = c64(rng, n, 100.0)
    x[7::40] *= 60.0                                                   # pulses for the blanker to find
    return x


def test_nb_process(gpu_ctx):
    """out of place and in place (d_in == d_out, which the header allows): the same result, and two calls so that the rings carry"""
    chans, n_each = [3, 0, 4, 1], [0, 1, 65, 511]
    rng = np.random.default_rng(31)
    x = [[nb_input(rng, n) for n in n_each] for _ in range(2)]

    def make(in_place):
        def case(lay):
            nb = NoiseBlanker(gpu_ctx, nchan=5, max_in=1024)
            try:
                for ch in range(5):
                    nb.setup(ch, 12000.0, [100.0 + 20 * ch, 50.0])
                res = []
                for call in range(2):
                    g_in, s_in = lay.inp(x[call], 8, inplace=in_place)
                    g_out, s_out = (g_in, s_in) if in_place else lay.out(4, 511, 8, 8)
                    nb.process_dev(chans, g_in.ptr, s_in, n_each, g_out.ptr, s_out)
                    gpu_ctx.sync()
                    res.append(lay.take(g_out, [8 * n for n in n_each]))
                return res, nb.state(list(range(5)))
            finally:
                nb.close()
        return case

    assert contain(gpu_ctx, make(False)) == contain(gpu_ctx, make(True))


# ------------------------------------------------------------------------------------------------------------- the libm arrays
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_math(gpu_ctx, oracle, n):
    rng = np.random.default_rng(n)
    x = [np.abs(rng.standard_normal(n)).astype(np.float32) * np.float32(1e3)]
    y = [rng.standard_normal(n).astype(np.float32)]
    L = gpu_ctx.lib

    def case(lay):
        g_x, _ = lay.inp(x, 4)
        g_y, _ = lay.inp(y, 4)
        g_log, _ = lay.out(1, n, 4, 4)
        g_bits, _ = lay.out(1, n, 4, 4)
        g_at, _ = lay.out(1, n, 4, 4)
        check(L.kg_math_dev(gpu_ctx.h, 0, 10.0, ptr(g_x.ptr), 0, n, ptr(g_log.ptr)), "kg_math_dev")
        check(L.kg_math_dev(gpu_ctx.h, 2, 10.0, None, 0x3F800000, n, ptr(g_bits.ptr)), "kg_math_dev")       # expf of the floats from 1.0 on
        check(L.kg_math_atan2f_dev(gpu_ctx.h, ptr(g_y.ptr), ptr(g_x.ptr), n, ptr(g_at.ptr)), "kg_math_atan2f_dev")
        gpu_ctx.sync()
        return lay.take(g_log, 4 * n), lay.take(g_bits, 4 * n), lay.take(g_at, 4 * n)

    log, bits, _ = contain(gpu_ctx, case)
    assert log[0][2] == np.asarray(oracle.libm_log10f(x[0]), np.float32).tobytes()
    assert bits[0][2] == np.asarray(oracle.libm_expf_bits(0x3F800000, n), np.float32).tobytes()
