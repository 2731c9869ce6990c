"""The audio spectrum rows on the device (specAF_FFT, rx/rx_sound.cpp:175-220): kg_snd_spec_rows_dev against every byte of the
reference's rows (tests/golden/spec_ref.npz, Pin 1), and kg_fir_process_spec_dev -- the rows formed inside the CFastFIR block kernel
from the registers that hold the filtered spectrum -- against the host model (csrc/kg_spec.h through tools/spec_host_driver.cpp)
applied to the spectrum the same call stored, with its outputs, positions and history bit-equal to kg_fir_process_each_dev on a twin
object.  No byte is compared across different transforms: power is re * re alone, so bytes are ill-conditioned wherever re ~ 0."""
import ctypes as C

import numpy as np
import pytest

from flydog_sdr_gps_amd import snd
from flydog_sdr_gps_amd._lib import check, ptr

from . import spec_common as sc

pytestmark = pytest.mark.gpu
PAD = 64


@pytest.fixture(scope="module")
def golden():
    return sc.load()


@pytest.fixture(scope="module")
def pool():
    return sc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sc.build_driver(tmp_path_factory.mktemp("spec"))


def _rows_dev(ctx, spec, inst, row_stride):
    """-> the whole row buffer uint8 [nrows, row_stride], pre-filled with 0xAA"""
    out = np.full((spec.shape[0], row_stride), 0xAA, np.uint8)
    d_spec, d_rows = ctx.alloc(spec.nbytes), ctx.alloc(out.nbytes)
    try:
        ctx.upload(d_spec, spec)
        ctx.upload(d_rows, out)
        snd.spec_rows_dev(ctx, d_spec, 1024, inst, d_rows, row_stride)
        ctx.sync()
        ctx.download(d_rows, out)
    finally:
        ctx.free(d_spec)
        ctx.free(d_rows)
    return out


def test_rows_equal_the_reference_on_every_byte(gpu_ctx, golden, pool):
    names, spec = pool
    want = golden["rows"]
    # 67 rows (not a multiple of the four waves of a workgroup), a padded row stride, every pool spectrum at both scales
    src = np.arange(67) % len(names)
    inst = ((np.arange(67) // len(names)) & 1).astype(np.int32)
    got = _rows_dev(gpu_ctx, np.ascontiguousarray(spec[src]), inst, 1024 + PAD)
    seen = set()
    for r in range(67):
        bad = np.flatnonzero(got[r, :1024] != want[src[r], inst[r]])
        assert bad.size == 0, (names[src[r]], int(inst[r]), "first differing byte", int(bad[0]), int(got[r, bad[0]]), int(want[src[r], inst[r], bad[0]]))
        seen.add((int(src[r]), int(inst[r])))
    assert len(seen) == 2 * len(names)
    assert (got[:, 1024:] == 0xAA).all(), "the padding between rows was written"
    # one row, each instance
    for i in (sc.PASSBAND, sc.CHAN_NULL):
        k = names.index("inf_overflow_zero_re")
        one = _rows_dev(gpu_ctx, spec[k:k + 1], np.array([i], np.int32), 1024)
        assert np.array_equal(one[0], want[k, i]), i


def _each_dev(F, chans, d_in, in_stride, n_each, d_out, out_stride):
    chans, n_each = np.ascontiguousarray(chans, np.int32), np.ascontiguousarray(n_each, np.int32)
    nout = np.zeros(chans.size, np.int32)
    check(F.lib.kg_fir_process_each_dev(F.h, ptr(chans), chans.size, ptr(int(d_in)), int(in_stride), ptr(n_each), ptr(int(d_out)),
                                        int(out_stride), ptr(nout)), "kg_fir_process_each_dev")
    return nout


def test_fused_rows_in_the_fir_block(gpu_ctx, driver, tmp_path):
    ctx = gpu_ctx
    NCH, CALLS, MAXBLK = 3, 8, 4
    n_each = np.array([170, 1621, 0], np.int32)
    inst = np.array([sc.PASSBAND, sc.CHAN_NULL, sc.PASSBAND], np.int32)
    chans = np.arange(NCH, dtype=np.int32)
    in_stride, out_stride, tap_stride, row_stride = 1621, MAXBLK * 512, MAXBLK * 1024, MAXBLK * 1024 + PAD
    # A: rows + d_out + d_post; B: kg_fir_process_each_dev (the twin); R: rows only; Z: no d_out for the first half, then with one
    firs = {k: snd.FastFir(ctx, nchan=NCH, max_in=2048) for k in "ABRZ"}
    bufs = {}
    try:
        for F in firs.values():
            F.setup(0, 300.0, 2700.0, 0.0, 12000.0)
            F.setup(1, -4900.0, 4900.0, 0.0, 12000.0)
            F.setup(2, -2700.0, -300.0, 0.0, 12000.0)
        rng = np.random.default_rng(0x5BEC)
        d_in = ctx.alloc(NCH * in_stride * 8)
        for k in "ABRZ":
            bufs[k] = {"out": ctx.alloc(NCH * out_stride * 8), "rows": ctx.alloc(NCH * row_stride), "post": ctx.alloc(NCH * tap_stride * 8)}
        rows_total = 0
        for call in range(CALLS):
            x = (rng.standard_normal((NCH, in_stride)) + 1j * rng.standard_normal((NCH, in_stride))).astype(np.complex64) * np.float32(3000.0)
            ctx.upload(d_in, x)
            fill = np.full((NCH, row_stride), 0xAA, np.uint8)
            for k in "ARZ":
                ctx.upload(bufs[k]["rows"], fill)
            z_out = call >= CALLS // 2
            nA = firs["A"].process_spec_dev(chans, d_in, in_stride, n_each, bufs["A"]["out"], out_stride, bufs["A"]["rows"], row_stride, inst,
                                            bufs["A"]["post"], tap_stride)
            nB = _each_dev(firs["B"], chans, d_in, in_stride, n_each, bufs["B"]["out"], out_stride)
            nR = firs["R"].process_spec_dev(chans, d_in, in_stride, n_each, bufs["R"]["out"], out_stride, bufs["R"]["rows"], row_stride, inst)
            nZ = firs["Z"].process_spec_dev(chans, d_in, in_stride, n_each, bufs["Z"]["out"] if z_out else None, out_stride,
                                            bufs["Z"]["rows"], row_stride, inst)
            ctx.sync()
            assert np.array_equal(nA, nB) and np.array_equal(nR, nB) and np.array_equal(nZ, nB), (call, nA, nB, nR, nZ)
            assert nB[2] == 0
            for ch in range(NCH):
                assert firs["A"].pos(ch) == firs["B"].pos(ch) == firs["R"].pos(ch) == firs["Z"].pos(ch), (call, ch)
            got = {}
            for k in "ABRZ":
                o = np.zeros((NCH, out_stride), np.complex64)
                ctx.download(bufs[k]["out"], o)
                got[k] = o
            rows = {}
            for k in "ARZ":
                r = np.zeros((NCH, row_stride), np.uint8)
                ctx.download(bufs[k]["rows"], r)
                rows[k] = r
            post = np.zeros((NCH, tap_stride), np.complex64)
            ctx.download(bufs["A"]["post"], post)
            for ch in range(NCH):
                n = int(nB[ch])
                for k in "AR" + ("Z" if z_out else ""):                 # existing behaviour unchanged: bit-equal outputs
                    assert np.array_equal(got[k][ch, :n].view(np.uint32), got["B"][ch, :n].view(np.uint32)), (call, ch, k)
                nb = n // 512
                if nb:
                    want = sc.host_rows(driver, post[ch, :nb * 1024].reshape(nb, 1024), tmp_path)[:, inst[ch]]
                    for k in "ARZ":
                        have = rows[k][ch, :nb * 1024].reshape(nb, 1024)
                        bad = np.argwhere(have != want)
                        assert bad.size == 0, (call, ch, k, "first differing byte", bad[0], int(have[tuple(bad[0])]), int(want[tuple(bad[0])]))
                    assert want.min() >= 55 and len(np.unique(want)) > 20   # a real spectrum, not a constant row
                    rows_total += nb
                for k in "ARZ":
                    assert (rows[k][ch, nb * 1024:] == 0xAA).all(), (call, ch, k, "wrote past the completed blocks")
        assert rows_total >= 2 + 25                                      # ch 0: 170 * 8 / 512, ch 1: 1621 * 8 / 512
        ctx.free(d_in)
    finally:
        for b in bufs.values():
            for d in b.values():
                ctx.free(d)
        for F in firs.values():
            F.close()


def test_process_spec_host_arrays(gpu_ctx, driver, tmp_path):
    """FastFir.process_spec: the OutBuf == NULL call gives the same rows and the same position"""
    F, G = snd.FastFir(gpu_ctx, nchan=1, max_in=2048), snd.FastFir(gpu_ctx, nchan=1, max_in=2048)
    try:
        for o in (F, G):
            o.setup(0, -4000.0, 4000.0, 0.0, 12000.0)
        rng = np.random.default_rng(7)
        x = ((rng.standard_normal(1300) + 1j * rng.standard_normal(1300)) * 900).astype(np.complex64)
        out, rows, post = F.process_spec(0, x, sc.CHAN_NULL, want_post=True)
        none, rows2, _ = G.process_spec(0, x, sc.CHAN_NULL, want_out=False)
        assert none is None and out.size == 1024 and rows.shape == (2, 1024) and np.array_equal(rows, rows2) and F.pos(0) == G.pos(0) == 1300 - 1024
        assert np.array_equal(rows, sc.host_rows(driver, post, tmp_path)[:, sc.CHAN_NULL])
    finally:
        F.close()
        G.close()
