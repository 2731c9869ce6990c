"""The device's sinf, cosf and atan2f (csrc/kg_libm_trig.h: the GNU C Library 2.35 algorithms restated) against the image's libm -- what the
synchronous-AM PLL of rx/wdsp/SAM_demod.cpp calls on every sample and feeds back into itself -- through the C ABI (kg_math_dev,
kg_math_atan2f_dev): BIT-EXACT, NaNs as NaNs.  sinf / cosf: every float of [-2 pi, 2 pi] (the PLL's phase is in [0, 2 pi)), strided
patterns over the whole range, the special values; atan2f: 2^24 random pairs of bit patterns, 2^24 pairs from the correlator's range,
and every pairing of signed zeros, infinities, NaN, subnormals and the branch edges of e_atan2f.c / s_atanf.c.

The truth is libm.so.6 itself: a small C loop over its sinf / cosf / atan2f is compiled here and loaded through ctypes (numpy's own
functions are not glibc's).  tools/check_sam_libm.cpp runs the same restatements exhaustively on a CPU (profiles/sam_libm_exhaustive.txt)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import post

pytestmark = pytest.mark.gpu

TRUTH_C = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
void libm_sincos_bits(int fn, uint32_t first, uint64_t n, float *out)
{
    for (uint64_t i = 0; i < n; i++) {
        uint32_t u = first + (uint32_t) i;
        float x;
        memcpy(&x, &u, 4);
        out[i] = fn ? cosf(x) : sinf(x);
    }
}
void libm_sincos_arr(int fn, const float *x, uint64_t n, float *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = fn ? cosf(x[i]) : sinf(x[i]);
}
void libm_atan2f(const float *y, const float *x, uint64_t n, float *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = atan2f(y[i], x[i]);
}
"""


@pytest.fixture(scope="module")
def libm(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed to call libm.so.6's own functions over arrays"
    d = tmp_path_factory.mktemp("libm_truth")
    src, so = os.path.join(d, "t.c"), os.path.join(d, "libt.so")
    open(src, "w").write(TRUTH_C)
    subprocess.run([cc, "-O1", "-fno-builtin", "-shared", "-fPIC", src, "-o", so, "-lm"], check=True)
    lib = C.CDLL(so)
    lib.libm_sincos_bits.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.libm_sincos_arr.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.libm_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def truth_bits(lib, fn, first, n):
    out = np.empty(n, np.float32)
    lib.libm_sincos_bits(fn, first, n, out.ctypes.data)
    return out


def truth_atan2(lib, y, x):
    y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
    out = np.empty(y.size, np.float32)
    lib.libm_atan2f(y.ctypes.data, x.ctypes.data, y.size, out.ctypes.data)
    return out


TWO_PI_BITS = int(np.float32(2 * np.pi).view(np.uint32))            # the float nearest 2 pi (just above it)


@pytest.mark.parametrize("fn,name", [(post.MATH_SINF, "sinf"), (post.MATH_COSF, "cosf")])
def test_every_float_of_minus_two_pi_to_two_pi(gpu_ctx, libm, fn, name):
    CH = 1 << 26
    total = 0
    for sign in (0, 0x80000000):
        end = TWO_PI_BITS + 1
        for lo in range(0, end, CH):
            n = min(CH, end - lo)
            got = post.math_dev(gpu_ctx, fn, first_bits=sign + lo, n=n)
            want = truth_bits(libm, fn - post.MATH_SINF, sign + lo, n)
            bad = np.flatnonzero(~same(got, want))
            assert bad.size == 0, (name, [hex(sign + lo + int(b)) for b in bad[:4]], got[bad[:4]], want[bad[:4]])
            total += n
    assert total == 2 * (TWO_PI_BITS + 1)


@pytest.mark.parametrize("fn,name", [(post.MATH_SINF, "sinf"), (post.MATH_COSF, "cosf")])
def test_strided_whole_range_and_specials(gpu_ctx, libm, fn, name):
    bits = np.concatenate([np.arange(0, 1 << 32, 509, dtype=np.uint64).astype(np.uint32),          # 8.4 M patterns: reduce_large, NaNs
                           np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 1, 0x80000001, 0x007fffff,
                                     0x39800000, 0x3f490fdb, 0x42f00000, 0x42f00001, 0x7f7fffff, 0xff7fffff], np.uint32)])
    x = bits.view(np.float32)
    got = post.math_dev(gpu_ctx, fn, x=x)
    want = np.empty_like(x)
    libm.libm_sincos_arr(fn - post.MATH_SINF, x.ctypes.data, x.size, want.ctypes.data)
    bad = np.flatnonzero(~same(got, want))
    assert bad.size == 0, (name, [hex(int(b)) for b in bits[bad[:6]]], got[bad[:6]], want[bad[:6]])
    assert np.isnan(got[-13]) and np.isnan(got[-12]) and np.isnan(got[-11])          # Inf, -Inf, NaN


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38,
                    3.4028235e38, -3.4028235e38, 2.0 ** 60, 2.0 ** 61, 2.0 ** -60, 2.0 ** -61, 2.0 ** 25, 2.0 ** 26, 2.0 ** -29,
                    0.4375, 0.6875, 1.1875, 2.4375, -0.4375, 3.0, 1e-38, 5e-39, 0.5, 1.5, 2.0, -2.0, 1e30, -1e30, 1e-30, 100.0,
                    -100.0, 3.14159274, -3.14159274], np.float32)


def test_atan2f_random_pairs_correlator_range_and_specials(gpu_ctx, libm):
    rng = np.random.default_rng(0x5A3)
    n = 1 << 24
    cases = [rng.integers(0, 1 << 32, (2, n), dtype=np.uint64).astype(np.uint32).view(np.float32),                  # any bit patterns
             (rng.integers(-(1 << 20), 1 << 20, (2, n)) * np.float32(0.5)).astype(np.float32),                       # the correlator's
             np.stack(np.meshgrid(SPECIAL, SPECIAL)).reshape(2, -1).astype(np.float32),                              # the branch edges
             np.array([[0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39], [-0.0, -0.0, 0.0, 0.0, 3e-39, -3e-39, 1e-45, 1e-45]],
                      np.float32)]                                                                                   # signed zeros, subnormals
    for y, x in cases:
        got = post.math_atan2f_dev(gpu_ctx, y, x)
        want = truth_atan2(libm, y, x)
        bad = np.flatnonzero(~same(got, want))
        assert bad.size == 0, (y[bad[:4]], x[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert post.math_atan2f_dev(gpu_ctx, np.float32([-0.0]), np.float32([-1.0]))[0] == np.float32(-np.pi)
