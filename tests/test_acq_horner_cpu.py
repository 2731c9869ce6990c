"""The C/A correlator's combine as a Horner chain with the row part of the twiddle folded into pass 2
(kg_acq.hip, kg_radix16_stage2f_k / kg_horner4v in kg_fft.h): the algebra in float64, and the host-built
constant table against numpy.

Thread t owns the outputs n = t + 256 (c + 4 d) of an N = 4096 P point cell.  With R = N / 256:
    W_N^{n k2} = (W_N^t W_{R/4}^d)^{k2} W_R^{c k2} = V[d]^{k2} W_R^{c k2},      V[d] = W_N^{t + 1024 d}
The row part rides on the internal twiddles of row c of the last radix-16's second stage (table entry
12 k2 + 4 (c - 1) + d' = W16^{c d'} W_R^{c k2}), the rest is Horner from k2 = P - 1 down."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def root(k, n):
    return np.exp(2j * np.pi * (np.asarray(k) % n) / n)


def row_consts(P):
    """kg_acq_row_consts in float64: [P][12] complex."""
    R = 16 * P
    out = np.zeros((P, 12), np.complex128)
    for k2 in range(P):
        for c in range(1, 4):
            for d in range(4):
                out[k2, 4 * (c - 1) + d] = root(c * (d * (R // 16) + k2), R)
    return out


def stage2_plain(x):
    """kg_radix16_stage2f (SIGN = +1): x[..., 4c + d'] -> y[..., c + 4d] = sum_d' W16^{c d'} x[4c + d'] j^{d' d}."""
    y = np.zeros_like(x)
    for c in range(4):
        for d in range(4):
            y[..., c + 4 * d] = sum(root(c * dp, 16) * x[..., 4 * c + dp] * 1j ** (dp * d) for dp in range(4))
    return y


def stage2_rowk(x, k):
    """kg_radix16_stage2f_k: the same blocks the kernel forms -- products, fused sums, differences as 2 u - s."""
    y = np.zeros_like(x)
    s02, s13 = x[..., 0] + x[..., 2], x[..., 1] + x[..., 3]                 # row 0: no twiddles
    d02, d13 = x[..., 0] - x[..., 2], x[..., 1] - x[..., 3]
    y[..., 0], y[..., 8], y[..., 4], y[..., 12] = s02 + s13, s02 - s13, d02 + 1j * d13, d02 - 1j * d13
    for c in range(1, 4):
        z = [x[..., 4 * c + dp] for dp in range(4)]
        kk = k[4 * (c - 1):4 * c]
        u0, u1 = kk[0] * z[0], kk[1] * z[1]
        s02, s13 = u0 + kk[2] * z[2], u1 + kk[3] * z[3]
        d02, d13 = 2 * u0 - s02, 2 * u1 - s13
        y[..., c], y[..., c + 8] = s02 + s13, s02 - s13
        y[..., c + 4], y[..., c + 12] = d02 + 1j * d13, d02 - 1j * d13
    return y


@pytest.mark.parametrize("P", [4, 16])
def test_folded_rows_plus_horner_equal_the_twiddled_sum(P):
    N = 4096 * P
    rng = np.random.default_rng(1000 + P)
    # the inputs of every thread's last second stage, per item: [k2][t][16]
    x = rng.standard_normal((P, 256, 16)) + 1j * rng.standard_normal((P, 256, 16))
    t = np.arange(256)
    m = np.arange(16)
    n = t[:, None] + 256 * m[None, :]                          # [t][m]: every n < 4096
    assert np.array_equal(np.sort(n.ravel()), np.arange(4096))
    Z = stage2_plain(x)                                        # Z_k2[n] as today's pass 2 delivers it
    want = sum(root(n * k2, N) * Z[k2] for k2 in range(P))
    K = row_consts(P)
    V = np.stack([root(t + 1024 * d, N) for d in range(4)], axis=1)      # [t][d]
    Vm = V[:, m >> 2]                                          # the factor of output m = c + 4 d
    acc = stage2_rowk(x[P - 1], K[P - 1])                      # the first item is the copy
    for k2 in range(P - 2, -1, -1):
        acc = acc * Vm + stage2_rowk(x[k2], K[k2])
    scale = np.abs(want).max()
    assert np.abs(acc - want).max() <= 1e-12 * scale
    # k2 = 0: the folded stage is today's stage
    assert np.abs(stage2_rowk(x[0], K[0]) - Z[0]).max() <= 1e-12 * np.abs(Z[0]).max()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host driver"
    exe = str(tmp_path_factory.mktemp("acqtab") / "acq_tables_host_driver")
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tools", "acq_tables_host_driver.cpp")], check=True)
    return exe


@pytest.mark.parametrize("P", [4, 16])
def test_host_built_row_constants(driver, tmp_path, P):
    out = str(tmp_path / "tab.bin")
    subprocess.run([driver, str(P), out], check=True)
    got = np.fromfile(out, np.float32).reshape(P, 12, 2)
    want = row_consts(P)
    w32 = np.stack([want.real.astype(np.float32), want.imag.astype(np.float32)], axis=-1)
    # double values rounded to fp32; the builder is exact on the axes where cos / sin in double leave 6e-17
    axis = (np.abs(want.real) < 1e-15) | (np.abs(want.imag) < 1e-15)
    w32[axis] = (np.round(np.stack([want.real, want.imag], axis=-1)[axis]) + 0.0).astype(np.float32)     # (+ 0.0: no -0)
    assert np.array_equal(got.view(np.uint32), w32.view(np.uint32))
    assert np.all(got[0, [0, 4, 8]] == np.float32([1, 0]))     # k2 = 0: z0 of every row keeps its value exactly


def test_restart_factors_halve_the_drift_of_the_65536_chain(driver, tmp_path):
    """Term k2 of the chain carries V^k2 with V = fl(W): one rounding of V comes out k2 times.  kg_acq_mid_factors gives the step
    that takes in term 7 the factor M = W^8 / V^7, so terms 8 .. 15 carry V^(k2 - 8) M V^7 = W^8 V^(k2 - 8) (1 + e_M): the
    table against numpy, and the factor of every term of every lane against W^k2 in float64 (the drift alone, without the
    roundings of the chain's own arithmetic)."""
    out = str(tmp_path / "mid.bin")
    subprocess.run([driver, "mid", out], check=True)
    got = np.fromfile(out, np.float32).reshape(4, 256, 2)
    M = got[..., 0].astype(np.float64) + 1j * got[..., 1]
    n = np.arange(256)[None, :] + 1024 * np.arange(4)[:, None]
    W = root(n, 65536)
    V = W.real.astype(np.float32).astype(np.float64) + 1j * W.imag.astype(np.float32).astype(np.float64)
    want = root(8 * n, 65536) / V ** 7
    assert np.abs(M - want).max() <= 2.0 ** -23                  # the double quotient, rounded to fp32 per component
    assert got[0, 0, 0] == 1 and got[0, 0, 1] == 0               # lag 0: every factor is exactly one
    plain = max(np.abs(V ** k / W ** k - 1).max() for k in range(16))
    restarted = max(np.abs((V ** k if k < 8 else V ** (k - 8) * M * V ** 7) / W ** k - 1).max() for k in range(16))
    u = 2.0 ** -24
    assert restarted <= 8.5 * u                                  # 7 roundings of V and one of M, each at most u in modulus... sqrt(2) u / sqrt(2)
    assert plain >= 1.8 * restarted, (plain, restarted)
