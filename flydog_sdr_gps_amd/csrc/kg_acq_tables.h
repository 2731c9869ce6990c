// kg_acq_tables.h -- host-built constant tables of the acquisition kernels (plain C++: no HIP types, so that a
// stand-alone host program can call the same builders, tests/test_acq_horner_cpu.py).
#pragma once

#include <math.h>

// exp(+2 pi i k / n) in double, rounded to fp32, exact on the axes (as kg_ctx's tables).
static inline void kg_unit_root_f(long k, long n, float *re, float *im)
{
    k %= n;
    if (k < 0) k += n;
    if (k == 0) { *re = 1.f; *im = 0.f; return; }
    if (4 * k == n) { *re = 0.f; *im = 1.f; return; }
    if (2 * k == n) { *re = -1.f; *im = 0.f; return; }
    if (4 * k == 3 * n) { *re = 0.f; *im = -1.f; return; }
    const double a = 2.0 * M_PI * (double) k / (double) n;
    *re = (float) cos(a); *im = (float) sin(a);
}

// Row constants of the C/A correlator's last pass (acq_correlate_kernel, kg_radix16_stage2f_k): thread t owns the outputs
// n = t + 256 (c + 4 d) of an N = 4096 P point cell, and the wave-uniform part W_R^{c k2}, R = N / 256, of the combine
// twiddle W_N^{n k2} rides on the internal twiddles of row c of the second radix-4 stage:
//     out[(12 k2 + 4 (c - 1) + d)] = W_16^{c d} W_R^{c k2} = W_R^{c (d R / 16 + k2)},   c = 1..3, d = 0..3
// -- each ONE root of unity, rounded once (row 0 has no twiddles and is not stored).  out: P * 12 (re, im) pairs.
#define KG_ACQ_ROWK 12
static inline void kg_acq_row_consts(int P, float *out)
{
    const long R = 16L * P;                    // N / 256
    for (int k2 = 0; k2 < P; k2++)
        for (int c = 1; c < 4; c++)
            for (int d = 0; d < 4; d++) {
                float *o = out + 2 * (KG_ACQ_ROWK * k2 + 4 * (c - 1) + d);
                kg_unit_root_f((long) c * (d * (R / 16) + k2), R, &o[0], &o[1]);
            }
}

// The Horner chain of the C/A correlator (acq_correlate_kernel) gives term k2 the factor V^k2 with V = fl(W), W = W_N^{t + 1024 d}:
// the one rounding of V, W (1 + e), comes out as W^k2 (1 + k2 e) -- 15 e at the far end of the P = 16 chain, a relative error
// near 1e-6 in a peak's power where the lines of a spectrum sit in the planes k2 = 10 .. 15 (tests/test_dft_truth_gpu.py).  So
// the P = 16 chain is RESTARTED once: the step that takes in term KG_ACQ_MID - 1 multiplies by M = W^MID / V^(MID - 1) instead
// of by V, and what the terms MID .. 15 have gathered reaches the end as W^MID (1 + e_M): no term carries more than 7 e + e_M.
// out: [4][256] (re, im) pairs, entry 256 d + t; V as kg_unit_root_f rounds it, the quotient in double.
#define KG_ACQ_MID 8
static inline void kg_acq_mid_factors(long N, float *out)
{
    for (int d = 0; d < 4; d++)
        for (int t = 0; t < 256; t++) {
            const long n = t + 1024L * d;
            float vr, vi;
            kg_unit_root_f(n, N, &vr, &vi);
            double pr = 1.0, pi = 0.0;                 // V^(MID - 1)
            for (int i = 0; i < KG_ACQ_MID - 1; i++) {
                const double r = pr * vr - pi * vi, m = pr * vi + pi * vr;
                pr = r; pi = m;
            }
            const double a = 2.0 * M_PI * (double) ((KG_ACQ_MID * n) % N) / (double) N;
            const double wr = cos(a), wi = sin(a), q = pr * pr + pi * pi;
            out[2 * (256 * d + t)] = (float) ((wr * pr + wi * pi) / q);          // W^MID conj(V^7) / |V^7|^2
            out[2 * (256 * d + t) + 1] = (float) ((wi * pr - wr * pi) / q);
        }
}
