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
