// kg_libm_trig.h -- sinf, cosf and atan2f as the reference's host computes them, on the device AND the host, bit for bit.
// The method, and why, are kg_libm.h's; these three live apart because tests/test_ref_pins_cpu.py pins kg_libm.h's constants against
// the oracle's copy of log10f / powf / expf as text.
#ifndef KG_LIBM_TRIG_H
#define KG_LIBM_TRIG_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kg_libm {
// ---- s_sinf.c / s_cosf.c / e_atan2f.c (glibc 2.35), host AND device ---------------------------------------------------------
// The synchronous-AM PLL (rx/wdsp/SAM_demod.cpp) feeds sinf / cosf of its phase error and atan2f of its correlator back into itself
// on every sample: a one-ulp difference moves the whole trajectory.  Restated from the published algorithms, like the functions above,
// and written for host C++ too, so that tools/check_sam_libm.cpp runs them on a CPU against the image's libm.
//   sinf / cosf: Szabolcs Nagy's method (sincosf.h, sincosf_data.c of ARM's optimized routines): |x| < pi/4 a polynomial in double;
//   |x| < 120 reduce_fast (x - n pi/2 with n from x 2/pi 2^24 truncated: the PLL's phase, [0, 2 pi), is always here); beyond, reduce_large
//   (the 4/pi bits of __inv_pio4, 3 integer products); Inf / NaN give NaN.  glibc's x86_64 multiarch selects s_sinf-fma / s_cosf-fma on an
//   FMA-capable host: the same C compiled with -mfma, so every a + b * c of the polynomials and of reduce_fast is ONE fused operation --
//   that is what kg_fma does here.  Pinned: ALL floats with |x| <= 120, and the whole float range, equal the image's sinf / cosf
//   bit for bit (tools/check_sam_libm.cpp; NaN results compare as NaN: the device's NaN is the positive quiet one, x86's the negative).
//   atan2f: fdlibm's __ieee754_atan2f over __atanf (float arithmetic, 11-term odd/even polynomial).  x86_64 has no multiarch build of
//   either in 2.35 (the baseline build has no FMA instructions to contract into): plain float operations.
#define KG_HD __host__ __device__ __forceinline__
KG_HD uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
KG_HD float u2f(uint32_t x) { return __builtin_bit_cast(float, x); }
KG_HD double kg_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

struct sincosf_t { double sign[4], hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3; };
KG_HD const sincosf_t &sincosf_tab(int k)
{
    static constexpr sincosf_t t[2] = {
        {{1.0, -1.0, -1.0, 1.0}, 0x1.45F306DC9C883p+23, 0x1.921FB54442D18p0, 0x1p0, -0x1.ffffffd0c621cp-2, 0x1.55553e1068f19p-5,
         -0x1.6c087e89a359dp-10, 0x1.99343027bf8c3p-16, -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13},
        {{1.0, -1.0, -1.0, 1.0}, 0x1.45F306DC9C883p+23, 0x1.921FB54442D18p0, -0x1p0, 0x1.ffffffd0c621cp-2, -0x1.55553e1068f19p-5,
         0x1.6c087e89a359dp-10, -0x1.99343027bf8c3p-16, -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13}};
    return t[k];
}
KG_HD uint32_t inv_pio4(int i)          // 4/pi in overlapping 32-bit windows, 8 bits apart
{
    static constexpr uint32_t t[24] = {
        0xa2u,       0xa2f9u,     0xa2f983u,   0xa2f9836eu, 0xf9836e4eu, 0x836e4e44u, 0x6e4e4415u, 0x4e441529u,
        0x441529fcu, 0x1529fc27u, 0x29fc2757u, 0xfc2757d1u, 0x2757d1f5u, 0x57d1f534u, 0xd1f534ddu, 0xf534ddc0u,
        0x34ddc0dbu, 0xddc0db62u, 0xc0db6295u, 0xdb629599u, 0x6295993cu, 0x95993c43u, 0x993c4390u, 0x3c439041u};
    return t[i];
}
KG_HD uint32_t abstop12(float x) { return (f2u(x) >> 20) & 0x7ffu; }

KG_HD float sinf_poly(double x, double x2, const sincosf_t &p, int n)
{
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double s1 = kg_fma(x2, p.s3, p.s2);
        const double x7 = x3 * x2;
        const double s = kg_fma(x3, p.s1, x);
        return (float) kg_fma(x7, s1, s);
    }
    const double x4 = x2 * x2;
    const double c2 = kg_fma(x2, p.c4, p.c3);
    const double c1 = kg_fma(x2, p.c1, p.c0);
    const double x6 = x4 * x2;
    const double c = kg_fma(x4, p.c2, c1);
    return (float) kg_fma(x6, c2, c);
}

KG_HD double reduce_fast(double x, const sincosf_t &p, int *np)
{
    const double r = x * p.hpi_inv;
    const int n = ((int32_t) r + 0x800000) >> 24;
    *np = n;
    return kg_fma(-(double) n, p.hpi, x);
}

KG_HD double reduce_large(uint32_t xi, int *np)
{
    const int a = (int) ((xi >> 26) & 15u);
    const int shift = (int) ((xi >> 23) & 7u);
    xi = (xi & 0xffffffu) | 0x800000u;
    xi <<= shift;
    uint64_t res0 = (uint64_t) (uint32_t) (xi * inv_pio4(a));
    const uint64_t res1 = (uint64_t) xi * inv_pio4(a + 4);
    const uint64_t res2 = (uint64_t) xi * inv_pio4(a + 8);
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    const uint64_t n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    *np = (int) n;
    return (double) (int64_t) res0 * 0x1.921FB54442D18p-62;
}

// sin (cos = 0) or cos (cos = 1) of a float
KG_HD float sincosf_glibc(float y, int cos)
{
    double x = y;
    int n;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        if (abstop12(y) < abstop12(0x1p-12f)) return cos ? 1.0f : y;
        return sinf_poly(x, x * x, sincosf_tab(0), cos);
    }
    if (abstop12(y) < abstop12(120.0f)) {
        x = reduce_fast(x, sincosf_tab(0), &n);
        const double s = sincosf_tab(0).sign[n & 3];
        return sinf_poly(x * s, x * x, sincosf_tab((n & 2) ? 1 : 0), n ^ cos);
    }
    if (abstop12(y) < abstop12(__builtin_huge_valf())) {
        const uint32_t xi = f2u(y);
        const int sign = (int) (xi >> 31);
        x = reduce_large(xi, &n);
        const double s = sincosf_tab(0).sign[(n + sign) & 3];
        return sinf_poly(x * s, x * x, sincosf_tab(((n + sign) & 2) ? 1 : 0), n ^ cos);
    }
    return __builtin_nanf("");                                          // __math_invalidf: Inf, NaN
}
KG_HD float sinf_glibc(float x) { return sincosf_glibc(x, 0); }
KG_HD float cosf_glibc(float x) { return sincosf_glibc(x, 1); }

KG_HD float atanf_glibc(float x)                                        // s_atanf.c
{
    const float atanhi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
    const float atanlo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
    const float aT[11] = {3.3333334327e-01f, -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f, 9.0908870101e-02f,
                          -7.6918758452e-02f, 6.6610731184e-02f, -5.8335702866e-02f, 4.9768779427e-02f, -3.6531571299e-02f,
                          1.6285819933e-02f};
    const int32_t hx = (int32_t) f2u(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c000000) {                                            // |x| >= 2^25
        if (ix > 0x7f800000) return x + x;                             // NaN
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {                                             // |x| < 0.4375
        if (ix < 0x31000000) return x;                                 // |x| < 2^-29
        id = -1;
    } else {
        x = u2f((uint32_t) ix);
        if (ix < 0x3f980000) {                                         // |x| < 1.1875
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else { id = 3; x = -1.0f / x; }
        }
    }
    float z = x * x;
    const float w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    z = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -z : z;
}

KG_HD float atan2f_glibc(float y, float x)                              // e_atan2f.c
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f,
                pi_lo = -8.7422776573e-08f;
    const int32_t hx = (int32_t) f2u(x), ix = hx & 0x7fffffff, hy = (int32_t) f2u(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;               // NaN
    if (hx == 0x3f800000) return atanf_glibc(y);                        // x = 1
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);                  // 2 sign(x) + sign(y)
    if (iy == 0) {
        if (m < 2) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) {
            switch (m) {
            case 0: return pi_o_4 + tiny;
            case 1: return -pi_o_4 - tiny;
            case 2: return 3.0f * pi_o_4 + tiny;
            default: return -3.0f * pi_o_4 - tiny;
            }
        }
        switch (m) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return pi + tiny;
        default: return -pi - tiny;
        }
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int32_t k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;                              // |y / x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0f;                               // |y| / x < -2^60
    else z = atanf_glibc(__builtin_fabsf(y / x));
    switch (m) {
    case 0: return z;
    case 1: return u2f(f2u(z) ^ 0x80000000u);
    case 2: return pi - (z - pi_lo);
    default: return (z - pi_lo) - pi;
    }
}
#undef KG_HD
}  // namespace kg_libm
#endif
