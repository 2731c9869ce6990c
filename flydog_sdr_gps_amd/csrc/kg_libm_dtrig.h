// kg_libm_dtrig.h -- sin and cos in double of a FLOAT-VALUED argument with |x| <= 2.5, CORRECTLY ROUNDED, on the device AND the host.
// For the seeds of the WSPR decoder's phase recurrences (extensions/wspr/wspr.cpp:96-110): the reference takes them from the host's
// libm, whose double sin / cos is not correctly rounded and cannot be restated from a published method bit for bit (stage
// 2).  So the host twin and the kernels share THIS function, and the golden's maker builds the reference a second time with it.
// Apart from kg_libm.h / kg_libm_trig.h because those two are pinned as text by a test.
//
// The method: double-double arithmetic (Dekker, Knuth; the accurate sum of Joldes, Muller and Popescu, relative error <= 3 u^2 with
// no condition on cancellation), every product's low part by an explicit fma.  k = round(x 2/pi) is 0, 1 or 2; r = x - k pi/2 with pi/2
// in three doubles (k P1 is exact: k is 1 or 2); sin r and cos r by their Taylor series in z = r^2, Horner in double-double, to
// r^27 / 27! and r^28 / 28! (|r| <= pi/4: the first term left out is below 2^-107 of the result); the quadrant picks one and its sign.
// The sum is normalised, so its high part is the nearest double unless the value lies within about 2^-100 of a rounding boundary --
// tools/check_wspr_dtrig.cpp runs ALL floats of the domain against libquadmath (profiles/wspr_dtrig_check.txt): none does.
// Outside the domain (|x| > 2.5, Inf, NaN) the result is NaN: the decoder refuses the candidates that could get there.
#ifndef KG_LIBM_DTRIG_H
#define KG_LIBM_DTRIG_H

#if defined(__HIPCC__)
#define KG_DT_HD __host__ __device__ __forceinline__
#else
#define KG_DT_HD inline
#endif

namespace kg_libm {

struct dd_t { double hi, lo; };

KG_DT_HD dd_t dd_two_sum(double a, double b)                  // a + b = s + e exactly
{
    const double s = a + b, bb = s - a;
    return dd_t{s, (a - (s - bb)) + (b - bb)};
}
KG_DT_HD dd_t dd_fast_two_sum(double a, double b)             // the same for |a| >= |b|
{
    const double s = a + b;
    return dd_t{s, b - (s - a)};
}
KG_DT_HD dd_t dd_add(dd_t a, dd_t b)
{
    dd_t s = dd_two_sum(a.hi, b.hi);
    const dd_t t = dd_two_sum(a.lo, b.lo);
    s = dd_fast_two_sum(s.hi, s.lo + t.hi);
    return dd_fast_two_sum(s.hi, s.lo + t.lo);
}
KG_DT_HD dd_t dd_mul(dd_t a, dd_t b)
{
    const double p = a.hi * b.hi;
    const double e = __builtin_fma(a.hi, b.hi, -p);
    return dd_fast_two_sum(p, __builtin_fma(a.hi, b.lo, __builtin_fma(a.lo, b.hi, e)));
}

#define KG_DT_PIO2_1 0x1.921fb54442d18p+0
#define KG_DT_PIO2_2 0x1.1a62633145c07p-54
#define KG_DT_PIO2_3 (-0x1.f1976b7ed8fbcp-110)
#define KG_DT_2OPI 0x1.45f306dc9c883p-1

// (-1)^k / (2k + 3)! and (-1)^(k + 1) / (2k + 2)! to twice double precision
KG_DT_HD dd_t dtrig_sin_c(int k)
{
    static constexpr dd_t c[13] = {
        {-0x1.5555555555555p-3, -0x1.5555555555555p-57},   {0x1.1111111111111p-7, 0x1.1111111111111p-63},     {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73},
        {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},   {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80},   {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
        {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97},  {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},   {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112},
        {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},  {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130},  {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139},
        {-0x1.d1ab1c2dccea3p-94, -0x1.054d0c78aea14p-149}};
    return c[k];
}
KG_DT_HD dd_t dtrig_cos_c(int k)
{
    static constexpr dd_t c[14] = {
        {-0x1.0000000000000p-1, 0.0},                      {0x1.5555555555555p-5, 0x1.5555555555555p-59},     {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65},
        {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},    {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76},  {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
        {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92},  {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},   {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107},
        {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},   {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124},  {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135},
        {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143},  {0x1.0a18a2635085dp-98, 0x1.b9e2e28e1aa54p-153}};
    return c[k];
}

// sin r (want_cos = 0) or cos r of a double-double |r| <= pi/4
KG_DT_HD dd_t dtrig_kernel(dd_t r, int want_cos)
{
    const dd_t z = dd_mul(r, r);
    if (want_cos) {
        dd_t s = dtrig_cos_c(13);
#pragma unroll
        for (int k = 12; k >= 0; k--) s = dd_add(dd_mul(s, z), dtrig_cos_c(k));
        return dd_add(dd_t{1.0, 0.0}, dd_mul(z, s));
    }
    dd_t s = dtrig_sin_c(12);
#pragma unroll
    for (int k = 11; k >= 0; k--) s = dd_add(dd_mul(s, z), dtrig_sin_c(k));
    return dd_add(r, dd_mul(dd_mul(r, z), s));
}

// sin (want_cos = 0) or cos of x, a double that holds a float's value, |x| <= 2.5
KG_DT_HD double dtrig_f2d(double x, int want_cos)
{
    const double ax = x < 0 ? -x : x;
    if (!(ax <= 2.5)) return __builtin_nan("");
    if (ax == 0.0) return want_cos ? 1.0 : x;                                   // sin keeps the zero's sign
    const int k = (int) (ax * KG_DT_2OPI + 0.5);                                // 0, 1, 2
    dd_t r = dd_t{ax, 0.0};
    if (k) {
        const double kd = (double) k;
        r = dd_add(dd_add(r, dd_t{-kd * KG_DT_PIO2_1, -kd * KG_DT_PIO2_2}), dd_t{-kd * KG_DT_PIO2_3, 0.0});
    }
    // quadrant k: sin = sin r, cos r, -sin r;  cos = cos r, -sin r, -cos r
    const dd_t v = dtrig_kernel(r, (want_cos ^ k) & 1);
    const bool neg = want_cos ? (k != 0) : ((k == 2) != (x < 0));
    return neg ? -v.hi : v.hi;
}
KG_DT_HD double sin_f2d(double x) { return dtrig_f2d(x, 0); }
KG_DT_HD double cos_f2d(double x) { return dtrig_f2d(x, 1); }

}  // namespace kg_libm
#endif
