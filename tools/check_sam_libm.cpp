// Host-side exhaustive check of csrc/kg_libm_trig.h's sinf / cosf / atan2f restatements against the image's libm (the functions
// rx/wdsp/SAM_demod.cpp calls).  The restatements are __host__ __device__: this runs the very code the kernels inline, on a CPU.
//
//   hipcc -O2 -std=c++17 -ffp-contract=off -pthread tools/check_sam_libm.cpp -o check_sam_libm && ./check_sam_libm [threads]
//
// sinf / cosf: every float with |x| <= 120 (the reduce_fast range, which holds the PLL's phase), then every other float (reduce_large,
// Inf, NaN).  atan2f: 2^26 random (y, x) pairs of random bit patterns, 2^26 pairs from the PLL's operating range (|y|, |x| < 2^20 as
// float), and every pairing of 46 special values (signed zeros, infinities, NaN, subnormals, 1, the 2^60 ratio edges).  A difference
// is a bit difference, except that a NaN result equals a NaN result.
#include "../flydog_sdr_gps_amd/csrc/kg_libm_trig.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>

static bool same(float a, float b)
{
    uint32_t ua, ub;
    memcpy(&ua, &a, 4); memcpy(&ub, &b, 4);
    return ua == ub || (a != a && b != b);
}

static uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <typename F> static void parallel(int nt, uint64_t total, F f)
{
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([=] { f(total * t / nt, total * (t + 1) / nt, t); });
    for (auto &x : th) x.join();
}

int main(int argc, char **argv)
{
    const int nt = argc > 1 ? atoi(argv[1]) : 8;
    // ---- sinf / cosf over all 2^32 patterns, counted by range
    std::atomic<uint64_t> n_in{0}, bad_in{0}, n_out{0}, bad_out{0};
    std::atomic<uint32_t> first_bad{0xffffffffu};
    parallel(nt, 1ull << 32, [&](uint64_t a, uint64_t b, int) {
        uint64_t ni = 0, bi = 0, no = 0, bo = 0;
        for (uint64_t u = a; u < b; u++) {
            const float x = kg_libm::u2f((uint32_t) u);
            const bool in = fabsf(x) <= 120.0f;
            const bool ok = same(kg_libm::sinf_glibc(x), sinf(x)) && same(kg_libm::cosf_glibc(x), cosf(x));
            if (in) { ni++; bi += !ok; } else { no++; bo += !ok; }
            if (!ok) { uint32_t f = first_bad.load(); while ((uint32_t) u < f && !first_bad.compare_exchange_weak(f, (uint32_t) u)) {} }
        }
        n_in += ni; bad_in += bi; n_out += no; bad_out += bo;
    });
    printf("sinf/cosf |x| <= 120: %llu floats, %llu differences\n", (unsigned long long) n_in, (unsigned long long) bad_in);
    printf("sinf/cosf |x| > 120, Inf, NaN: %llu floats, %llu differences\n", (unsigned long long) n_out, (unsigned long long) bad_out);
    if (bad_in || bad_out) printf("  first difference at 0x%08x\n", first_bad.load());
    // ---- atan2f
    std::atomic<uint64_t> bad_r{0}, bad_p{0};
    const uint64_t NR = 1ull << 26;
    parallel(nt, NR, [&](uint64_t a, uint64_t b, int t) {
        uint64_t s = 0x5a3d1e00ull + a, br = 0, bp = 0;
        for (uint64_t i = a; i < b; i++) {
            const uint64_t r = splitmix(s);
            const float y = kg_libm::u2f((uint32_t) r), x = kg_libm::u2f((uint32_t) (r >> 32));
            br += !same(kg_libm::atan2f_glibc(y, x), atan2f(y, x));
            const uint64_t q = splitmix(s);                                    // the correlator's range
            const float yp = (float) ((int32_t) (uint32_t) q >> 11) * 0.5f, xp = (float) ((int32_t) (uint32_t) (q >> 32) >> 11) * 0.5f;
            bp += !same(kg_libm::atan2f_glibc(yp, xp), atan2f(yp, xp));
        }
        bad_r += br; bad_p += bp;
        (void) t;
    });
    const float sp[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, -NAN, 1.0f, -1.0f, 1e-45f, -1e-45f, 1.1754942e-38f, -1.1754942e-38f,
                        1.17549435e-38f, 3.4028235e38f, -3.4028235e38f, 0x1p60f, 0x1p61f, 0x1p-60f, 0x1p-61f, 0x1p34f, 0x1p-29f,
                        0.4375f, 0.6875f, 1.1875f, 2.4375f, -0.4375f, 3.0f, 1e-38f, 5e-39f, 0x1.fffffep-127f, 0.5f, 1.5f, 2.0f,
                        -2.0f, 1e30f, -1e30f, 1e-30f, 100.0f, -100.0f, 7.0f, 0x1p25f, 0x1p26f, 0x1p-25f, 3.14159274f, -3.14159274f, 1e-20f};
    const int NS = sizeof sp / sizeof sp[0];
    int bad_s = 0;
    for (int i = 0; i < NS; i++)
        for (int j = 0; j < NS; j++)
            if (!same(kg_libm::atan2f_glibc(sp[i], sp[j]), atan2f(sp[i], sp[j]))) {
                if (bad_s++ < 8) printf("  atan2f(%a, %a): %a vs libm %a\n", sp[i], sp[j], kg_libm::atan2f_glibc(sp[i], sp[j]), atan2f(sp[i], sp[j]));
            }
    printf("atan2f: %llu random bit patterns %llu differences; %llu correlator-range pairs %llu differences; %d special pairs %d differences\n",
           (unsigned long long) NR, (unsigned long long) bad_r, (unsigned long long) NR, (unsigned long long) bad_p, NS * NS, bad_s);
    const bool ok = !bad_in && !bad_out && !bad_r && !bad_p && !bad_s;
    printf("%s\n", ok ? "ok" : "DIFFERENCES");
    return ok ? 0 : 1;
}
