// Developer tool: kg_libm::sin_f2d / cos_f2d (csrc/kg_libm_dtrig.h) on EVERY float with 0 < |x| <= 2.5 against libquadmath's sinq / cosq
// rounded to double -- the judge of "correctly rounded".  Positive arguments go to the judge; the negative ones are held to the symmetry
// (sin odd, cos even, bit for bit).  At most 16 threads.  Its summary is kept in profiles/wspr_dtrig_check.txt.
//   g++ -O2 -ffp-contract=off -mfma -pthread -o check_wspr_dtrig tools/check_wspr_dtrig.cpp -lquadmath && ./check_wspr_dtrig
#include <quadmath.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_libm_dtrig.h"

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv)
{
    uint32_t last;
    const float top = 2.5f;
    memcpy(&last, &top, 4);
    const uint32_t step = argc > 1 ? (uint32_t) atoi(argv[1]) : 1;                // a stride, for a quick look
    const unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::mutex m;
    uint64_t total = 0, bad_sin = 0, bad_cos = 0, bad_sym = 0;
    std::vector<uint32_t> shown;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            uint64_t n = 0, bs = 0, bc = 0, by = 0;
            std::vector<uint32_t> mine;
            for (uint64_t u = 1 + (uint64_t) t * step; u <= last; u += (uint64_t) nt * step) {
                const uint32_t w = (uint32_t) u;
                float f;
                memcpy(&f, &w, 4);
                const double x = f;
                const double s = kg_libm::sin_f2d(x), c = kg_libm::cos_f2d(x);
                const double ws = (double) sinq((__float128) x), wc = (double) cosq((__float128) x);
                n++;
                if (bits(s) != bits(ws)) { bs++; if (mine.size() < 16) mine.push_back(w); }
                if (bits(c) != bits(wc)) { bc++; if (mine.size() < 16) mine.push_back(w); }
                if (bits(kg_libm::sin_f2d(-x)) != bits(-s) || bits(kg_libm::cos_f2d(-x)) != bits(c)) by++;
            }
            std::lock_guard<std::mutex> g(m);
            total += n; bad_sin += bs; bad_cos += bc; bad_sym += by;
            shown.insert(shown.end(), mine.begin(), mine.end());
        });
    for (auto &x : th) x.join();
    const bool zero_ok = bits(kg_libm::sin_f2d(0.0)) == bits(0.0) && bits(kg_libm::sin_f2d(-0.0)) == bits(-0.0) && kg_libm::cos_f2d(0.0) == 1.0 && kg_libm::cos_f2d(-0.0) == 1.0;
    const double out = kg_libm::sin_f2d((double) __builtin_nextafterf(2.5f, 3.0f));
    printf("floats with 0 < x <= 2.5, every %u-th: %llu arguments, %u threads\n", step, (unsigned long long) total, nt);
    printf("sin_f2d differs from (double) sinq: %llu\ncos_f2d differs from (double) cosq: %llu\n", (unsigned long long) bad_sin, (unsigned long long) bad_cos);
    printf("sin(-x) != -sin(x) or cos(-x) != cos(x): %llu\n", (unsigned long long) bad_sym);
    printf("zeros: %s; the float above 2.5 gives %s\n", zero_ok ? "sin(+-0) = +-0, cos(+-0) = 1" : "WRONG", out != out ? "NaN" : "A NUMBER");
    for (uint32_t w : shown) printf("  argument bits 0x%08x\n", w);
    return (bad_sin || bad_cos || bad_sym || !zero_ok || out == out) ? 1 : 0;
}
