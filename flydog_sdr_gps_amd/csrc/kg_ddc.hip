// kg_ddc.hip -- the waterfall digital down-converter on gfx950.
//
// In the reference this is FPGA fabric, one instance per waterfall channel,
// clocked at the ADC rate:  IQ_MIXER (verilog/rx/iq_mixer.v:5-67: 48-bit phase
// accumulator, 15-bit sin/cos, 18x18 multiply, round to 24 bits)
// -> cic_prune_var "wf1" x2 (verilog/rx/cic_prune_var.v + cic_wf1.vh: 5
// integrators at the ADC rate, 89-bit wrapping accumulators, decimate by
// R = 2^k <= 8192, 5 combs, Hogenauer-pruned widths 89/89/89/89/28 and
// 23/22/21/20/20, rounded to 16 bits; R = 1 bypass) -> 16-bit IQ into the
// 8192-sample buffer the host reads as iq_t (verilog/rx/waterfall_1cic.v:58-142).
// The host programs it with CmdSetWFFreq / CmdSetWFDecim / CmdWFReset
// (rx/rx_waterfall.cpp:466,507,1005).  Here the ADC stream lives in HBM and all
// channels are computed from it.
//
// Bit-exactness target: a sequential restatement of the Verilog structure (the
// tests' CPU model).  Frozen by us because the Xilinx DDS IP is closed: the sine
// table, round(16383 cos/sin) addressed by phase bits 47:35, and no phase dither.
//
// Parallelisation.  The integrators are prefix sums over the whole stream and the
// pruning (the 5th integrator accumulates floor(I4 / 2^61)) makes the output depend
// on the exact wrapped value of I4 at every ADC sample, so time cannot simply be
// cut into independent pieces.  The stream is cut into runs of L samples:
//   A  every run integrates from a zero state -> local end state e_r, advanced to the END
//      of the channel's share of the block: T(len) advances a state over len zero-input
//      samples (binomial coefficients; validated in tools/ and the tests)
//   S  carry scan: end-referred, the states the runs start from are a plain prefix SUM
//      of pass A's results (the argument is above sub96), taken in levels: over the 256
//      runs of a workgroup inside pass A itself (ddc_wf_run_kernel), then by one wave per
//      (channel, I/Q) over the at most 64 workgroup totals, which also adds the carried-in
//      state and leaves the state after the block (ddc_wf_scan_wg_kernel)
//   B  every run takes its exact start state back from the end, integrates again, feeds
//      the pruned 5th integrator and records its value at every decimation strobe
//      (relative to the run start) plus the run total
//   S2 prefix sum of the run totals (mod 2^28) in the same levels: inside pass B's
//      workgroups, then one wave over the workgroup totals (ddc_wf_tau_wg_kernel); the
//      combs add the two levels
//   C  per output: absolute I5, the five pruned combs (a 6-tap dependency on
//      earlier outputs only, so fully parallel), rounding, int16 store.
// Nothing above bit 88 of an integrator is ever read, so any modulus 2^k with k >= 89 keeps
// the result exact: the run passes work modulo 2^64 on (state >> shift) where 24 + 5 log2 R
// <= 64, modulo 2^96 (three 32-bit limbs) above that, and the scan modulo 2^96 throughout;
// states are stored 128 bits wide (upper limb zero).
#include <type_traits>
#include "kg_common.h"
#include "kg_ddc_plan.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef unsigned long long u64;
typedef unsigned int u32;

struct u128 { u64 lo, hi; };

#define DDC_DEV __device__ __forceinline__

DDC_DEV u128 mk128(u64 lo, u64 hi) { u128 r; r.lo = lo; r.hi = hi; return r; }
DDC_DEV u128 add128(u128 a, u128 b)
{
    u128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}
DDC_DEV u128 mul128(u128 a, u128 b)          // modulo 2^128
{
    u128 r;
    r.lo = a.lo * b.lo;
    r.hi = __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
    return r;
}
// j(j+1)/2 and j(j+1)(j+2)/6 exactly (j < 2^40), as 128-bit values
DDC_DEV u128 binom2(u64 j)
{
    const u64 a = (j & 1) ? j : j / 2, b = (j & 1) ? (j + 1) / 2 : j + 1;
    return mk128(a * b, __umul64hi(a, b));
}
DDC_DEV u128 binom3(u64 j)
{
    // j (j+1) (j+2) < 2^120 is even and a multiple of 3: halve it, then divide by 3 exactly =
    // multiply by the inverse of 3 modulo 2^128 (no 64-bit division: that is a software loop here)
    const u128 ab = mk128(j * (j + 1), __umul64hi(j, j + 1));
    u128 p = mul128(ab, mk128(j + 2, 0));
    p.lo = (p.lo >> 1) | (p.hi << 63); p.hi >>= 1;
    return mul128(p, mk128(0xAAAAAAAAAAAAAAABull, 0xAAAAAAAAAAAAAAAAull));
}

struct ddc_state4 { u128 i[4]; };            // integrators 1..4

// Per-channel persistent state (HBM).
struct ddc_chan {
    // phase and sample_no are REFERENCE values: the NCO accumulator and the decimation counter as they stood when the host
    // last set them (set_wf / set_phase / reset).  A push passes the number of samples pushed since then (`pushed`, the
    // same for every channel of the call) and every kernel derives its own start values from it: no kernel writes these
    // two fields, so kernels of consecutive pushes on different streams (round 4: the deferred output stage) all read
    // consistent values.
    u64 phase;            // 48-bit NCO accumulator at the reference point
    u64 phase_inc;        // CmdSetWFFreq (rx_waterfall.cpp:507)
    int log2r;            // CmdSetWFDecim: R = 1 << log2r
    u32 sample_no;        // decimation counter (cic_prune_var.v:65-80) at the reference point
    ddc_state4 integ[2];  // I, Q integrators 1..4
    u32 integ5[2];        // 28-bit integrator 5
    u32 hist[2][5];       // integrator-5 value at the last five strobes (what the comb registers hold)
    int active;
};

// iq_mixer.v:27-51, IN_WIDTH 16, OUT_WIDTH 24: (prod >>> 11) + prod[10], prod = (adc<<2)*(dds<<3)
// prod = 32 * adc * dds and |adc * dds| < 2^30, so in 32-bit arithmetic: (m >> 6) + bit 5 of m
DDC_DEV int mix24(int adc, int dds)
{
    const int m = adc * dds;
    return (m + 32) >> 6;                     // = (m >> 6) + bit 5 of m, one instruction fewer (|m| < 2^30)
}

#define DDC_THREADS 256
#define DDC_TAB KG_NCO_TAB            // NCO table entries: sin(a) = T[a], cos(a) = T[a + 2048], a < 8192
#ifndef DDC_STAGE_STROBES
#define DDC_STAGE_STROBES 16      // strobes per run collected before a flush: 64 bytes per run and store (8 = half lines: ddc14 +6 %)
#endif
#define DDC_STAGE_ROW (DDC_STAGE_STROBES + 1)    // words per lane row of a staging tile (odd stride: conflict-free)
#define DDC_STAGE_BYTES ((DDC_THREADS / 64) * 2 * 64 * DDC_STAGE_ROW * 4)

// The scan's arithmetic.  Nothing above bit 88 of an integrator is ever read, so the scan keeps a state as 4 x 96
// bits in 32-bit limbs (the stored form stays 128 bits wide, upper limb zero): a product with a coefficient is
// 3 / 5 / 6 multiply-adds of 32 x 32 -> 64 bits (the run length and its binomials have 1-2 / 2 / 3 limbs) where
// the 128 x 128-bit product took some forty-five instructions, and a state crosses lanes in 12 shuffles, not 32.
struct u96 { u32 w[3]; };
struct sc4 { u96 i[4]; };                     // integrators 1..4, mod 2^96
struct sc_coef { u64 L, c2; u96 c3; };        // len, len (len+1) / 2 (exact: len < 2^32, asserted beside DDC_RUN_MAX), len (len+1) (len+2) / 6 mod 2^96
DDC_DEV u96 u96_zero() { u96 r; r.w[0] = r.w[1] = r.w[2] = 0; return r; }
DDC_DEV u96 u96_of(const u128 &v) { u96 r; r.w[0] = (u32) v.lo; r.w[1] = (u32) (v.lo >> 32); r.w[2] = (u32) v.hi; return r; }
DDC_DEV u128 u128_of(const u96 &v) { return mk128((u64) v.w[0] | ((u64) v.w[1] << 32), (u64) v.w[2]); }
DDC_DEV u96 add96(const u96 &a, const u96 &b)
{
    u96 r; unsigned c0, c1;
    r.w[0] = __builtin_addc(a.w[0], b.w[0], 0u, &c0);
    r.w[1] = __builtin_addc(a.w[1], b.w[1], c0, &c1);
    r.w[2] = a.w[2] + b.w[2] + c1;
    return r;
}
DDC_DEV u96 mul96_64(const u96 &a, u64 b)      // a * b mod 2^96
{
    const u32 b0 = (u32) b, b1 = (u32) (b >> 32);
    const u64 p0 = (u64) a.w[0] * b0;
    const u64 p1 = (u64) a.w[1] * b0 + (p0 >> 32);
    const u64 q0 = (u64) a.w[0] * b1 + (u32) p1;
    u96 r;
    r.w[0] = (u32) p0;
    r.w[1] = (u32) q0;
    r.w[2] = a.w[2] * b0 + a.w[1] * b1 + (u32) (p1 >> 32) + (u32) (q0 >> 32);
    return r;
}
DDC_DEV u96 mul96_96(const u96 &a, const u96 &b)
{
    u96 r = mul96_64(a, (u64) b.w[0] | ((u64) b.w[1] << 32));
    r.w[2] += a.w[0] * b.w[2];
    return r;
}
DDC_DEV sc_coef sc_coef_for(u64 len)
{
    sc_coef c;
    c.L = len; c.c2 = binom2(len).lo; c.c3 = u96_of(binom3(len));
    return c;
}
DDC_DEV sc4 sc_zero() { sc4 r; for (int k = 0; k < 4; k++) r.i[k] = u96_zero(); return r; }
DDC_DEV sc4 sc_of(const ddc_state4 &s) { sc4 r; for (int k = 0; k < 4; k++) r.i[k] = u96_of(s.i[k]); return r; }
DDC_DEV ddc_state4 state_of(const sc4 &s) { ddc_state4 r; for (int k = 0; k < 4; k++) r.i[k] = u128_of(s.i[k]); return r; }
// advance a state over len zero-input samples: the binomial matrix of the four cascaded integrators
DDC_DEV sc4 sc_Tc(const sc_coef &k, const sc4 &s)
{
    sc4 r;
    r.i[0] = s.i[0];
    r.i[1] = add96(s.i[1], mul96_64(s.i[0], k.L));
    r.i[2] = add96(add96(s.i[2], mul96_64(s.i[1], k.L)), mul96_64(s.i[0], k.c2));
    r.i[3] = add96(add96(add96(s.i[3], mul96_64(s.i[2], k.L)), mul96_64(s.i[1], k.c2)), mul96_96(s.i[0], k.c3));
    return r;
}
DDC_DEV sc4 sc_T(u64 len, const sc4 &s) { return sc_Tc(sc_coef_for(len), s); }
DDC_DEV sc4 sc_add(const sc4 &a, const sc4 &b) { sc4 r; for (int k = 0; k < 4; k++) r.i[k] = add96(a.i[k], b.i[k]); return r; }
DDC_DEV sc4 sc_shfl(const sc4 &s, int src)
{
    sc4 r;
    for (int k = 0; k < 4; k++) for (int w = 0; w < 3; w++) r.i[k].w[w] = __shfl(s.i[k].w[w], src);
    return r;
}
DDC_DEV sc4 sc_shfl_up(const sc4 &s, int d)
{
    sc4 r;
    for (int k = 0; k < 4; k++) for (int w = 0; w < 3; w++) r.i[k].w[w] = __shfl_up(s.i[k].w[w], d);
    return r;
}

// Round 4: END-REFERRED states.  T(a) T(b) = T(a + b) for every integer a, b (the binomial matrix of the cascaded
// integrators), so the state a run starts from, sum over the earlier runs j of T(s0 - s1_j) e_j + T(s0) S_0, is
// T(-(n - s0)) [ sum_j T(n - s1_j) e_j + T(n) S_0 ]: pass A advances its zero-state result to the END of the entry's share
// of the block (one advance per run, in the pass that has 17 instructions per sample to hide it in), the carry scan is a
// plain prefix SUM of 96-bit words -- no multiplications, no lengths -- and pass B takes its start state back from the end
// (one inverse advance per run); the state after the block is the sum itself.  A sum can be taken in levels wherever the
// values happen to be: inside pass A's workgroups, then over the workgroup totals (ddc_wf_run_kernel, ddc_wf_scan_wg_kernel)
// -- where the affine scan was a kernel of its own between the passes, 36 us alone and 57 us beside the bypass kernel (a
// chunked prefix-sum kernel in its place measured the same 36: waiting on other workgroups, not the multiplications, was
// its cost).
DDC_DEV u96 sub96(const u96 &a, const u96 &b)
{
    u96 r; unsigned c0, c1;
    r.w[0] = __builtin_subc(a.w[0], b.w[0], 0u, &c0);
    r.w[1] = __builtin_subc(a.w[1], b.w[1], c0, &c1);
    r.w[2] = a.w[2] - b.w[2] - c1;
    return r;
}
// T(-m): the coefficients of T(len) at len = -m are -m, m (m - 1) / 2, -m (m - 1) (m - 2) / 6  (m < 2^32)
DDC_DEV sc4 sc_Tinv(u64 m, const sc4 &s)
{
    if (m == 0) return s;
    const u64 c2 = binom2(m - 1).lo;
    const u96 c3 = m >= 2 ? u96_of(binom3(m - 2)) : u96_zero();
    sc4 r;
    r.i[0] = s.i[0];
    r.i[1] = sub96(s.i[1], mul96_64(s.i[0], m));
    r.i[2] = add96(sub96(s.i[2], mul96_64(s.i[1], m)), mul96_64(s.i[0], c2));
    r.i[3] = sub96(add96(sub96(s.i[3], mul96_64(s.i[2], m)), mul96_64(s.i[1], c2)), mul96_96(s.i[0], c3));
    return r;
}
DDC_DEV sc4 sc_Tinv_c(u64 m, u64 c2, const u96 &c3, const sc4 &s)
{
    sc4 r;
    r.i[0] = s.i[0];
    r.i[1] = sub96(s.i[1], mul96_64(s.i[0], m));
    r.i[2] = add96(sub96(s.i[2], mul96_64(s.i[1], m)), mul96_64(s.i[0], c2));
    r.i[3] = sub96(add96(sub96(s.i[3], mul96_64(s.i[2], m)), mul96_64(s.i[1], c2)), mul96_96(s.i[0], c3));
    return r;
}
// The distances to the end are the same for every channel that takes the whole block: n - k L, k = 0 .. nruns (run r ends
// at k = r + 1, starts at k = r).  Their coefficients -- 40 % of an advance, 128-bit products -- come from a table built
// once per (n, L) (ddc_endco_kernel; a steady stream of equal blocks builds it once); an entry with another share of the
// block (a capture) computes its own.
struct ddc_endco { u64 m, c2, c2i; u96 c3, c3i; u32 pad[2]; };        // T(m): m, c2, c3;  T(-m): -m, c2i, -c3i
// Pass A: a run's result advanced over its distance `len` to the end (modulo 2^96, as the sums that follow)
DDC_DEV sc4 ddc_to_end(const ddc_state4 &e, u64 len, const ddc_endco *__restrict__ co)
{
    if (co) {
        sc_coef k; k.L = co->m; k.c2 = co->c2; k.c3 = co->c3;
        return sc_Tc(k, sc_of(e));
    }
    return sc_T(len, sc_of(e));
}
// Pass B: the state a run starts from = (the sum of its workgroup's runs before it + what the workgroup starts from), both
// referred to the end, taken back over the run's distance `len` to the end.  (One function, 96 bits from the sum to the
// inverse advance, and pass A's results likewise as sc4 up to the kernel's prefix sum: the same arithmetic written as
// separate steps through the 128-bit stored form allocated 100 registers in pass B's narrow form and 131 in pass A's general
// one, a wave per SIMD fewer each, though its live values never exceed 83 and 102 -- kernel-resource-usage remarks.)
DDC_DEV ddc_state4 ddc_run_start(const ddc_state4 &before, const ddc_state4 &wg, u64 len, const ddc_endco *__restrict__ co)
{
    const sc4 s = sc_add(sc_of(before), sc_of(wg));
    if (co) return state_of(sc_Tinv_c(co->m, co->c2i, co->c3i, s));
    return state_of(sc_Tinv(len, s));
}
__global__ void ddc_endco_kernel(ddc_endco *__restrict__ tab, long n, int L, int nruns)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nruns) return;
    const long at = (long) k * L;
    const u64 m = at < n ? (u64) (n - at) : 0ull;
    ddc_endco c;
    c.m = m; c.c2 = binom2(m).lo; c.c3 = u96_of(binom3(m));
    c.c2i = m >= 1 ? binom2(m - 1).lo : 0ull;
    c.c3i = m >= 2 ? u96_of(binom3(m - 2)) : u96_zero();
    c.pad[0] = c.pad[1] = 0;
    tab[k] = c;
}
// inclusive prefix sum over lanes 0 .. 2^LOG - 1 (every lane of the group calls it)
template <int LOG> DDC_DEV void sc_scan_add(sc4 &e, int lane)
{
#pragma unroll
    for (int d = 1; d < (1 << LOG); d <<= 1) {
        const sc4 a = sc_shfl_up(e, d);
        if (lane >= d) e = sc_add(a, e);
    }
}

// Passes A and B.  grid = (ceil(nruns / 256), nchan).  The body of a thread's run; the kernel below adds the
// workgroup-level prefix sums of pass A's end-referred results and of pass B's integrator-5 totals.
// MODE (round 5): which of the body's forms an instantiation carries.  The register budget of a kernel is that of its
// widest form -- with everything in one function 119 / 124 registers, four waves per SIMD, for passes that stall on
// table reads and dependent adds and gain from every further wave -- so the launches are split by what their entries need:
//   DDC_ALL     every form (the staged and vector-store forms of R <= 8, the 128-bit pass A of runs longer than 1024)
//   DDC_NARROW  the 64-bit form alone: pass A of any decimation in runs of at most 1024 samples, pass B of 16 <= R <= 256
//   DDC_WIDE    pass B of R >= 512 alone (96-bit integrators)
enum { DDC_ALL = 0, DDC_NARROW = 1, DDC_WIDE = 2 };
template <bool PASS_B, int MODE>
DDC_DEV void ddc_wf_run_body(
    const short *__restrict__ adc, long n, int L, int nruns,
    const ddc_chan *__restrict__ chans, const int *__restrict__ chan_list,
    const u32 *__restrict__ nco,              // the 16-bit table T[DDC_TAB] (kg_ddc_create), two entries per word
    ddc_state4 *__restrict__ local,           // B: in [nlist][2][nruns]: the end-referred sum of the workgroup's runs before this one
    u32 *__restrict__ c0rel,                  // B: relative I5 at strobes; entry li: I at c0off[li], Q right after
    const long *__restrict__ c0off, const long *__restrict__ nouts,
    const int *__restrict__ sel,              // list entries this launch covers (null: all, in order)
    int stage_bytes,                          // pass B, R <= 8: dynamic LDS for the strobe staging tiles, else 0
    u64 pushed,                               // samples pushed since the call's reference point: the entry's own count is
    const u64 *__restrict__ pdelta,           //   pushed + pdelta[li] (channels retuned or joined at different times differ in age)
    const long *__restrict__ nlim,            // [nlist] samples of the block this entry consumes (capture: 8192 R; else n)
    const int *__restrict__ reset_tab,        // [nlist] capture: the decimation counter starts the block at zero (rst_wf_samp_wr)
    const ddc_endco *__restrict__ endco, long endco_n,    // [nruns + 1] coefficients of the distances n - k L for a share of endco_n samples
    const ddc_state4 *__restrict__ wgbase,    // B: in [nlist][2][gridDim.x] what the workgroup's first run adds to local[]: both are referred to
                                              //    the END of the entry's share (sc_Tinv above)
    sc4 &outI, sc4 &outQ, bool &have,         // A: the run's end-referred result, for the caller's prefix sum (have: this thread has a run)
    u32 &outTi, u32 &outTq)                   // B: the run's integrator-5 totals likewise
{
    __shared__ short tab[DDC_TAB];
    extern __shared__ u32 stage_lds[];        // [waves][2][64][DDC_STAGE_ROW] when stage_bytes != 0
    for (int i = threadIdx.x; i < DDC_TAB / 2; i += DDC_THREADS) ((u32 *) tab)[i] = nco[i];
    __syncthreads();
    const int li = sel ? sel[blockIdx.y] : (int) blockIdx.y;
    const ddc_chan ch = chans[chan_list[li]];
    const int reset_first = reset_tab[li];
    pushed += pdelta[li];
    const int r = blockIdx.x * DDC_THREADS + threadIdx.x;
    n = nlim[li];                             // this entry's share of the block (wave-uniform)
    if (r >= nruns || (long) r * L >= n) return;
    const long s0 = (long) r * L, s1 = (s0 + L < n) ? s0 + L : n;
    const ddc_endco *co = n == endco_n ? endco + (PASS_B ? r : r + 1) : nullptr;
    const long wbI = ((long) li * 2 + 0) * gridDim.x + blockIdx.x, wbQ = ((long) li * 2 + 1) * gridDim.x + blockIdx.x;
    (void) wbI; (void) wbQ;
    // the 48-bit accumulator sits in the TOP bits of a 64-bit register: it wraps by itself (no mask per sample)
    u64 ph = (ch.phase + (pushed + (u64) s0) * ch.phase_inc) << 16;
    const u64 inc16 = ch.phase_inc << 16;
    const int log2r = ch.log2r;
    const u64 Rm1 = (1ull << log2r) - 1;
    const int shift = 65 - 5 * log2r;         // cic_prune_var.v:224-247

    if (log2r == 0) return;                   // R == 1 bypass: ddc_wf_bypass_kernel

    const u64 cnt_call = reset_first ? 0ull : (((u64) ch.sample_no + pushed) & Rm1);   // the decimation counter at the start of this call
    const u64 cnt0 = cnt_call + (u64) s0;                // samples since the counter was last zero
    const long lI = ((long) li * 2 + 0) * nruns + r, lQ = ((long) li * 2 + 1) * nruns + r;
    u32 i5i = 0, i5q = 0;
    u32 c = (u32) (cnt0 & Rm1);                           // decimation counter, sample_no
    long o = (long) (cnt0 >> log2r);                      // index of the next strobe's output
    u32 *c0i = c0rel + c0off[li], *c0q = c0i + ((nouts[li] + 3) & ~3l);      // planes start 16-byte aligned
    // eight samples per round from one 16-byte load (runs start 128-byte aligned relative to
    // the block; an unaligned block or the ragged end of the last run go sample by sample).
    // The load runs ONE GROUP AHEAD of the arithmetic: issued at the top of a group and consumed at the
    // top of the next, its L2 latency hides behind the ~170 instructions of the group in between (a
    // load consumed where it is issued stalled every group of every lane for the whole round trip).
    // The last whole group of a run re-reads itself: one load site, never skipped.
    const bool al = (((uintptr_t) (adc + s0)) & 15) == 0;          // L is a multiple of 8: every group of the run is aligned alike
    const long g1 = al ? s1 : s0;                                  // the group loops run to g1: a misaligned block goes sample by sample
    // Round 4: TWO groups ahead.  With the ADC stream coming from HBM (a block larger than the Infinity Cache, or one the
    // DMA engine has just written) the first touch of a 128-byte line -- one in eight of a lane's loads -- takes longer than
    // the one group of arithmetic the load used to run ahead of: the bench's rotation of nine 32 MiB blocks cost ddc14
    // 0.44 -> 0.47 ms.
    const long last_grp = g1 - 8;                                  // start of the run's last whole group (callers check s0 + 8 <= g1)
    int4 ahead = make_int4(0, 0, 0, 0), ahead2 = make_int4(0, 0, 0, 0);
    if (s0 + 8 <= g1) {
        ahead = *(const int4 *) (adc + s0);
        ahead2 = *(const int4 *) (adc + (s0 + 8 <= last_grp ? s0 + 8 : last_grp));
    }
    auto samples8 = [&](long t, short (&buf)[8]) {                 // callers guarantee t + 8 <= g1 and walk t in steps of 8 from s0
        const int4 v = ahead;
        ahead = ahead2;
        // (g1 is not needed here any more -- the single look-ahead that read it is gone -- but it stays captured, at this place:
        // without the capture the compiler allocates the registers of every kernel built from this body differently, and that
        // is a change to time on a GPU)
        (void) g1;
        const long tn = t + 16 <= last_grp ? t + 16 : last_grp;         // (the last groups re-read the run's last one: one load site, never skipped)
        ahead2 = *(const int4 *) (adc + tn);
        buf[0] = (short) v.x; buf[1] = (short) (v.x >> 16); buf[2] = (short) v.y; buf[3] = (short) (v.y >> 16);
        buf[4] = (short) v.z; buf[5] = (short) (v.z >> 16); buf[6] = (short) v.w; buf[7] = (short) (v.w >> 16);
    };

    // Pass A always starts from zero: over a run of at most 1024 samples the integrators hold plain
    // sums below 2^23 * 1024^4 / 24 < 2^59, so 64 bits are exact for every R (stored sign-extended).
    const bool short_zero_run = !PASS_B && L <= 1024;
    if (MODE == DDC_NARROW || (MODE == DDC_ALL && (log2r <= 8 || short_zero_run))) {
        // Narrow path.  The integrator inputs are m << shift, so bits [shift-1:0] of every
        // integrator stay zero, and nothing above bit 88 is ever read (integrator 5 takes
        // [88 -: 28]): for R <= 256 the live bits [88:shift] are 24 + 5 log2 R <= 64 bits, kept
        // here as (state >> shift) mod 2^64.  Same values as the 128-bit path, half the adds.
        const int sh5 = 5 * log2r - 4;                    // 61 - shift
        u64 I[4], Q[4];
        if (PASS_B) {
            const ddc_state4 a = ddc_run_start(local[lI], wgbase[wbI], (u64) (n - s0), co);
            const ddc_state4 b = ddc_run_start(local[lQ], wgbase[wbQ], (u64) (n - s0), co);
            for (int k = 0; k < 4; k++) {
                I[k] = (a.i[k].lo >> shift) | (a.i[k].hi << (64 - shift));
                Q[k] = (b.i[k].lo >> shift) | (b.i[k].hi << (64 - shift));
            }
        } else {
            for (int k = 0; k < 4; k++) I[k] = Q[k] = 0;
        }
        // Round 4, two instructions per sample and channel off each pass:
        //  pass A integrates BIASED mixer outputs, u = mix24 + 2^24 = (m + 32 + 2^30) >> 6 as an unsigned value (|m| < 2^30):
        //  no sign extension into the 64-bit adds; what a constant 2^24 leaves in the four integrators after len samples
        //  -- 2^24 x C(len + k - 1, k) -- is taken off once per run (everything is modulo 2^64 either way);
        //  pass B lets integrator 5 run on in 32 bits and masks it to 28 where it is stored (2^28 divides 2^32).
        auto step = [&](int a) {
            const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
            ph += inc16;
            if (!PASS_B) {
                const u32 ui = ((u32) (a * ec) + 0x40000020u) >> 6, uq = ((u32) (a * es) + 0x40000020u) >> 6;
                I[0] += (u64) ui; I[1] += I[0]; I[2] += I[1]; I[3] += I[2];
                Q[0] += (u64) uq; Q[1] += Q[0]; Q[2] += Q[1]; Q[3] += Q[2];
            } else {
                const long long mi = mix24(a, ec), mq = mix24(a, es);
                I[0] += (u64) mi; I[1] += I[0]; I[2] += I[1]; I[3] += I[2];
                Q[0] += (u64) mq; Q[1] += Q[0]; Q[2] += Q[1]; Q[3] += Q[2];
                i5i += (u32) (I[3] >> sh5);                           // integrator4[88 -: 28] (cic_wf1.vh), masked where stored
                i5q += (u32) (Q[3] >> sh5);
                c = (c + 1) & (u32) Rm1;
                if (c == 0) { c0i[o] = i5i & 0x0FFFFFFFu; c0q[o] = i5q & 0x0FFFFFFFu; o++; }      // strobe: sample_no was R - 1
            }
        };
        long t = s0;
        // R = 2 and R = 4 strobe four (two) times per group of eight samples: when the group is
        // aligned to the decimation counter and the output index to the store width, the strobes
        // of a group leave as ONE 16-byte (8-byte) store per component instead of scattered
        // 4-byte ones (every lane works on a different run, so each store is its own transaction:
        // at R = 2 the scalar stores made pass B 13 times slower than pass A).
        // R <= 8, pass B: every lane of a wave works on a different run, so a strobe store touches 64
        // different lines.  With staging tiles the wave collects 16 strobes per run in LDS
        // (lane rows of 17 words: conflict-free) and flushes them transposed: four lanes write
        // one run's 64 bytes, a store instruction writes 16 whole lines.  Needs the regular case:
        // a full wave of full runs aligned to the decimation, 16 | strobes per run, 16-byte
        // aligned staging rows; anything else takes the paths below.
        if (MODE == DDC_ALL && PASS_B && stage_bytes && log2r <= 3) {
            const int lane = threadIdx.x & 63, K = L >> log2r;
            const bool ok = al && c == 0 && (s1 - s0) == L && (K & (DDC_STAGE_STROBES - 1)) == 0 && (o & 3) == 0 &&
                            ((uintptr_t) c0i & 15) == 0 && ((uintptr_t) c0q & 15) == 0;
            if (__popcll(__ballot(ok)) == 64) {
                u32 *tI = stage_lds + (threadIdx.x >> 6) * (2 * 64 * DDC_STAGE_ROW), *tQ = tI + 64 * DDC_STAGE_ROW;
                // output index of the wave's first run (lane 0); lane l's run starts l * K later
                const long o_wave = ((long) __shfl((int) (o >> 32), 0) << 32) | (unsigned) __shfl((int) o, 0);
                int kcol = 0;
                long kdone = 0;                                           // strobes of this run already flushed
                auto flush = [&]() {                                      // 16 strobes of 64 runs -> 2 x 4 stores of whole lines
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    constexpr int LPR = DDC_STAGE_STROBES / 4, RPS = 64 / LPR;   // lanes per run, runs per store instruction
#pragma unroll
                    for (int q = 0; q < 64 / RPS; q++) {
                        const int rl = q * RPS + lane / LPR, col = (lane % LPR) * 4;
                        const u32 *ri = tI + rl * DDC_STAGE_ROW + col, *rq = tQ + rl * DDC_STAGE_ROW + col;
                        const uint4 vi = make_uint4(ri[0], ri[1], ri[2], ri[3]);
                        const uint4 vq = make_uint4(rq[0], rq[1], rq[2], rq[3]);
                        const long dst = o_wave + (long) rl * K + kdone + col;
                        *(uint4 *) (c0i + dst) = vi;
                        *(uint4 *) (c0q + dst) = vq;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    kdone += DDC_STAGE_STROBES;
                    kcol = 0;
                };
                // One copy of the loop per decimation: the strobe positions of a group are compile-time, so the group
                // is straight-line code -- the eight table reads go out together at its top (with a branch per sample
                // each read was waited for where it was issued: a lone wave per SIMD has nothing to hide that behind).
                // A full tile is flushed at the TOP of the next group, before that group's sample load is issued: the
                // load is then always the youngest vector-memory operation, and waiting for it does not wait for stores
                // issued a moment ago.
                auto staged_loop = [&](auto lr_tag) {
                    constexpr int LR = decltype(lr_tag)::value;
                    for (; t + 8 <= g1; t += 8) {
                        if (kcol == DDC_STAGE_STROBES) flush();           // wave-uniform
                        short buf[8];
                        samples8(t, buf);
                        int ec[8], es[8];
#pragma unroll
                        for (int w = 0; w < 8; w++) { ec[w] = KG_NCO_COS(tab, ph); es[w] = KG_NCO_SIN(tab, ph); ph += inc16; }
#pragma unroll
                        for (int w = 0; w < 8; w++) {
                            const long long mi = mix24(buf[w], ec[w]), mq = mix24(buf[w], es[w]);
                            I[0] += (u64) mi; I[1] += I[0]; I[2] += I[1]; I[3] += I[2];
                            Q[0] += (u64) mq; Q[1] += Q[0]; Q[2] += Q[1]; Q[3] += Q[2];
                            i5i += (u32) (I[3] >> sh5);
                            i5q += (u32) (Q[3] >> sh5);
                            if (((w + 1) & ((1 << LR) - 1)) == 0) {       // strobe (the group starts aligned)
                                tI[lane * DDC_STAGE_ROW + kcol + ((w + 1) >> LR) - 1] = i5i & 0x0FFFFFFFu;
                                tQ[lane * DDC_STAGE_ROW + kcol + ((w + 1) >> LR) - 1] = i5q & 0x0FFFFFFFu;
                            }
                        }
                        kcol += 8 >> LR;
                    }
                    if (kcol == DDC_STAGE_STROBES) flush();
                };
                if (log2r == 1) staged_loop(std::integral_constant<int, 1>());
                else if (log2r == 2) staged_loop(std::integral_constant<int, 2>());
                else staged_loop(std::integral_constant<int, 3>());
                o += K;                                                    // all K strobes of the run are out
            }
        }
        if (MODE == DDC_ALL && PASS_B && log2r <= 2 && c == 0 && (o & 3) == 0 && ((uintptr_t) c0i & 15) == 0 && ((uintptr_t) c0q & 15) == 0) {
            auto quiet = [&](int a) {                     // step() without the strobe store
                const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
                const long long mi = mix24(a, ec), mq = mix24(a, es);
                ph += inc16;
                I[0] += (u64) mi; I[1] += I[0]; I[2] += I[1]; I[3] += I[2];
                Q[0] += (u64) mq; Q[1] += Q[0]; Q[2] += Q[1]; Q[3] += Q[2];
                i5i += (u32) (I[3] >> sh5);
                i5q += (u32) (Q[3] >> sh5);
            };
            const u32 M28 = 0x0FFFFFFFu;
            if (log2r == 1) {
                for (; t + 8 <= g1; t += 8) {
                    short buf[8];
                    samples8(t, buf);
                    uint4 vi, vq;
                    quiet(buf[0]); quiet(buf[1]); vi.x = i5i & M28; vq.x = i5q & M28;
                    quiet(buf[2]); quiet(buf[3]); vi.y = i5i & M28; vq.y = i5q & M28;
                    quiet(buf[4]); quiet(buf[5]); vi.z = i5i & M28; vq.z = i5q & M28;
                    quiet(buf[6]); quiet(buf[7]); vi.w = i5i & M28; vq.w = i5q & M28;
                    *(uint4 *) (c0i + o) = vi; *(uint4 *) (c0q + o) = vq;
                    o += 4;
                }
            } else {
                for (; t + 8 <= g1; t += 8) {
                    short buf[8];
                    samples8(t, buf);
                    uint2 vi, vq;
                    quiet(buf[0]); quiet(buf[1]); quiet(buf[2]); quiet(buf[3]); vi.x = i5i & M28; vq.x = i5q & M28;
                    quiet(buf[4]); quiet(buf[5]); quiet(buf[6]); quiet(buf[7]); vi.y = i5i & M28; vq.y = i5q & M28;
                    *(uint2 *) (c0i + o) = vi; *(uint2 *) (c0q + o) = vq;
                    o += 2;
                }
            }
            // c is 0 again: eight is a multiple of R
        }
        for (; t + 8 <= g1; t += 8) {                     // whole groups, no per-sample masking
            short buf[8];
            samples8(t, buf);
            if (PASS_B && c + 8 <= (u32) Rm1) {
                // no strobe inside this group (most groups once R >= 16): straight-line code, the eight table
                // reads go out together (with the strobe test between them each was waited for where it was issued)
                int ec[8], es[8];
#pragma unroll
                for (int w = 0; w < 8; w++) { ec[w] = KG_NCO_COS(tab, ph); es[w] = KG_NCO_SIN(tab, ph); ph += inc16; }
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    const long long mi = mix24(buf[w], ec[w]), mq = mix24(buf[w], es[w]);
                    I[0] += (u64) mi; I[1] += I[0]; I[2] += I[1]; I[3] += I[2];
                    Q[0] += (u64) mq; Q[1] += Q[0]; Q[2] += Q[1]; Q[3] += Q[2];
                    i5i += (u32) (I[3] >> sh5);
                    i5q += (u32) (Q[3] >> sh5);
                }
                c += 8;
                continue;
            }
#pragma unroll
            for (int w = 0; w < 8; w++) step(buf[w]);
        }
        for (; t < s1; t++) step(adc[t]);                 // ragged end of the block's last run
        if (PASS_B) {
            outTi = i5i & 0x0FFFFFFFu; outTq = i5q & 0x0FFFFFFFu; have = true;
        } else {
            {   // the bias of pass A's inputs, out of the four integrators: 2^24 x C(len + k - 1, k), k = 1 .. 4, modulo 2^64
                const u64 len = (u64) (s1 - s0);          // <= 8192: len (len+1) (len+2) (len+3) < 2^53
                const u64 b1 = len, b2 = len * (len + 1) / 2, b3 = len * (len + 1) * (len + 2) / 6,
                          b4 = len * (len + 1) * (len + 2) * (len + 3) / 24;
                I[0] -= b1 << 24; I[1] -= b2 << 24; I[2] -= b3 << 24; I[3] -= b4 << 24;
                Q[0] -= b1 << 24; Q[1] -= b2 << 24; Q[2] -= b3 << 24; Q[3] -= b4 << 24;
            }
            ddc_state4 a, b;
            for (int k = 0; k < 4; k++) {
                // R <= 256: bits above 88 are never read, a logical shift will do; wider R (zero-state
                // sums): the value is signed and must be extended through bit 88
                const u64 hi_i = log2r <= 8 ? I[k] >> (64 - shift) : (u64) ((long long) I[k] >> (shift ? 64 - shift : 63));
                const u64 hi_q = log2r <= 8 ? Q[k] >> (64 - shift) : (u64) ((long long) Q[k] >> (shift ? 64 - shift : 63));
                a.i[k] = mk128(I[k] << shift, hi_i);
                b.i[k] = mk128(Q[k] << shift, hi_q);
            }
            outI = ddc_to_end(a, (u64) (n - s1), co); outQ = ddc_to_end(b, (u64) (n - s1), co); have = true;
        }
        return;
    }

    if (MODE == DDC_NARROW) return;               // (not reached: the narrow form returned above)
    if (PASS_B) {
        // Pass B, R >= 512.  Nothing above bit 88 of an integrator is ever read (integrator 5 takes [88 -: 28]), so
        // the states are kept mod 2^96 as three 32-bit limbs: an integrator step is one three-instruction carry
        // chain (v_add_co / v_addc_co / v_addc_co) where the 128-bit form took an add, a compare for the carry and
        // a second add with carry-in per half -- 89 -> 57 instructions per sample and channel, and these five of
        // the fourteen BASELINE channels were two thirds of pass B's work.
        struct u96 { u32 w[3]; };
        auto add96 = [](u96 &a, const u96 &b) {
            unsigned c0, c1;
            a.w[0] = __builtin_addc(a.w[0], b.w[0], 0u, &c0);
            a.w[1] = __builtin_addc(a.w[1], b.w[1], c0, &c1);
            a.w[2] = a.w[2] + b.w[2] + c1;
        };
        u96 I[4], Q[4];
        {
            const ddc_state4 a = ddc_run_start(local[lI], wgbase[wbI], (u64) (n - s0), co);
            const ddc_state4 b = ddc_run_start(local[lQ], wgbase[wbQ], (u64) (n - s0), co);
            for (int k = 0; k < 4; k++) {
                I[k].w[0] = (u32) a.i[k].lo; I[k].w[1] = (u32) (a.i[k].lo >> 32); I[k].w[2] = (u32) a.i[k].hi;
                Q[k].w[0] = (u32) b.i[k].lo; Q[k].w[1] = (u32) (b.i[k].lo >> 32); Q[k].w[2] = (u32) b.i[k].hi;
            }
        }
        auto step = [&](int a) {
            const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
            const long long mi = mix24(a, ec), mq = mix24(a, es);
            ph += inc16;
            // in = sign-extended m << shift (shift = 65 - 5 log2 R is 0 .. 20 here), 96 bits
            const u64 li = (u64) mi << shift, lq = (u64) mq << shift;
            u96 xi, xq;
            xi.w[0] = (u32) li; xi.w[1] = (u32) (li >> 32); xi.w[2] = (u32) (shift ? mi >> (64 - shift) : mi >> 63);
            xq.w[0] = (u32) lq; xq.w[1] = (u32) (lq >> 32); xq.w[2] = (u32) (shift ? mq >> (64 - shift) : mq >> 63);
            add96(I[0], xi); add96(I[1], I[0]); add96(I[2], I[1]); add96(I[3], I[2]);
            add96(Q[0], xq); add96(Q[1], Q[0]); add96(Q[2], Q[1]); add96(Q[3], Q[2]);
            // integrator 5 accumulates integrator4[88 -: 28] (cic_wf1.vh)
            i5i += (I[3].w[2] << 3) | (I[3].w[1] >> 29);             // (masked to 28 bits where it is stored)
            i5q += (Q[3].w[2] << 3) | (Q[3].w[1] >> 29);
            c = (c + 1) & (u32) Rm1;
            if (c == 0) { c0i[o] = i5i & 0x0FFFFFFFu; c0q[o] = i5q & 0x0FFFFFFFu; o++; }              // strobe: sample_no was R - 1
        };
        long t = s0;
        for (; t + 8 <= g1; t += 8) {
            short buf[8];
            samples8(t, buf);
            if (c + 8 <= (u32) Rm1) {                         // no strobe inside this group: see the narrow path
                int ec[8], es[8];
#pragma unroll
                for (int w = 0; w < 8; w++) { ec[w] = KG_NCO_COS(tab, ph); es[w] = KG_NCO_SIN(tab, ph); ph += inc16; }
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    const long long mi = mix24(buf[w], ec[w]), mq = mix24(buf[w], es[w]);
                    const u64 li = (u64) mi << shift, lq = (u64) mq << shift;
                    u96 xi, xq;
                    xi.w[0] = (u32) li; xi.w[1] = (u32) (li >> 32); xi.w[2] = (u32) (shift ? mi >> (64 - shift) : mi >> 63);
                    xq.w[0] = (u32) lq; xq.w[1] = (u32) (lq >> 32); xq.w[2] = (u32) (shift ? mq >> (64 - shift) : mq >> 63);
                    add96(I[0], xi); add96(I[1], I[0]); add96(I[2], I[1]); add96(I[3], I[2]);
                    add96(Q[0], xq); add96(Q[1], Q[0]); add96(Q[2], Q[1]); add96(Q[3], Q[2]);
                    i5i += (I[3].w[2] << 3) | (I[3].w[1] >> 29);
                    i5q += (Q[3].w[2] << 3) | (Q[3].w[1] >> 29);
                }
                c += 8;
                continue;
            }
#pragma unroll
            for (int w = 0; w < 8; w++) step(buf[w]);
        }
        for (; t < s1; t++) step(adc[t]);
        outTi = i5i & 0x0FFFFFFFu; outTq = i5q & 0x0FFFFFFFu; have = true;
        return;
    }
    if (MODE != DDC_ALL) return;
    // pass A of runs longer than 1024 samples at R >= 512: the zero-state sums need the full width
    ddc_state4 SI, SQ;
    if (PASS_B) {
        SI = ddc_run_start(local[lI], wgbase[wbI], (u64) (n - s0), co);
        SQ = ddc_run_start(local[lQ], wgbase[wbQ], (u64) (n - s0), co);
    } else {
        for (int k = 0; k < 4; k++) { SI.i[k] = mk128(0, 0); SQ.i[k] = mk128(0, 0); }
    }
    auto step = [&](int a) {
        const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
        const long long mi = mix24(a, ec), mq = mix24(a, es);
        ph += inc16;
        // in = sign-extended m << shift, 128 bits
        const u128 xi = mk128((u64) mi << shift, (u64) (shift ? mi >> (64 - shift) : mi >> 63));
        const u128 xq = mk128((u64) mq << shift, (u64) (shift ? mq >> (64 - shift) : mq >> 63));
        SI.i[0] = add128(SI.i[0], xi); SI.i[1] = add128(SI.i[1], SI.i[0]);
        SI.i[2] = add128(SI.i[2], SI.i[1]); SI.i[3] = add128(SI.i[3], SI.i[2]);
        SQ.i[0] = add128(SQ.i[0], xq); SQ.i[1] = add128(SQ.i[1], SQ.i[0]);
        SQ.i[2] = add128(SQ.i[2], SQ.i[1]); SQ.i[3] = add128(SQ.i[3], SQ.i[2]);
        if (PASS_B) {
            // integrator 5 accumulates integrator4[88 -: 28] (cic_wf1.vh)
            i5i = (i5i + (u32) ((SI.i[3].hi << 3) | (SI.i[3].lo >> 61))) & 0x0FFFFFFFu;
            i5q = (i5q + (u32) ((SQ.i[3].hi << 3) | (SQ.i[3].lo >> 61))) & 0x0FFFFFFFu;
            c = (c + 1) & (u32) Rm1;
            if (c == 0) { c0i[o] = i5i; c0q[o] = i5q; o++; }          // strobe: sample_no was R - 1
        }
    };
    long t = s0;
    for (; t + 8 <= g1; t += 8) {
        short buf[8];
        samples8(t, buf);
#pragma unroll
        for (int w = 0; w < 8; w++) step(buf[w]);
    }
    for (; t < s1; t++) step(adc[t]);
    if (PASS_B) {
        outTi = i5i; outTq = i5q; have = true;
    } else {
        outI = ddc_to_end(SI, (u64) (n - s1), co); outQ = ddc_to_end(SQ, (u64) (n - s1), co); have = true;
    }
}

// Round 4: the carry scan's first two levels ride on pass A.  A workgroup's 256 threads hold 256 consecutive runs of
// one channel: their end-referred results are prefix-summed right here (additions of 4 x 96 bits: a wave scan, the four wave
// totals through LDS) -- local[r] = the sum of the workgroup's runs before r, wgtot = the workgroup's total -- and what is
// left for a kernel of its own is the prefix over at most 64 workgroup totals per (channel, I/Q) (ddc_wf_scan_wg_kernel:
// one wave each, a few microseconds where the chunked scan took 36 alone and 57 .. 85 beside the bypass kernel).
template <bool PASS_B, int MODE>
__global__ __launch_bounds__(DDC_THREADS) void ddc_wf_run_kernel(
    const short *__restrict__ adc, long n, int L, int nruns,
    const ddc_chan *__restrict__ chans, const int *__restrict__ chan_list, const u32 *__restrict__ nco,
    ddc_state4 *__restrict__ local,           // [nlist][2][nruns]  A: out = the end-referred sum of the workgroup's runs before r;  B: in
    u32 *__restrict__ c0rel,
    u32 *__restrict__ tau,                    // [nlist][2][nruns]  B: out = the integrator-5 total of the workgroup's runs before r
    const long *__restrict__ c0off, const long *__restrict__ nouts, const int *__restrict__ sel, int stage_bytes,
    u64 pushed, const u64 *__restrict__ pdelta, const long *__restrict__ nlim, const int *__restrict__ reset_tab,
    const ddc_endco *__restrict__ endco, long endco_n,
    ddc_state4 *__restrict__ wgtot,           // [nlist][2][gridDim.x]  A: out = the end-referred sum of the workgroup's runs (B: null)
    const ddc_state4 *__restrict__ wgbase,    // [nlist][2][gridDim.x]  B: in = what ddc_wf_scan_wg_kernel made of wgtot: the carried-in state
                                              //                        + the workgroups before this one, end-referred (A: null)
    u32 *__restrict__ wgtau)                  // [nlist][2][gridDim.x]  B: out = the workgroup's integrator-5 total (A: null)
{
    sc4 oI = sc_zero(), oQ = sc_zero();
    bool have = false;
    u32 oTi = 0, oTq = 0;
    ddc_wf_run_body<PASS_B, MODE>(adc, n, L, nruns, chans, chan_list, nco, local, c0rel, c0off, nouts, sel, stage_bytes, pushed,
                            pdelta, nlim, reset_tab, endco, endco_n, wgbase, oI, oQ, have, oTi, oTq);
    if (PASS_B) {
        // The prefix of the runs' integrator-5 totals in the same levels: tau[r] = the sum of the workgroup's runs before r,
        // wgtau = the workgroup's total; ddc_wf_tau_wg_kernel turns the totals into each workgroup's absolute start value and
        // the combs add the two (a prefix kernel over all runs was 16 us on the step's critical path, 100 in a busy GPU).
        __shared__ u32 s_t[2][DDC_THREADS / 64];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int li = sel ? sel[blockIdx.y] : (int) blockIdx.y;
        const long r = (long) blockIdx.x * DDC_THREADS + threadIdx.x;
        u32 vi = have ? oTi : 0u, vq = have ? oTq : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 ai = __shfl_up(vi, d), aq = __shfl_up(vq, d);
            if (lane >= d) { vi += ai; vq += aq; }
        }
        if (lane == 63) { s_t[0][wave] = vi; s_t[1][wave] = vq; }
        u32 xi = __shfl_up(vi, 1), xq = __shfl_up(vq, 1);
        if (lane == 0) { xi = 0; xq = 0; }
        __syncthreads();
        u32 pi = 0, pq = 0;
        for (int w = 0; w < wave; w++) { pi += s_t[0][w]; pq += s_t[1][w]; }
        if (have) {
            tau[((long) li * 2 + 0) * nruns + r] = (pi + xi) & 0x0FFFFFFFu;
            tau[((long) li * 2 + 1) * nruns + r] = (pq + xq) & 0x0FFFFFFFu;
        }
        if (threadIdx.x == DDC_THREADS - 1) {
            wgtau[((long) li * 2 + 0) * gridDim.x + blockIdx.x] = (pi + vi) & 0x0FFFFFFFu;
            wgtau[((long) li * 2 + 1) * gridDim.x + blockIdx.x] = (pq + vq) & 0x0FFFFFFFu;
        }
    }
    if (!PASS_B) {
        __shared__ sc4 s_w[2][DDC_THREADS / 64];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int li = sel ? sel[blockIdx.y] : (int) blockIdx.y;
        const long r = (long) blockIdx.x * DDC_THREADS + threadIdx.x;
        sc4 iI = oI, iQ = oQ;
        sc_scan_add<6>(iI, lane);
        sc_scan_add<6>(iQ, lane);
        if (lane == 63) { s_w[0][wave] = iI; s_w[1][wave] = iQ; }
        __syncthreads();
        sc4 pI = sc_zero(), pQ = sc_zero();
        for (int w = 0; w < wave; w++) { pI = sc_add(pI, s_w[0][w]); pQ = sc_add(pQ, s_w[1][w]); }
        if (threadIdx.x == DDC_THREADS - 1) {                      // inclusive of the last thread: the workgroup's total
            wgtot[((long) li * 2 + 0) * gridDim.x + blockIdx.x] = state_of(sc_add(pI, iI));
            wgtot[((long) li * 2 + 1) * gridDim.x + blockIdx.x] = state_of(sc_add(pQ, iQ));
        }
        sc4 xI = sc_shfl_up(iI, 1), xQ = sc_shfl_up(iQ, 1);        // exclusive inside the wave
        if (lane == 0) { xI = sc_zero(); xQ = sc_zero(); }
        if (have) {
            local[((long) li * 2 + 0) * nruns + r] = state_of(sc_add(pI, xI));
            local[((long) li * 2 + 1) * nruns + r] = state_of(sc_add(pQ, xQ));
        }
    }
}

// The third level: one wave per (channel, I/Q) over its workgroup totals (at most 64: max_runs / 256).
__global__ __launch_bounds__(64) void ddc_wf_scan_wg_kernel(
    const ddc_state4 *__restrict__ wgtot, ddc_state4 *__restrict__ wgbase, int gx, ddc_chan *__restrict__ chans,
    const int *__restrict__ chan_list, const long *__restrict__ nlim, const int *__restrict__ reset_tab)
{
    const int pair = blockIdx.x, li = pair >> 1, comp = pair & 1, lane = threadIdx.x;
    ddc_chan *ch = chans + chan_list[li];
    if (ch->log2r == 0) return;
    const int reset_first = reset_tab[li];
    sc4 inc = lane < gx ? sc_of(wgtot[(long) pair * gx + lane]) : sc_zero();
    // the carried-in state, advanced to the end of the entry's share (lane 0; the loads above are in flight meanwhile)
    sc4 base = sc_zero();
    if (lane == 0 && !reset_first) base = sc_T((u64) nlim[li], sc_of(ch->integ[comp]));
    sc_scan_add<6>(inc, lane);
    base = sc_shfl(base, 0);
    sc4 exc = sc_shfl_up(inc, 1);
    if (lane == 0) exc = sc_zero();
    if (lane < gx) wgbase[(long) pair * gx + lane] = state_of(sc_add(base, exc));
    if (lane == 63) ch->integ[comp] = state_of(sc_add(base, inc));     // the state after the block
}

#define BYP_G 4                                // groups of four samples per thread and block: a block is BYP_G x 1024 samples
// A whole, aligned block of NB bypass channels, straight-line (the general form in the kernel spends most of its instructions
// on the ragged cases: a branch and an exec mask per group, channel and store).
template <int NB>
DDC_DEV void ddc_bypass_block(const int2 (&cur)[BYP_G], long blk, const short *tab, const u64 (&inc16)[4], const u64 (&ph0)[4],
                              short2 *const (&orow)[4])
{
#pragma unroll
    for (int g = 0; g < BYP_G; g++) {
        const long t0 = blk * (BYP_G * 1024) + g * 1024 + 4 * (long) threadIdx.x;
        const int2 v = cur[g];
        const short a[4] = {(short) v.x, (short) (v.x >> 16), (short) v.y, (short) (v.y >> 16)};
#pragma unroll
        for (int b = 0; b < NB; b++) {
            u64 ph = (ph0[b] + (u64) t0 * (inc16[b] >> 16)) << 16;    // top-aligned: wraps by itself
            int4 w0;
            int *w = (int *) &w0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
                const int mi = mix24(a[q], ec), mq = mix24(a[q], es);
                w[q] = (int) (((u32) (mi >> 8) & 0xffffu) | ((u32) (mq >> 8) << 16));      // short2 {i, q}
                ph += inc16[b];
            }
            *(int4 *) (orow[b] + t0) = w0;
        }
    }
}
// The whole blocks of a pass, in a loop of their own: the next block's loads, this block's arithmetic, its stores -- nothing
// conditional, so the wait in front of the arithmetic counts exactly the operations issued since this block's loads.
template <int NB>
DDC_DEV long ddc_bypass_whole(const short *__restrict__ adc, long blk, long nfb, const short *tab, const u64 (&inc16)[4],
                              const u64 (&ph0)[4], short2 *const (&orow)[4])
{
    auto fetch = [&](long bk, int2 (&v)[BYP_G]) {
#pragma unroll
        for (int g = 0; g < BYP_G; g++) v[g] = *(const int2 *) (adc + bk * (BYP_G * 1024) + g * 1024 + 4 * (long) threadIdx.x);
    };
    if (blk >= nfb) return blk;
    int2 cur[BYP_G], nxt[BYP_G];
    fetch(blk, cur);
    for (; blk < nfb; blk += gridDim.x) {
        fetch(blk + gridDim.x < nfb ? blk + gridDim.x : blk, nxt);
        // (opaque: a phase accumulator and a row address per group and channel, carried from block to block by the
        // compiler's strength reduction, were 216 registers and two waves per SIMD)
        long bo = blk;
        asm volatile("" : "+s"(bo));
        ddc_bypass_block<NB>(cur, bo, tab, inc16, ph0, orow);
#pragma unroll
        for (int g = 0; g < BYP_G; g++) cur[g] = nxt[g];
    }
    return blk;
}

// The same whole blocks when the caller's rows (or the sample stream) are NOT 16-byte (8-byte) aligned -- `out_stride = n + 1`
// is enough: four single-dword stores per lane and channel at a 16-byte pitch then took the place of one 16-byte store
// (86 us instead of 36 for 2^24 samples x 2 channels; tools/micro/bypass_rate.hip).  Transposed lane mapping instead: lane l of
// wave w takes samples 256 w + 64 q + l (q = 0 .. 3) of a 1024-sample group, so every load instruction reads 128 contiguous
// bytes and every store instruction writes 256, whatever the alignment.
template <int NB>
DDC_DEV long ddc_bypass_whole_t(const short *__restrict__ adc, long blk, long nfb, const short *tab, const u64 (&inc16)[4],
                                const u64 (&ph0)[4], short2 *const (&orow)[4])
{
    const long lo = 256 * (long) (threadIdx.x >> 6) + (threadIdx.x & 63);       // this lane's first sample inside a group
    auto fetch = [&](long bk, short (&v)[BYP_G][4]) {
#pragma unroll
        for (int g = 0; g < BYP_G; g++)
#pragma unroll
            for (int q = 0; q < 4; q++) v[g][q] = adc[bk * (BYP_G * 1024) + g * 1024 + lo + 64 * q];
    };
    if (blk >= nfb) return blk;
    short cur[BYP_G][4], nxt[BYP_G][4];
    fetch(blk, cur);
    for (; blk < nfb; blk += gridDim.x) {
        fetch(blk + gridDim.x < nfb ? blk + gridDim.x : blk, nxt);
        long bo = blk;
        asm volatile("" : "+s"(bo));
#pragma unroll
        for (int g = 0; g < BYP_G; g++) {
            const long t0 = bo * (BYP_G * 1024) + g * 1024 + lo;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                u64 ph = (ph0[b] + (u64) t0 * (inc16[b] >> 16)) << 16;    // top-aligned: wraps by itself
                const u64 step = inc16[b] << 6;                           // 64 samples on
                int *o = (int *) (orow[b] + t0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
                    const int mi = mix24(cur[g][q], ec), mq = mix24(cur[g][q], es);
                    o[64 * q] = (int) (((u32) (mi >> 8) & 0xffffu) | ((u32) (mq >> 8) << 16));      // short2 {i, q}
                    ph += step;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < BYP_G; g++)
#pragma unroll
            for (int q = 0; q < 4; q++) cur[g][q] = nxt[g][q];
    }
    return blk;
}

// R == 1 bypass (cic_prune_var.v:289-297): out = mixer output [23 -: 16], no filter state at all,
// so it is sample-parallel: lane-contiguous groups of four samples per thread.
__global__ __launch_bounds__(256, 4) void ddc_wf_bypass_kernel(
    const short *__restrict__ adc, long n, const ddc_chan *__restrict__ chans, const int *__restrict__ chan_list,
    const int *__restrict__ bypass_list, int nbypass,     // list entries with R == 1
    const u32 *__restrict__ nco, short2 *__restrict__ out, long out_stride, u64 pushed, const u64 *__restrict__ pdelta,
    const long *__restrict__ nlim,            // [nlist] samples this entry takes (capture: max_out; else n)
    const long *__restrict__ out_off,         // [nlist] entry li writes at out + li out_stride + out_off[li]
    int by_chan)                              // ... or at row chan_list[li] (kg_ctx::rows_by_chan)
{
    __shared__ short tab[DDC_TAB];
    for (int i = threadIdx.x; i < DDC_TAB / 2; i += 256) ((u32 *) tab)[i] = nco[i];
    __syncthreads();
    // Persistent over the blocks of the stream: the 20 KiB table is staged once per workgroup.  Round 4: ONE pass over the ADC
    // samples for ALL bypass channels (up to four at a time; the channels' parameters are read once, into scalar registers),
    // and the kernel was LATENCY-bound on its own reads: one 8-byte load per lane, waited for where it was issued, 8 KiB in
    // flight per CU -- 33 MB took 48 us of the kernel's 86 (knock-out builds: no stores 69 us, no table reads 83, loads alone
    // 8.6).  Now a thread has eight loads in flight (this block's four groups and the next block's) and the whole blocks
    // run in a straight-line loop (ddc_bypass_whole).
    const long bs = BYP_G * 1024;
    const long nblk = (n + bs - 1) / bs;
    const bool al8 = (((uintptr_t) adc) & 7) == 0;
    for (int b0 = 0; b0 < nbypass; b0 += 4) {
        const int nb4 = nbypass - b0 < 4 ? nbypass - b0 : 4;
        u64 inc16[4], ph0[4]; long nbs[4]; short2 *orow[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int li = bypass_list[b0 + (b < nb4 ? b : 0)];
            const ddc_chan *ch = chans + chan_list[li];
            inc16[b] = ch->phase_inc << 16;
            ph0[b] = ch->phase + (pushed + pdelta[li]) * ch->phase_inc;
            nbs[b] = b < nb4 ? nlim[li] : 0;
            orow[b] = out + (long) (by_chan ? chan_list[li] : li) * out_stride + out_off[li];
        }
        // samples up to which every channel of the four takes whole aligned blocks, rows that take 16-byte stores
        long nfull = n;
        bool rows16 = true;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (b < nb4) { nfull = nbs[b] < nfull ? nbs[b] : nfull; rows16 = rows16 && (((uintptr_t) orow[b]) & 15) == 0; }
        const long nany = nfull;                   // samples up to which every channel of the four takes whole blocks
        long blk = blockIdx.x;
        if (rows16 && al8) {
            const long nfb = nfull / bs;
            switch (nb4) {
            case 1: blk = ddc_bypass_whole<1>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            case 2: blk = ddc_bypass_whole<2>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            case 3: blk = ddc_bypass_whole<3>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            default: blk = ddc_bypass_whole<4>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            }
        } else {
            const long nfb = nany / bs;
            switch (nb4) {
            case 1: blk = ddc_bypass_whole_t<1>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            case 2: blk = ddc_bypass_whole_t<2>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            case 3: blk = ddc_bypass_whole_t<3>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            default: blk = ddc_bypass_whole_t<4>(adc, blk, nfb, tab, inc16, ph0, orow); break;
            }
        }
        // what is left: the ragged end of the stream, entries that take less than the block (a capture), unaligned rows
        for (; blk < nblk; blk += gridDim.x) {
            for (int g = 0; g < BYP_G; g++) {
                const long t0 = blk * bs + g * 1024 + 4 * (long) threadIdx.x;
                if (t0 >= n) continue;
                short a[4];
                const bool full = t0 + 4 <= n;
                if (full && al8) {
                    const int2 v = *(const int2 *) (adc + t0);
                    a[0] = (short) v.x; a[1] = (short) (v.x >> 16); a[2] = (short) v.y; a[3] = (short) (v.y >> 16);
                } else {
                    for (int q = 0; q < 4; q++) a[q] = (t0 + q < n) ? adc[t0 + q] : (short) 0;
                }
                for (int b = 0; b < nb4; b++) {
                    const long nb = nbs[b];
                    if (t0 >= nb) continue;
                    const bool fullb = t0 + 4 <= nb;
                    u64 ph = (ph0[b] + (u64) t0 * (inc16[b] >> 16)) << 16;    // top-aligned: wraps by itself
                    short2 *o = orow[b] + t0;
                    short2 r[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int ec = KG_NCO_COS(tab, ph), es = KG_NCO_SIN(tab, ph);
                        const int mi = mix24(a[q], ec), mq = mix24(a[q], es);
                        r[q] = make_short2((short) (mi >> 8), (short) (mq >> 8));
                        ph += inc16[b];
                    }
                    if (fullb && (((uintptr_t) o) & 15) == 0) {
                        int4 w0;
                        w0.x = *(int *) &r[0]; w0.y = *(int *) &r[1]; w0.z = *(int *) &r[2]; w0.w = *(int *) &r[3];
                        *(int4 *) o = w0;
                    } else {
                        for (int q = 0; q < 4; q++) if (t0 + q < nb) o[q] = r[q];
                    }
                }
            }
        }
    }
}

// ... and of the integrator-5 totals: in = the workgroups' totals, out = integrator 5 at each workgroup's first run.
__global__ __launch_bounds__(64) void ddc_wf_tau_wg_kernel(u32 *__restrict__ wgtau, int gx, ddc_chan *__restrict__ chans,
                                                          const int *__restrict__ chan_list, const int *__restrict__ reset_tab)
{
    const int pair = blockIdx.x, li = pair >> 1, comp = pair & 1, lane = threadIdx.x;
    ddc_chan *ch = chans + chan_list[li];
    if (ch->log2r == 0) return;
    const int reset_first = reset_tab[li];
    u32 v = lane < gx ? wgtau[(long) pair * gx + lane] : 0u;
    const u32 i5 = reset_first ? 0u : ch->integ5[comp];
    for (int d = 1; d < 64; d <<= 1) { const u32 a = __shfl_up(v, d); if (lane >= d) v += a; }
    u32 x = __shfl_up(v, 1);
    if (lane == 0) x = 0;
    if (lane < gx) wgtau[(long) pair * gx + lane] = (i5 + x) & 0x0FFFFFFFu;
    if (lane == 63) ch->integ5[comp] = (i5 + v) & 0x0FFFFFFFu;       // the state after the call
}

// sign-extend the low `bits` bits
DDC_DEV int sext32(int v, int bits) { return (v << (32 - bits)) >> (32 - bits); }

// Combs + rounding, four consecutive outputs per thread.  cic_wf1.vh: comb widths
// 23,22,21,20,20; their inputs drop 5,1,1,1,0 LSBs; out = comb5[19 -: 16] + comb5[3].
// Channels decimate differently, so the grid is flat: workgroup w belongs to the list entry
// li with wg_start[li] <= w < wg_start[li + 1] (bypass channels own none).  A workgroup first
// puts the absolute integrator-5 values of its 1024 outputs and the five before them in LDS
// (16-byte loads of the run-relative values: the I and Q planes of a channel start 16-byte aligned),
// then every thread runs the five combs over a nine-value window: 30 differences for four outputs
// where one output per thread took 15 each, and a quarter of the load and store instructions.
#define DDC_COMB_TILE 1024
__global__ __launch_bounds__(256) void ddc_wf_comb_kernel(
    const u32 *__restrict__ c0rel, const u32 *__restrict__ i5start, int log2L, int nruns,
    const long *__restrict__ c0off, const ddc_chan *__restrict__ chans, const int *__restrict__ chan_list, const long *__restrict__ nouts,
    u64 pushed, const u64 *__restrict__ pdelta,   // samples pushed since the entry's reference point: pushed + pdelta[li]
    const int *__restrict__ reset_tab,        // [nlist] capture: counter and comb registers start the block at zero
    const int *__restrict__ wg_start, int nlist,
    short2 *__restrict__ out, long out_stride, const long *__restrict__ out_off,   // entry li writes at out + li out_stride + out_off[li]
    u32 *__restrict__ hist_out,               // [nlist][2][5]
    const u32 *__restrict__ wgtau, int gx,    // end-referred levels: i5start[] is relative to its run pass workgroup's start value wgtau[li][comp][run / 256]
    int by_chan)                              // rows of `out` by channel number (kg_ctx::rows_by_chan)
{
    __shared__ __attribute__((aligned(16))) int s_c0[2][DDC_COMB_TILE + 8];       // [d]: output o0 - 8 + d (three unused slots keep 16-byte rows)
    int lo = 0, hi = nlist;                   // wg_start[lo] <= blockIdx.x < wg_start[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int) blockIdx.x >= wg_start[mid]) lo = mid; else hi = mid; }
    const int li = lo, t = threadIdx.x;
    const ddc_chan *ch = chans + chan_list[li];
    const int log2r = ch->log2r;
    const int reset_first = reset_tab[li];
    const long nout = nouts[li], plane = (nout + 3) & ~3l;
    const long o0 = (long) (blockIdx.x - wg_start[li]) * DDC_COMB_TILE;
    const u32 base = reset_first ? 0u : (u32) (((u64) ch->sample_no + pushed + pdelta[li]) & ((1ull << log2r) - 1));     // sample_no before this call
    auto absolute = [&](int comp, long oo, u32 rel) -> u32 {
        const long g = ((oo + 1) << log2r) - 1 - (long) base;    // sample index of the strobe
        const int run = (int) (g >> log2L);
        const u32 wb = wgtau[((long) li * 2 + comp) * gx + (run >> 8)];
        return (rel + i5start[((long) li * 2 + comp) * nruns + run] + wb) & 0x0FFFFFFFu;
    };
#pragma unroll
    for (int comp = 0; comp < 2; comp++) {
        const u32 *src = c0rel + c0off[li] + comp * plane;
        // the four outputs of this thread
        const long oo = o0 + 4 * t;
        u32 v[4] = {0, 0, 0, 0};
        if (oo + 4 <= nout) {
            const uint4 q = *(const uint4 *) (src + oo);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int k = 0; k < 4; k++) if (oo + k < nout) v[k] = src[oo + k];
        }
        int4 w4;                              // one 16-byte LDS store per thread (four 4-byte ones: stride-4 words, 4-way conflicts)
        int *w4p = (int *) &w4;
        for (int k = 0; k < 4; k++) {
            u32 a = 0;
            if (oo + k < nout) {
                a = absolute(comp, oo + k, v[k]);
                if (oo + k >= nout - 5) hist_out[((long) li * 2 + comp) * 5 + (int) (oo + k - (nout - 5))] = a;
            }
            w4p[k] = sext32((int) a, 28);
        }
        *(int4 *) &s_c0[comp][8 + 4 * t] = w4;
        // the five outputs before the tile: strobes of earlier calls (zero after a reset) or earlier tiles
        if (t < 5) {
            const long pb = o0 - 5 + t;
            const u32 a = pb < 0 ? (reset_first ? 0u : ch->hist[comp][5 + pb]) : absolute(comp, pb, src[pb]);
            s_c0[comp][3 + t] = sext32((int) a, 28);
        }
    }
    __syncthreads();
    const long o = o0 + 4 * t;
    short res[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (o < nout) {
        for (int comp = 0; comp < 2; comp++) {
            // comb k output at position d needs its input at d and d-1
            const int W[5] = {23, 22, 21, 20, 20}, D[5] = {5, 1, 1, 1, 0};
            int v[9];
            {                                 // the nine-value window [3 + 4t, 12 + 4t) from three 16-byte reads of [4t, 4t + 12)
                const int4 q0 = *(const int4 *) &s_c0[comp][4 * t], q1 = *(const int4 *) &s_c0[comp][4 * t + 4],
                           q2 = *(const int4 *) &s_c0[comp][4 * t + 8];
                v[0] = q0.w; v[1] = q1.x; v[2] = q1.y; v[3] = q1.z; v[4] = q1.w; v[5] = q2.x; v[6] = q2.y; v[7] = q2.z; v[8] = q2.w;
            }
            int cnt = 9;
            for (int k = 0; k < 5; k++) {
                int x[9];
                for (int d = 0; d < cnt; d++) x[d] = sext32(v[d] >> D[k], W[k]);
                for (int d = 1; d < cnt; d++) v[d - 1] = sext32(x[d] - x[d - 1], W[k]);
                cnt--;
            }
            for (int k = 0; k < 4; k++) res[comp][k] = (short) ((v[k] >> 4) + ((v[k] >> 3) & 1));
        }
    }
    // out through LDS, so that the stores are lane-contiguous whatever the alignment of the caller's rows
    __syncthreads();                          // every thread has read its window
    int *s_out = &s_c0[0][0];
    {
        int4 o4;
        int *o4p = (int *) &o4;
        for (int k = 0; k < 4; k++) o4p[k] = (int) ((unsigned short) res[0][k] | ((unsigned) (unsigned short) res[1][k] << 16));
        *(int4 *) &s_out[4 * t] = o4;
    }
    __syncthreads();
    short2 *dst = out + (long) (by_chan ? chan_list[li] : li) * out_stride + out_off[li] + o0;
    for (int k = 0; k < 4; k++) {
        const int e = t + 256 * k;
        if (o0 + e < nout) { const int w = s_out[e]; dst[e] = make_short2((short) (w & 0xffff), (short) (w >> 16)); }
    }
}

// after a call: the comb history (phase and counter are reference values + the host's `pushed`, see ddc_chan)
__global__ void ddc_wf_finish_kernel(ddc_chan *__restrict__ chans, const int *__restrict__ chan_list, int nlist,
                                     long n, const long *__restrict__ nouts, const u32 *__restrict__ hist_new,
                                     const int *__restrict__ reset_tab)
{
    const int li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= nlist) return;
    const int reset_first = reset_tab[li];
    ddc_chan *ch = chans + chan_list[li];
    if (ch->log2r == 0) return;
    const long nout = nouts[li];
    if (nout <= 0) return;
    for (int comp = 0; comp < 2; comp++) {
        u32 h[5];
        for (int d = 0; d < 5; d++) {
            // the last five strobes: fewer than five new ones keep part of the old history
            const long back = 4 - d;             // 0 = most recent
            if (back < nout) h[d] = hist_new[((long) li * 2 + comp) * 5 + d];
            else h[d] = reset_first ? 0u : ch->hist[comp][d + nout];
        }
        for (int d = 0; d < 5; d++) ch->hist[comp][d] = h[d];
    }
}

// ---------------------------------------------------------------------------
struct kg_ddc {
    kg_ctx *ctx;
    int nchan;
    long max_samples;
    kg_dbuf<ddc_chan> d_chans;
    std::vector<ddc_chan> h_chans;            // host mirror of the scalar fields
    kg_dbuf<u32> d_nco;
    // Buffers a push's run passes fill and its output stage (run-total prefix, combs, finish) drains: TWO sets, used in
    // turn, so that push k + 1's run passes may overwrite nothing push k's output stage still reads (deferred mode).
    kg_dbuf<ddc_state4> d_local[2]; kg_dbuf<u32> d_c0rel[2], d_tau[2], d_hist;
    int max_runs; long c0_cap[2];
    hipStream_t side; hipEvent_t ev_fork, ev_join;                   // pass B of the small decimations beside the rest
    bool side_borrowed;                                              // `side` is the owner's (a receiver bank's): not destroyed here
    kg_stage_cache pack_cache;                 // the per-call tables of the last push (a steady stream repeats them: no upload)
    std::vector<u64> h_pushed;                 // per channel: samples pushed since its reference point (ddc_chan.phase / .sample_no)
    std::vector<char> h_stale;                 // per channel: a capture cut its filters short; the next continuous push resets it
    std::vector<char> seen;                    // scratch of a push: channels listed so far
    // Deferred output stage (kg_ddc_wf_set_deferred): the stage runs on `tail`, the context's stream carries only pass A,
    // the state scan and pass B, so the NEXT push's pass A starts while this push's combs are still writing.
    bool deferred;
    hipStream_t tail;
    hipEvent_t ev_runs, ev_tail[2];            // run passes of the push done (main stream) / output stage of the push of that parity done
    hipEvent_t ev_adc;                         // deferred mode: behind the output stream's last reader of the caller's samples (the bypass kernel)
    bool tail_rec[2];                          // ev_tail[p] has been recorded
    bool tail_unjoined;                        // the context's stream has not yet been made to wait for the last output stage
    int parity;                                // buffer set of the NEXT push
    void *after_ev;                            // kg_ddc_wf_tail_after: the next push's writers of the caller's rows wait for it
    kg_dbuf<ddc_endco> d_endco; long endco_n; int endco_L, endco_runs;      // end-distance coefficients of the last (n, L, nruns)
    kg_dbuf<ddc_state4> d_wgtot[2], d_wgbase[2];   // [nchan][2][DDC_MAX_GX] per buffer set: pass A's workgroup totals, pass B's workgroup bases
    kg_dbuf<u32> d_wgtau[2];                   // likewise: the integrator-5 totals of pass B's workgroups, then their start values
};

static_assert(DDC_PLAN_THREADS == DDC_THREADS && DDC_PLAN_COMB_TILE == DDC_COMB_TILE && DDC_PLAN_BYPASS_BLOCK == BYP_G * 1024 &&
              DDC_PLAN_ALL == DDC_ALL && DDC_PLAN_NARROW == DDC_NARROW && DDC_PLAN_WIDE == DDC_WIDE, "kg_ddc_plan.h plans for these kernels");
static const int DDC_MAX_GX = DDC_TARGET_RUNS * 2 / DDC_THREADS;      // workgroups of a run pass per channel: one lane each in ddc_wf_scan_wg_kernel
static_assert(DDC_MAX_GX <= 64, "ddc_wf_scan_wg_kernel scans one workgroup total per lane");
static_assert(DDC_THREADS == 256, "ddc_wf_comb_kernel finds a run's pass-B workgroup as run >> 8");
// The distances the end-referred states are advanced by are at most one push's share of samples, max_runs x DDC_RUN_MAX.
static_assert((unsigned long long) DDC_TARGET_RUNS * 2 * DDC_RUN_MAX < (1ull << 32),
              "sc_coef.c2 and sc_Tinv's c2 are 64 bits wide: an advance of 2^32 samples or more needs a u96 there");

// The object's second stream, handed over by an owner that lays out its streams itself (kg_rxbank.hip: which hardware queue
// a stream lands on follows from the order streams are created in).  Before the first push.  Not part of the ABI.
int kg_ddc_use_side_stream(kg_ddc *d, hipStream_t s)
{
    KG_REQUIRE(d && s && !d->side, KG_ERR_STATE, "kg_ddc_use_side_stream: the object already has a second stream");
    KG_HIP(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
    KG_HIP(hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming));
    d->side = s; d->side_borrowed = true;
    return KG_OK;
}

static int ddc_init(kg_ddc *d)
{
    const int nchan = d->nchan;
    const size_t max_samples = (size_t) d->max_samples;
    d->h_chans.assign(nchan, ddc_chan());
    for (auto &c : d->h_chans) memset(&c, 0, sizeof c);
    d->max_runs = (int) ((max_samples + DDC_RUN_MIN - 1) / DDC_RUN_MIN);
    if (d->max_runs > DDC_TARGET_RUNS * 2) d->max_runs = DDC_TARGET_RUNS * 2;
    d->c0_cap[0] = d->c0_cap[1] = 0;
    d->h_pushed.assign(nchan, 0);
    d->h_stale.assign(nchan, 0);
    d->deferred = false; d->tail = nullptr; d->tail_rec[0] = d->tail_rec[1] = false; d->tail_unjoined = false;
    d->parity = 0; d->after_ev = nullptr;
    KG_TRY(d->d_chans.alloc(nchan, "kg_ddc_create: channels"));
    KG_HIP(hipMemset(d->d_chans, 0, sizeof(ddc_chan) * nchan));
    KG_TRY(d->d_nco.alloc(sizeof(short) * DDC_TAB / sizeof(u32), "kg_ddc_create: NCO table"));
    KG_HIP(hipFuncSetAttribute((const void *) ddc_wf_run_kernel<true, DDC_ALL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               DDC_STAGE_BYTES));
    for (int p = 0; p < 2; p++) {
        KG_TRY(d->d_local[p].alloc(2 * (size_t) nchan * d->max_runs, "kg_ddc_create: run states"));
        KG_TRY(d->d_tau[p].alloc(2 * (size_t) nchan * d->max_runs, "kg_ddc_create: run totals"));
    }
    KG_TRY(d->d_hist.alloc(10 * (size_t) nchan, "kg_ddc_create: histories"));
    KG_TRY(d->d_endco.alloc((size_t) d->max_runs + 1, "kg_ddc_create: end coefficients"));
    for (int p = 0; p < 2; p++) {
        KG_TRY(d->d_wgtot[p].alloc(2 * (size_t) nchan * DDC_MAX_GX, "kg_ddc_create: workgroup totals"));
        KG_TRY(d->d_wgbase[p].alloc(2 * (size_t) nchan * DDC_MAX_GX, "kg_ddc_create: workgroup bases"));
        KG_TRY(d->d_wgtau[p].alloc(2 * (size_t) nchan * DDC_MAX_GX, "kg_ddc_create: workgroup totals"));
    }
    d->endco_n = -1; d->endco_L = 0; d->endco_runs = 0;
    // NCO table: ONE 16-bit sine table, sin(a) = T[a], cos(a) = T[a + 2048] (kg_common.h, kg_nco_table_build)
    std::vector<short> tab(DDC_TAB);
    kg_nco_table_build(tab.data());
    KG_HIP(hipMemcpy(d->d_nco, tab.data(), sizeof(short) * DDC_TAB, hipMemcpyHostToDevice));
    return KG_OK;
}

extern "C" {

int kg_ddc_create(kg_ctx *ctx, int nchan, size_t max_samples, kg_ddc **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_ddc_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= 4096, KG_ERR_INVALID, "kg_ddc_create: nchan %d", nchan);
    KG_REQUIRE(max_samples >= 64 && max_samples <= ((size_t) 1 << 32), KG_ERR_INVALID,
               "kg_ddc_create: max_samples %zu", max_samples);
    kg_ddc *d = new (std::nothrow) kg_ddc();
    KG_REQUIRE(d != nullptr, KG_ERR_NOMEM, "kg_ddc_create: alloc");
    d->ctx = ctx; d->nchan = nchan; d->max_samples = (long) max_samples;
    rc = ddc_init(d);
    if (rc) { kg_ddc_destroy(d); return rc; }
    *out = d;
    return KG_OK;
}


void kg_ddc_destroy(kg_ddc *d)
{
    if (!d) return;
    (void) hipSetDevice(d->ctx->device);
    (void) hipStreamSynchronize(d->ctx->stream);
    if (d->side) (void) hipStreamSynchronize(d->side);
    if (d->tail) (void) hipStreamSynchronize(d->tail);
    for (hipEvent_t e : {d->ev_fork, d->ev_join, d->ev_runs, d->ev_tail[0], d->ev_tail[1], d->ev_adc})
        if (e) (void) hipEventDestroy(e);
    if (d->side && !d->side_borrowed) kg_stream_put(d->ctx->device, d->side);
    kg_stream_put(d->ctx->device, d->tail);       // null passes
    delete d;
}

// Everything the object has in flight, on all of its streams.
static int ddc_sync_all(kg_ddc *d)
{
    KG_HIP(hipStreamSynchronize(d->ctx->stream));
    if (d->side) KG_HIP(hipStreamSynchronize(d->side));
    if (d->tail) KG_HIP(hipStreamSynchronize(d->tail));
    d->tail_unjoined = false;
    return KG_OK;
}

static inline u64 ddc_cur_phase(const kg_ddc *d, int ch)
{
    const ddc_chan &c = d->h_chans[ch];
    return (c.phase + d->h_pushed[ch] * c.phase_inc) & ((1ull << 48) - 1);
}
static inline u32 ddc_cur_cnt(const kg_ddc *d, int ch)
{
    const ddc_chan &c = d->h_chans[ch];
    return (u32) (((u64) c.sample_no + d->h_pushed[ch]) & ((1ull << c.log2r) - 1));
}

// The host copy of the scalar fields -> the device record (the filter state the host copy holds with it: zero after
// set_wf / reset).  Drains the object first.
static int ddc_upload(kg_ddc *d, int ch)
{
    int rc = ddc_sync_all(d);
    if (rc) return rc;
    KG_HIP(hipMemcpy(d->d_chans + ch, &d->h_chans[ch], sizeof(ddc_chan), hipMemcpyHostToDevice));
    return KG_OK;
}

// Move channel ch's reference point to "now" (phase and counter as they stand, pushed = 0) WITHOUT touching its filter
// state: only the two scalar fields go to the device.  Drains the object first.
static int ddc_rebase(kg_ddc *d, int ch)
{
    if (d->h_pushed[ch] == 0) return KG_OK;
    int rc = ddc_sync_all(d);
    if (rc) return rc;
    ddc_chan &c = d->h_chans[ch];
    c.phase = ddc_cur_phase(d, ch);
    c.sample_no = ddc_cur_cnt(d, ch);
    d->h_pushed[ch] = 0;
    KG_HIP(hipMemcpy(&d->d_chans[ch].phase, &c.phase, sizeof c.phase, hipMemcpyHostToDevice));
    KG_HIP(hipMemcpy(&d->d_chans[ch].sample_no, &c.sample_no, sizeof c.sample_no, hipMemcpyHostToDevice));
    return KG_OK;
}

int kg_ddc_set_wf(kg_ddc *d, int ch, uint64_t phase_inc, int decim)
{
    KG_REQUIRE(d != nullptr, KG_ERR_INVALID, "kg_ddc_set_wf: null argument");
    int rc = kg_ctx_use(d->ctx);
    if (rc) return rc;
    KG_REQUIRE(ch >= 0 && ch < d->nchan, KG_ERR_INVALID, "kg_ddc_set_wf: channel %d (0..%d)", ch, d->nchan - 1);
    int log2r = -1;
    for (int k = 0; k <= 13; k++) if (decim == (1 << k)) log2r = k;
    KG_REQUIRE(log2r >= 0, KG_ERR_INVALID, "kg_ddc_set_wf: decimation %d is not 1, 2, 4 .. 8192", decim);
    // changing the rate or frequency resets the sampler, as sample_wf() does (CmdWFReset, :1005)
    ddc_chan &c = d->h_chans[ch];
    memset(&c, 0, sizeof c);
    c.phase_inc = phase_inc & ((1ull << 48) - 1);
    c.log2r = log2r;
    c.active = 1;
    d->h_pushed[ch] = 0;
    d->h_stale[ch] = 0;
    return ddc_upload(d, ch);
}

int kg_ddc_reset_wf(kg_ddc *d, int ch)
{
    KG_REQUIRE(d != nullptr, KG_ERR_INVALID, "kg_ddc_reset_wf: null argument");
    int rc = kg_ctx_use(d->ctx);
    if (rc) return rc;
    KG_REQUIRE(ch >= 0 && ch < d->nchan && d->h_chans[ch].active, KG_ERR_INVALID,
               "kg_ddc_reset_wf: channel %d is not configured", ch);
    // rst_wf_samp_wr (waterfall_1cic.v:47): CIC registers and the decimation counter; the NCO
    // phase keeps running in the FPGA: reference phase + what has been pushed since
    ddc_chan &c = d->h_chans[ch];
    const u64 inc = c.phase_inc, ph = ddc_cur_phase(d, ch); const int l2 = c.log2r;
    memset(&c, 0, sizeof c);
    c.phase = ph; c.phase_inc = inc; c.log2r = l2; c.active = 1;
    d->h_pushed[ch] = 0;
    d->h_stale[ch] = 0;
    return ddc_upload(d, ch);
}

int kg_ddc_set_phase(kg_ddc *d, int ch, uint64_t phase)
{
    KG_REQUIRE(d != nullptr && ch >= 0 && ch < d->nchan && d->h_chans[ch].active, KG_ERR_INVALID,
               "kg_ddc_set_phase: channel %d is not configured", ch);
    int rc = kg_ctx_use(d->ctx);
    if (rc) return rc;
    if ((rc = ddc_rebase(d, ch))) return rc;            // the counter's reference moves to "now" with the phase's
    if ((rc = ddc_sync_all(d))) return rc;
    ddc_chan &c = d->h_chans[ch];
    c.phase = phase & ((1ull << 48) - 1);
    KG_HIP(hipMemcpy(&d->d_chans[ch].phase, &c.phase, sizeof c.phase, hipMemcpyHostToDevice));
    return KG_OK;
}

// Number of IQ pairs channel ch will produce for the next n samples.
long kg_ddc_wf_outputs(kg_ddc *d, int ch, size_t n)
{
    if (!d || ch < 0 || ch >= d->nchan || !d->h_chans[ch].active) return KG_ERR_INVALID;
    // a channel a capture left behind is reset by its next continuous push: the counter starts that block at zero
    if (d->h_stale[ch]) return (long) ((u64) n >> d->h_chans[ch].log2r);
    return (long) (((u64) ddc_cur_cnt(d, ch) + (u64) n) >> d->h_chans[ch].log2r);
}

// Deferred output stage.  Off (the default): kg_ddc_wf_push_dev leaves everything it enqueues ordered on the context's
// stream -- the caller's next enqueue on that stream sees the outputs.  On: the push returns with its output stage
// (R = 1 bypass channels, run-total prefix, combs) on a stream of the object; the context's stream carries only pass A,
// the state scan and pass B, so that the NEXT push's run passes start while this push's combs are still writing.  Whoever
// consumes the outputs first makes ITS stream wait for them with kg_ddc_wf_join (null: the context's stream).
int kg_ddc_wf_set_deferred(kg_ddc *d, int on)
{
    KG_REQUIRE(d != nullptr, KG_ERR_INVALID, "kg_ddc_wf_set_deferred: null argument");
    int rc = kg_ctx_use(d->ctx);
    if (rc) return rc;
    if ((rc = ddc_sync_all(d))) return rc;
    if (on && !d->tail) {
        if ((rc = kg_stream_get(d->ctx->device, &d->tail))) return rc;
        KG_HIP(hipEventCreateWithFlags(&d->ev_runs, hipEventDisableTiming));
        KG_HIP(hipEventCreateWithFlags(&d->ev_tail[0], hipEventDisableTiming));
        KG_HIP(hipEventCreateWithFlags(&d->ev_tail[1], hipEventDisableTiming));
        KG_HIP(hipEventCreateWithFlags(&d->ev_adc, hipEventDisableTiming));
    }
    d->deferred = on != 0;
    return KG_OK;
}

int kg_ddc_wf_join(kg_ddc *d, void *stream)
{
    KG_REQUIRE(d != nullptr, KG_ERR_INVALID, "kg_ddc_wf_join: null argument");
    int rc = kg_ctx_use(d->ctx);
    if (rc) return rc;
    const int last = d->parity ^ 1;                     // buffer set of the last push
    if (!d->tail || !d->tail_rec[last]) return KG_OK;   // nothing deferred is outstanding
    hipStream_t st = stream ? (hipStream_t) stream : d->ctx->stream;
    KG_HIP(hipStreamWaitEvent(st, d->ev_tail[last], 0));
    if (st == d->ctx->stream) d->tail_unjoined = false;
    return KG_OK;
}

// The NEXT push's writers of the caller's output rows (bypass kernel, combs) will not start before `event` (a
// hipEvent_t recorded by the caller behind its last reader of those rows): the write-after-read edge of a caller that
// reads push k's rows on its own stream while push k + 1 is already running.  Consumed by that push.
int kg_ddc_wf_tail_after(kg_ddc *d, void *event)
{
    KG_REQUIRE(d != nullptr, KG_ERR_INVALID, "kg_ddc_wf_tail_after: null argument");
    d->after_ev = event;
    return KG_OK;
}

// kg_ddc_wf_push_dev (max_out = 0: the continuous sampler) and kg_ddc_wf_capture_dev (max_out >= 1: CmdWFReset with
// WF_SAMP_WR_RST at the block's first sample, then the one-shot sampler of verilog/rx/iq_sampler_8k_32b.v, which stops
// when it holds max_out pairs: only the first max_out << log2r samples of the block reach a channel's filters).
// kg_ddc_wf_step_dev: the sampler mode PER ENTRY (max_out_tab[i]: 0 continuous, >= 1 reset + one-shot of that many pairs) and
// an offset into each entry's row (out_off[i] pairs): a bank of receivers in both modes in one set of launches.
//
// ddc_push_impl is the list of a push's steps: check, resets, plan (kg_ddc_plan.h: every decision of the call, pure host
// arithmetic), buffers, tables, enqueue (which decides nothing), commit.
struct ddc_push_args {
    const void *d_adc; size_t n; const int32_t *chan_list; int nlist; void *d_out; size_t out_stride; size_t max_out;
    int64_t *nouts; const int64_t *max_out_tab, *out_off;
    u64 cap(int i) const { return max_out_tab ? (u64) max_out_tab[i] : (u64) max_out; }      // 0: continuous sampler
};

// Step 1: the arguments.
static int ddc_push_check(kg_ddc *d, const ddc_push_args &a)
{
    KG_REQUIRE(d && a.d_adc && a.chan_list && a.d_out, KG_ERR_INVALID, "kg_ddc_wf_push_dev: null argument");
    for (int i = 0; i < a.nlist; i++) {
        KG_REQUIRE(!a.max_out_tab || (a.max_out_tab[i] >= 0 && a.max_out_tab[i] <= ((int64_t) 1 << 31)), KG_ERR_INVALID,
                   "kg_ddc_wf_step_dev: max_out[%d] = %lld", i, (long long) a.max_out_tab[i]);
        KG_REQUIRE(!a.out_off || (a.out_off[i] >= 0 && (size_t) a.out_off[i] <= a.out_stride), KG_ERR_INVALID,
                   "kg_ddc_wf_step_dev: out_off[%d] = %lld outside the row", i, a.out_off ? (long long) a.out_off[i] : 0ll);
    }
    KG_TRY(kg_ctx_use(d->ctx));
    KG_REQUIRE(a.n >= 1 && (long) a.n <= d->max_samples, KG_ERR_INVALID, "kg_ddc_wf_push_dev: n %zu (max %ld)", a.n, d->max_samples);
    KG_REQUIRE(a.nlist >= 1 && a.nlist <= d->nchan, KG_ERR_INVALID, "kg_ddc_wf_push_dev: nlist %d", a.nlist);
    KG_REQUIRE(((uintptr_t) a.d_adc & 1) == 0 && ((uintptr_t) a.d_out & 3) == 0, KG_ERR_INVALID,
               "kg_ddc_wf_push_dev: misaligned pointer");
    std::vector<char> &seen = d->seen;                              // (a flag per channel: no quadratic search of the list)
    seen.assign(d->nchan, 0);
    for (int i = 0; i < a.nlist; i++) {
        const int ch = a.chan_list[i];
        KG_REQUIRE(ch >= 0 && ch < d->nchan && d->h_chans[ch].active, KG_ERR_STATE,
                   "kg_ddc_wf_push_dev: channel %d is not configured", ch);
        KG_REQUIRE(!seen[ch], KG_ERR_INVALID, "kg_ddc_wf_push_dev: channel %d listed twice", ch);
        seen[ch] = 1;
    }
    return KG_OK;
}

// Step 2, not in a bank's PLAN pass (which changes nothing: the planner computes with the counts the reset WILL leave, refuses
// a rebase, and the replay pass comes here).  Synchronising, rare.
// A channel a capture left behind holds the filter state of a block cut short: the next CONTINUOUS push starts it
// from the reset state, as the reference does when it changes sampler mode (CmdWFReset with WF_SAMP_CONTIN,
// rx/rx_waterfall.cpp:971-978).  (Before the ages are compared: a reset moves the channel's reference point.)
// Then the 2^62 rule (DDC_PLAN_REBASE_AT): every channel of the call moves its reference point to "now".
static int ddc_push_resets(kg_ddc *d, const ddc_push_args &a)
{
    u64 oldest = 0;
    for (int i = 0; i < a.nlist; i++) {
        const int ch = a.chan_list[i];
        if (a.cap(i) == 0 && d->h_stale[ch]) {
            KG_TRY(kg_ddc_reset_wf(d, ch));
            d->h_stale[ch] = 0;
        }
        if (d->h_pushed[ch] > oldest) oldest = d->h_pushed[ch];
    }
    if (oldest + (u64) a.n >= DDC_PLAN_REBASE_AT)
        for (int i = 0; i < a.nlist; i++) KG_TRY(ddc_rebase(d, a.chan_list[i]));
    return KG_OK;
}

static ddc_plan_switch ddc_switch_of(const char *text)
{
    const ddc_plan_switch s = {text != nullptr, text ? atoi(text) : 0};
    return s;
}

// Step 3: the object's state and the tuning switches -> the planner; its refusals in the order it makes its checks.
static int ddc_push_plan(kg_ddc *d, const ddc_push_args &a, bool plan_pass, ddc_plan &P)
{
    std::vector<ddc_plan_entry> e(a.nlist);
    for (int i = 0; i < a.nlist; i++) {
        const int ch = a.chan_list[i];
        const ddc_plan_entry ei = {ch, d->h_chans[ch].log2r, ddc_cur_cnt(d, ch), d->h_pushed[ch], d->h_stale[ch] != 0, a.cap(i),
                                   a.out_off ? (long) a.out_off[i] : 0l};
        e[i] = ei;
    }
    const ddc_plan_in in = {(long) a.n, a.out_stride, d->ctx->num_cus, d->max_runs, plan_pass,
                            ddc_switch_of(kg_tuning_env("KIWIGPU_DDC_RUNS")), ddc_switch_of(kg_tuning_env("KIWIGPU_DDC_SIDE")),
                            ddc_switch_of(kg_tuning_env("KIWIGPU_DDC_STAGED"))};
    ddc_plan_make(e.data(), a.nlist, in, P);
    KG_REQUIRE(P.refusal != DDC_REFUSE_AGE, KG_ERR_STATE, "kg_ddc_wf_push_dev: 2^62 samples since a channel was last set");
    const int ncounted = P.refusal == DDC_REFUSE_OUT_STRIDE ? P.bad : a.nlist;
    if (a.nouts) for (int i = 0; i < ncounted; i++) a.nouts[i] = P.nouts[i];
    KG_REQUIRE(P.refusal != DDC_REFUSE_OUT_STRIDE, KG_ERR_INVALID, "kg_ddc_wf_push_dev: out_stride %zu < %ld outputs of channel %d (at offset %ld)",
               a.out_stride, P.nouts[P.bad], a.chan_list[P.bad], P.outoff[P.bad]);
    KG_REQUIRE(P.refusal != DDC_REFUSE_COMB_WGS, KG_ERR_INVALID, "kg_ddc_wf_push_dev: too many outputs in one call");
    KG_REQUIRE(P.refusal != DDC_REFUSE_NRUNS, KG_ERR_INVALID, "kg_ddc_wf_push_dev: %d runs > %d", P.nruns, d->max_runs);
    return KG_OK;
}

// Steps 4 and 5 run in a bank's PLAN pass too, up to the KG_PLAN_ONLY behind them, and there they do more than arithmetic:
//   - d_c0rel[par] may grow, behind a ddc_sync_all.  This push has enqueued nothing yet, so the drain waits only for
//     earlier pushes, and the REPLAY pass finds the capacity there.  (The drain clears tail_unjoined, rightly: the
//     context's stream has then waited for everything.)
// and, if the object has an output stream (it was in deferred mode once; a receiver bank's DDC never is):
//   - the context's stream and the second stream are made to wait for ev_tail[par], the output stage that last used this
//     push's buffer set.  One more wait for an event recorded two pushes ago orders nothing new, and the REPLAY pass
//     enqueues the same waits again in front of its launches.
//   - a CHANGED table block makes the context's stream wait for the previous output stage and clears tail_unjoined.  (With
//     an arena the stage cache is neither asked nor filled, so every block counts as changed.)  The wait lands in front of
//     the owner's one upload of the step's tables, where it has to be: that upload is what rewrites the tables.  The
//     REPLAY pass then finds nothing left to join.
// None of this touches a channel's state, the buffer parity or an event of this push: after a PLAN pass that is never
// replayed the object computes what it would have computed without it.

// Step 4: this push's buffer set.  It was last used two pushes ago: its output stage must have drained it (deferred mode; long done).
static int ddc_push_buffers(kg_ddc *d, const ddc_plan &P)
{
    const int par = d->parity;
    if (d->tail && d->tail_rec[par]) {
        KG_HIP(hipStreamWaitEvent(d->ctx->stream, d->ev_tail[par], 0));
        if (d->side) KG_HIP(hipStreamWaitEvent(d->side, d->ev_tail[par], 0));
    }
    if (P.c0_need > d->c0_cap[par]) {
        KG_TRY(ddc_sync_all(d));
        d->d_c0rel[par].reset(); d->c0_cap[par] = 0;    // nothing dangles if the allocation below fails
        KG_TRY(d->d_c0rel[par].alloc((size_t) (P.c0_need + 16), "kg_ddc_wf_push_dev: comb inputs"));
        d->c0_cap[par] = P.c0_need;
    }
    return KG_OK;
}

struct ddc_tabs {                                 // the staged tables of a push, on the device
    const long *c0off, *nouts, *nlim, *outoff; const u64 *pdelta; const int *list, *wgoff, *bypass, *run, *small, *rest, *reset;
};

// Step 5.  The per-call tables go through the context's staging ring in one piece: no stream synchronisation, and the
// previous call's kernels keep their own copy.
static int ddc_push_tables(kg_ddc *d, const ddc_plan &P, ddc_tabs &t)
{
    const int par = d->parity;
    // a CHANGED table is rewritten in the order of the context's stream: the previous push's output stage, on its own
    // stream in deferred mode, may still be reading the old one -- join it first (a steady stream never gets here)
    if (d->tail && d->tail_rec[par ^ 1] && d->tail_unjoined &&
        !(d->pack_cache.bytes == P.block.size() && d->pack_cache.host && memcmp(d->pack_cache.host, P.block.data(), P.block.size()) == 0)) {
        KG_HIP(hipStreamWaitEvent(d->ctx->stream, d->ev_tail[par ^ 1], 0));
        d->tail_unjoined = false;
    }
    void *base = nullptr;
    KG_TRY(kg_ctx_stage_cached(d->ctx, &d->pack_cache, P.block.data(), P.block.size(), &base));
    const unsigned char *b = (const unsigned char *) base;
    t.c0off = (const long *) (b + P.o_c0off); t.nouts = (const long *) (b + P.o_nouts); t.nlim = (const long *) (b + P.o_nlim);
    t.pdelta = (const u64 *) (b + P.o_pdelta); t.list = (const int *) (b + P.o_list); t.wgoff = (const int *) (b + P.o_wgoff);
    t.bypass = (const int *) (b + P.o_bypass); t.run = (const int *) (b + P.o_run);
    t.small = (const int *) (b + P.o_small); t.rest = (const int *) (b + P.o_rest);
    t.reset = (const int *) (b + P.o_reset); t.outoff = (const long *) (b + P.o_outoff);
    return KG_OK;
}

// Step 6 in three parts, each enqueueing what the plan says where the plan says.
struct ddc_push_job {
    kg_ddc *d; const ddc_push_args &a; const ddc_plan &P; const ddc_tabs &t;
    int par;                                       // this push's buffer set
    bool defer;
    hipStream_t st, ost;                           // the context's stream; where the writers of the caller's rows run
    bool side_used;
};

static int ddc_side_ready(kg_ddc *d)
{
    if (!d->side) {
        KG_TRY(kg_stream_get(d->ctx->device, &d->side));
        KG_HIP(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
        KG_HIP(hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming));
    }
    return KG_OK;
}

// Where the output stage runs, and the R = 1 bypass kernel.
static int ddc_enqueue_bypass(ddc_push_job &j)
{
    kg_ddc *d = j.d; const ddc_push_args &a = j.a; const ddc_plan &P = j.P; const ddc_tabs &t = j.t;
    // Deferred mode: the output stage's stream starts behind the tables and the caller's samples (fork event), behind the
    // previous push's output stage (stream order) and behind the caller's last reader of the rows (kg_ddc_wf_tail_after).
    if (j.defer) {
        KG_TRY(ddc_side_ready(d));
        j.ost = d->tail;
        KG_HIP(hipEventRecord(d->ev_fork, j.st));
        KG_HIP(hipStreamWaitEvent(j.ost, d->ev_fork, 0));
        if (d->after_ev) KG_HIP(hipStreamWaitEvent(j.ost, (hipEvent_t) d->after_ev, 0));
    } else if (d->after_ev) {
        KG_HIP(hipStreamWaitEvent(j.st, (hipEvent_t) d->after_ev, 0));
    }
    d->after_ev = nullptr;
    if (P.bypass.empty()) return KG_OK;
    hipStream_t bst = j.ost;
    if (!j.defer && P.bypass_beside) {
        KG_TRY(ddc_side_ready(d));
        KG_HIP(hipEventRecord(d->ev_fork, j.st));                    // behind the staged tables
        KG_HIP(hipStreamWaitEvent(d->side, d->ev_fork, 0));
        bst = d->side; j.side_used = true;
    }
    hipLaunchKernelGGL(ddc_wf_bypass_kernel, dim3((unsigned) P.bypass_blocks), dim3(256),
                       0, bst, (const short *) a.d_adc, (long) P.n_by_max, (const ddc_chan *) d->d_chans, t.list,
                       t.bypass, (int) P.bypass.size(), (const u32 *) d->d_nco, (short2 *) a.d_out, (long) a.out_stride, P.pushed, t.pdelta, t.nlim, t.outoff, d->ctx->rows_by_chan);
    KG_HIP(hipGetLastError());
    if (j.defer) KG_HIP(hipEventRecord(d->ev_adc, bst));             // the output stream's only reader of d_adc
    return KG_OK;
}

// The run passes on the context's stream: end coefficients, pass A, the state scan, pass B.
static int ddc_enqueue_runs(ddc_push_job &j)
{
    kg_ddc *d = j.d; const ddc_push_args &a = j.a; const ddc_plan &P = j.P; const ddc_tabs &t = j.t;
    const int par = j.par;
    hipStream_t st = j.st;
    ddc_state4 *const d_local = d->d_local[par];
    u32 *const d_c0rel = d->d_c0rel[par], *const d_tau = d->d_tau[par];
    // end-referred carry states (round 4): the coefficients of the runs' distances to the end, then prefix sums inside
    // pass A's workgroups + one wave per (channel, I/Q) over the workgroup totals
    if (!P.run.empty() && (d->endco_n != P.n_cover || d->endco_L != P.L || d->endco_runs != P.nruns)) {
        // (a changed block length: rare.  The previous push's pass B may still be reading the old table on the object's
        // second stream)
        KG_TRY(ddc_sync_all(d));
        hipLaunchKernelGGL(ddc_endco_kernel, dim3((unsigned) ((P.nruns + 1 + 255) / 256)), dim3(256), 0, st, d->d_endco, P.n_cover, P.L, P.nruns);
        KG_HIP(hipGetLastError());
        d->endco_n = P.n_cover; d->endco_L = P.L; d->endco_runs = P.nruns;
    }
    if (!P.run.empty()) {
        auto pass_a = P.a_narrow ? ddc_wf_run_kernel<false, DDC_NARROW> : ddc_wf_run_kernel<false, DDC_ALL>;
        hipLaunchKernelGGL(pass_a, dim3((unsigned) P.gx, (unsigned) P.run.size()), dim3(DDC_THREADS), 0, st,
                           (const short *) a.d_adc, (long) a.n, P.L, P.nruns, (const ddc_chan *) d->d_chans, t.list,
                           (const u32 *) d->d_nco, d_local, d_c0rel, d_tau, t.c0off,
                           t.nouts, t.run, 0, P.pushed, t.pdelta, t.nlim, t.reset, (const ddc_endco *) d->d_endco, d->endco_n,
                           d->d_wgtot[par], (const ddc_state4 *) nullptr, (u32 *) nullptr);
        KG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ddc_wf_scan_wg_kernel, dim3((unsigned) (2 * a.nlist)), dim3(64), 0, st, (const ddc_state4 *) d->d_wgtot[par],
                       d->d_wgbase[par], P.gx, d->d_chans, t.list, t.nlim, t.reset);
    KG_HIP(hipGetLastError());
    // Pass B (ddc_plan_launches): the one launch on the second stream forks behind the state scan and joins before the
    // run-total prefix.
    const int *const sels[3] = {t.run, t.small, t.rest};
    for (int k = 0; k < P.nb; k++) {
        const ddc_plan_launch &l = P.b[k];
        hipStream_t s = st;
        if (l.side) {
            KG_TRY(ddc_side_ready(d));
            j.side_used = true;
            KG_HIP(hipEventRecord(d->ev_fork, st));
            KG_HIP(hipStreamWaitEvent(d->side, d->ev_fork, 0));
            s = d->side;
        }
        const int stage = l.staged ? DDC_STAGE_BYTES : 0;
        auto pass_b = l.mode == DDC_NARROW ? ddc_wf_run_kernel<true, DDC_NARROW> : (l.mode == DDC_WIDE ? ddc_wf_run_kernel<true, DDC_WIDE> : ddc_wf_run_kernel<true, DDC_ALL>);
        hipLaunchKernelGGL(pass_b, dim3((unsigned) P.gx, (unsigned) l.count), dim3(DDC_THREADS), stage, s,
                           (const short *) a.d_adc, (long) a.n, P.L, P.nruns, (const ddc_chan *) d->d_chans, t.list,
                           (const u32 *) d->d_nco, d_local, d_c0rel, d_tau, t.c0off, t.nouts, sels[l.sel] + l.first, stage, P.pushed, t.pdelta, t.nlim, t.reset, (const ddc_endco *) d->d_endco, d->endco_n,
                           (ddc_state4 *) nullptr, (const ddc_state4 *) d->d_wgbase[par], d->d_wgtau[par]);
        KG_HIP(hipGetLastError());
    }
    return KG_OK;
}

// The output stage: run-total prefix, combs, comb history -- in line on the context's stream, or (deferred) on the
// object's output stream behind this push's run passes, with the context's stream free for the next push's.
static int ddc_enqueue_output(ddc_push_job &j)
{
    kg_ddc *d = j.d; const ddc_push_args &a = j.a; const ddc_plan &P = j.P; const ddc_tabs &t = j.t;
    const int par = j.par;
    hipStream_t st = j.st, ost = j.ost;
    if (j.defer) {
        KG_HIP(hipEventRecord(d->ev_runs, st));
        KG_HIP(hipStreamWaitEvent(ost, d->ev_runs, 0));
    }
    if (j.side_used) {                            // everything the second stream did is behind this point of the output stage
        KG_HIP(hipEventRecord(d->ev_join, d->side));
        KG_HIP(hipStreamWaitEvent(ost, d->ev_join, 0));
    }
    hipLaunchKernelGGL(ddc_wf_tau_wg_kernel, dim3(2 * a.nlist), dim3(64), 0, ost, d->d_wgtau[par], P.gx, d->d_chans, t.list,
                       t.reset);
    KG_HIP(hipGetLastError());
    if (P.comb_wgs > 0) {
        hipLaunchKernelGGL(ddc_wf_comb_kernel, dim3((unsigned) P.comb_wgs), dim3(256), 0, ost,
                           (const u32 *) d->d_c0rel[par], (const u32 *) d->d_tau[par], P.log2L, P.nruns, t.c0off,
                           (const ddc_chan *) d->d_chans, t.list, t.nouts,
                           P.pushed, t.pdelta, t.reset, t.wgoff, a.nlist, (short2 *) a.d_out, (long) a.out_stride, t.outoff,
                           d->d_hist, (const u32 *) d->d_wgtau[par], P.gx, d->ctx->rows_by_chan);
        KG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ddc_wf_finish_kernel, dim3((a.nlist + 63) / 64), dim3(64), 0, ost, d->d_chans,
                       t.list, a.nlist, (long) a.n, t.nouts, (const u32 *) d->d_hist, t.reset);
    KG_HIP(hipGetLastError());
    if (d->tail) {                                // (also in line: a later deferred push finds its buffer set covered)
        KG_HIP(hipEventRecord(d->ev_tail[par], ost));
        d->tail_rec[par] = true;
        d->tail_unjoined = j.defer;
    }
    if (j.defer) {
        // Everything that READS the caller's samples is ordered in front of whatever the caller enqueues next on the
        // context's stream (a streaming caller refills or recycles d_adc there): the run passes are on that stream already;
        // the bypass kernel (output stream) and pass B of the small decimations (second stream) are joined here.  Only the
        // readers: the output stage proper (run-total prefix, combs) stays free to run beside the next push.
        if (!P.bypass.empty()) KG_HIP(hipStreamWaitEvent(st, d->ev_adc, 0));
        if (j.side_used) KG_HIP(hipStreamWaitEvent(st, d->ev_join, 0));
    }
    return KG_OK;
}

static int ddc_push_enqueue(kg_ddc *d, const ddc_push_args &a, const ddc_plan &P, const ddc_tabs &t)
{
    ddc_push_job j = {d, a, P, t, d->parity, d->deferred, d->ctx->stream, d->ctx->stream, false};
    KG_TRY(ddc_enqueue_bypass(j));
    KG_TRY(ddc_enqueue_runs(j));
    return ddc_enqueue_output(j);
}

// Step 7: the push is in the queues.
static void ddc_push_commit(kg_ddc *d, const ddc_push_args &a)
{
    d->parity ^= 1;
    for (int i = 0; i < a.nlist; i++) {
        d->h_pushed[a.chan_list[i]] += (u64) a.n;                  // the NCO runs through the whole block either way
        if (a.cap(i) != 0) d->h_stale[a.chan_list[i]] = 1;         // filters stopped short of the block's end
    }
}

static int ddc_push_impl(kg_ddc *d, const void *d_adc, size_t n, const int32_t *chan_list, int nlist,
                         void *d_out, size_t out_stride, size_t max_out, int64_t *nouts,
                         const int64_t *max_out_tab = nullptr, const int64_t *out_off = nullptr)
{
    const ddc_push_args a = {d_adc, n, chan_list, nlist, d_out, out_stride, max_out, nouts, max_out_tab, out_off};
    KG_TRY(ddc_push_check(d, a));
    const bool plan_pass = d->ctx->arena && d->ctx->arena->mode == KG_ARENA_PLAN;
    if (!plan_pass) KG_TRY(ddc_push_resets(d, a));
    ddc_plan P;
    ddc_tabs t;
    KG_TRY(ddc_push_plan(d, a, plan_pass, P));
    KG_TRY(ddc_push_buffers(d, P));
    KG_TRY(ddc_push_tables(d, P, t));
    KG_PLAN_ONLY(d->ctx);
    KG_TRY(ddc_push_enqueue(d, a, P, t));
    ddc_push_commit(d, a);
    return KG_OK;
}


int kg_ddc_wf_push_dev(kg_ddc *d, const void *d_adc, size_t n, const int32_t *chan_list, int nlist,
                       void *d_out, size_t out_stride, int64_t *nouts)
{
    return ddc_push_impl(d, d_adc, n, chan_list, nlist, d_out, out_stride, 0, nouts);
}

int kg_ddc_wf_capture_dev(kg_ddc *d, const void *d_adc, size_t n, const int32_t *chan_list, int nlist,
                          void *d_out, size_t out_stride, size_t max_out, int64_t *nouts)
{
    KG_REQUIRE(max_out >= 1 && max_out <= ((size_t) 1 << 31), KG_ERR_INVALID, "kg_ddc_wf_capture_dev: max_out %zu", max_out);
    return ddc_push_impl(d, d_adc, n, chan_list, nlist, d_out, out_stride, max_out, nouts);
}

int kg_ddc_wf_step_dev(kg_ddc *d, const void *d_adc, size_t n, const int32_t *chan_list, int nlist, void *d_out,
                       size_t out_stride, const int64_t *out_off, const int64_t *max_out, int64_t *nouts)
{
    KG_REQUIRE(max_out != nullptr, KG_ERR_INVALID, "kg_ddc_wf_step_dev: max_out is null");
    return ddc_push_impl(d, d_adc, n, chan_list, nlist, d_out, out_stride, 0, nouts, max_out, out_off);
}

}  // extern "C"
