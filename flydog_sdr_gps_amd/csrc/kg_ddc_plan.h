// kg_ddc_plan.h -- what one waterfall-DDC push (kg_ddc_wf_push_dev / _capture_dev / _step_dev) will do, decided on the host.
//
// Plain C++: no HIP, no environment, no kg_ddc.  ddc_plan_make() is a pure function of the call's list (one ddc_plan_entry per
// entry, as the object's state stands AFTER the rare resets of kg_ddc.hip's "Resets" step), the block length and a few scalars
// of the object and the device.  kg_ddc.hip turns the plan into staged tables and launches without deciding anything again;
// tools/ddc_plan_host_driver.cpp prints it for tests/test_ddc_plan_cpu.py, which holds every branch to values derived by hand
// at 256 and at 8 compute units -- half of the branches need millions of samples to be taken on a real device.
#pragma once

#include <stdint.h>
#include <string.h>
#include <vector>

static const int DDC_RUN_MIN = 64, DDC_RUN_MAX = 8192, DDC_TARGET_RUNS = 8192;
// What the kernels fix (kg_ddc.hip asserts that they agree): threads of a run-pass workgroup, one run each; outputs of a comb
// workgroup; samples of a bypass block.
static const int DDC_PLAN_THREADS = 256, DDC_PLAN_COMB_TILE = 1024, DDC_PLAN_BYPASS_BLOCK = 4096;
// (the kernels form (age + sample index) x phase_inc in 64 bits mod 2^48: re-base long before anything wraps)
static const uint64_t DDC_PLAN_REBASE_AT = 1ull << 62;

struct ddc_plan_entry {
    int chan, log2r;
    uint32_t cnt;                  // the decimation counter as it stands (ddc_cur_cnt)
    uint64_t age;                  // samples pushed since the channel's reference point (h_pushed)
    bool stale;                    // a capture cut its filters short
    uint64_t max_out;              // 0: the continuous sampler; >= 1: reset + one-shot sampler of that many pairs
    long out_off;                  // pairs into the entry's row
};

// A tuning switch as kg_tuning_env answered it: unset, or atoi of its text.
struct ddc_plan_switch { bool set; int v; };

struct ddc_plan_in {
    long n;
    size_t out_stride;
    int num_cus, max_runs;
    bool plan_pass;                // a receiver bank's PLAN pass: nothing may be rebased, so the 2^62 rule refuses
    ddc_plan_switch runs, side, staged;       // KIWIGPU_DDC_RUNS, KIWIGPU_DDC_SIDE, KIWIGPU_DDC_STAGED
};

// The refusals that depend on planned values, in the order the checks are made.  `bad` is the entry an OUT_STRIDE refusal names:
// the entries before it have their output counts, it and the later ones do not.
enum { DDC_REFUSE_NONE = 0, DDC_REFUSE_AGE, DDC_REFUSE_OUT_STRIDE, DDC_REFUSE_COMB_WGS, DDC_REFUSE_NRUNS };

// Pass B: which entries (a piece of the selection `run`, `small` or `rest`), in which form of ddc_wf_run_kernel<true, mode>,
// with the staged strobe flush or without, on the object's second stream or in line.
enum { DDC_B_NONE = 0, DDC_B_BESIDE, DDC_B_STAGED, DDC_B_ONE, DDC_B_REST };
enum { DDC_SEL_RUN = 0, DDC_SEL_SMALL, DDC_SEL_REST };
enum { DDC_PLAN_ALL = 0, DDC_PLAN_NARROW = 1, DDC_PLAN_WIDE = 2 };
struct ddc_plan_launch { int sel, first, count, mode; bool staged, side; };

struct ddc_plan {
    int refusal, bad;
    // per entry
    std::vector<char> will_reset;              // continuous and stale: planned with the counts the reset leaves
    std::vector<long> c0off, nouts, nlim, outoff;
    std::vector<uint64_t> pdelta;              // age above `pushed`
    std::vector<int> list, wgoff, reset;       // (wgoff: nlist + 1 values)
    // selections of entries: R = 1; R >= 2; 2 <= R <= 8; the 16 <= R <= 256 entries (nmid of them), then the R >= 512 ones
    std::vector<int> bypass, run, small, rest;
    int nmid;
    uint64_t pushed;                           // the youngest age of the call
    bool need_rebase;                          // the oldest age + n reaches 2^62
    bool capture;                              // some entry captures
    long c0_need, comb_wgs, n_by_max, n_cover;
    int L, log2L, nruns, gx;                   // run length, runs, run-pass workgroups per entry
    bool a_narrow;                             // pass A in its 64-bit form alone (L <= 1024)
    bool bypass_beside;                           // the bypass kernel beside the run passes, where there are any (in-line mode)
    long bypass_blocks;
    int b_form; bool split;
    int nb; ddc_plan_launch b[3];
    // The per-call tables in one block, every table at a multiple of 16 bytes: c0off, nouts, nlim, pdelta, list, wgoff, bypass,
    // run, small, rest, reset, outoff.  (The stage cache compares it byte for byte; a bank's REPLAY pass checks it against the
    // one planned.)
    std::vector<unsigned char> block;
    size_t o_c0off, o_nouts, o_nlim, o_pdelta, o_list, o_wgoff, o_bypass, o_run, o_small, o_rest, o_reset, o_outoff;
};

static inline size_t ddc_plan_put(std::vector<unsigned char> &block, const void *src, size_t bytes)
{
    const size_t at = (block.size() + 15) & ~(size_t) 15;
    block.resize(at + bytes);
    if (bytes) memcpy(block.data() + at, src, bytes);
    return at;
}

// Ages and per-entry tables.  False: refused (P.refusal, P.bad).
static inline bool ddc_plan_entries(const ddc_plan_entry *e, int nlist, const ddc_plan_in &in, ddc_plan &P, long *n_run_max, long *n_run_sum)
{
    const uint64_t n = (uint64_t) in.n;
    // Channels whose reference points differ in age (one was retuned -- the most common command of a connection -- or joined
    // later, or was left out of earlier calls): the call passes the YOUNGEST age as `pushed` and a table of what each entry has
    // on top of it.  The table is the same from push to push while no channel is touched (every age grows by n), so it rides in
    // the content-cached per-call tables.
    // A channel a capture left behind starts its next CONTINUOUS push from the reset state: age and counter zero.
    P.will_reset.assign(nlist, 0);
    for (int i = 0; i < nlist; i++) P.will_reset[i] = e[i].max_out == 0 && e[i].stale;
    auto age_of = [&](int i) -> uint64_t { return P.will_reset[i] ? 0ull : e[i].age; };
    uint64_t oldest = P.pushed = age_of(0);
    for (int i = 1; i < nlist; i++) {
        const uint64_t a = age_of(i);
        if (a < P.pushed) P.pushed = a;
        if (a > oldest) oldest = a;
    }
    P.need_rebase = oldest + n >= DDC_PLAN_REBASE_AT;
    if (P.need_rebase && in.plan_pass) { P.refusal = DDC_REFUSE_AGE; return false; }
    P.pdelta.resize(nlist);
    for (int i = 0; i < nlist; i++) P.pdelta[i] = age_of(i) - P.pushed;
    P.c0off.resize(nlist); P.nouts.resize(nlist); P.nlim.resize(nlist); P.outoff.resize(nlist);
    P.list.resize(nlist); P.wgoff.resize(nlist + 1); P.reset.resize(nlist);
    P.bypass.clear(); P.run.clear(); P.small.clear(); P.rest.clear();
    std::vector<int> big;
    P.capture = false;
    P.c0_need = P.comb_wgs = P.n_by_max = 0;
    *n_run_max = *n_run_sum = 0;
    for (int i = 0; i < nlist; i++) {
        const int log2r = e[i].log2r;
        // samples of the block this channel's filters see: all of them, or (capture) what fills the one-shot sampler
        const bool cap = e[i].max_out != 0;
        const uint64_t want = cap ? e[i].max_out << log2r : n;
        P.capture = P.capture || cap;
        P.list[i] = e[i].chan;
        P.reset[i] = cap ? 1 : 0;
        P.outoff[i] = e[i].out_off;
        P.nlim[i] = (long) (want < n ? want : n);
        P.nouts[i] = (long) (((cap || P.will_reset[i] ? 0ull : (uint64_t) e[i].cnt) + (uint64_t) P.nlim[i]) >> log2r);
        if (log2r) { if (P.nlim[i] > *n_run_max) *n_run_max = P.nlim[i]; *n_run_sum += P.nlim[i]; }
        else if (P.nlim[i] > P.n_by_max) P.n_by_max = P.nlim[i];
        if ((size_t) (P.nouts[i] + P.outoff[i]) > in.out_stride) { P.refusal = DDC_REFUSE_OUT_STRIDE; P.bad = i; return false; }
        P.c0off[i] = P.c0_need;
        if (log2r) P.c0_need += 2 * ((P.nouts[i] + 3) & ~3l);             // I and Q planes, each a multiple of 16 bytes
        P.wgoff[i] = (int) P.comb_wgs;
        if (log2r) P.comb_wgs += (P.nouts[i] + DDC_PLAN_COMB_TILE - 1) / DDC_PLAN_COMB_TILE;
        else P.bypass.push_back(i);
        if (log2r) { P.run.push_back(i); (log2r <= 3 ? P.small : (log2r <= 8 ? P.rest : big)).push_back(i); }
    }
    P.nmid = (int) P.rest.size();
    P.rest.insert(P.rest.end(), big.begin(), big.end());
    P.wgoff[nlist] = (int) P.comb_wgs;
    if (P.comb_wgs >= (1l << 31)) { P.refusal = DDC_REFUSE_COMB_WGS; return false; }
    return true;
}

// Run length, runs and the form of pass A.  False: refused.
static inline bool ddc_plan_runs(int nlist, const ddc_plan_in &in, ddc_plan &P, long n_run_max, long n_run_sum)
{
    // run length: a power of two between 64 and 8192, about 8192 runs per call
    // One thread per (channel, run): with few channels take more, shorter runs so that the two
    // run passes still put about four waves on every SIMD (14 channels on MI355X: 16384 runs
    // instead of 8192 = 2.18 -> 1.91 ms per 2^24 samples, although the state scan doubles).
    const long want_threads = (long) in.num_cus * 4 * 4 * 64;
    int target = DDC_TARGET_RUNS;
    const long per_chan = (want_threads + nlist - 1) / nlist;
    if (per_chan > target) target = per_chan < in.max_runs ? (int) per_chan : in.max_runs;
    if (in.runs.set && in.runs.v >= 64 && in.runs.v <= in.max_runs) target = in.runs.v;
    // the runs cover the longest share of the block any filtered channel takes (the whole block unless capturing)
    P.n_cover = n_run_max > 0 ? n_run_max : 1;
    int L = DDC_RUN_MIN;
    while (L < DDC_RUN_MAX && (long) ((P.n_cover + L - 1) / L) > target) L <<= 1;
    if (P.capture) {
        // a capture's channels take very different shares (8192 R samples each): size the runs by the TOTAL work, about
        // four waves per SIMD over all of them, inside what the longest share allows
        // (runs of at most 1024 samples: pass A then integrates every decimation in 64 bits -- short_zero_run in
        // ddc_wf_run_body; with SURVEY's receiver mix, 352 M sample-channels per step, the total-work rule alone chose 2048 and
        // pass A of the R >= 512 channels ran its 128-bit form: 1.13 ms per step against pass B's 0.71)
        int Lw = DDC_RUN_MIN;
        while (Lw < 1024 && n_run_sum / Lw > want_threads) Lw <<= 1;
        if (Lw > L) L = Lw;
        while (L < DDC_RUN_MAX && (P.n_cover + L - 1) / L > in.max_runs) L <<= 1;
    }
    P.L = L;
    P.nruns = (int) ((P.n_cover + L - 1) / L);
    P.log2L = 0;
    while ((1 << P.log2L) < L) P.log2L++;
    if (P.nruns > in.max_runs) { P.refusal = DDC_REFUSE_NRUNS; return false; }
    P.gx = (P.nruns + DDC_PLAN_THREADS - 1) / DDC_PLAN_THREADS;
    // (runs of at most 1024 samples: every decimation integrates from zero in 64 bits -- the narrow form alone)
    P.a_narrow = L <= 1024;
    return true;
}

// The bypass kernel's grid and stream, and pass B's launches.
static inline void ddc_plan_launches(const ddc_plan_in &in, ddc_plan &P)
{
    // The object's second stream: work that does not depend on the pass A -> scan -> pass B chain runs beside
    // it -- the R = 1 bypass channels (no filter state at all) from the start, pass B of the R <= 8 channels
    // (below) -- and joins before the call's last kernels.  KIWIGPU_DDC_SIDE=0: everything in line.
    const bool side = in.side.set ? in.side.v != 0 : true;
    P.bypass_beside = side && !P.bypass.empty() && !P.run.empty();
    const long nblk_by = (P.n_by_max + DDC_PLAN_BYPASS_BLOCK - 1) / DDC_PLAN_BYPASS_BLOCK, cap_by = (long) in.num_cus * 4;   // LDS: 20 KiB each, 4 per CU
    P.bypass_blocks = P.bypass.empty() ? 0 : (nblk_by < cap_by ? nblk_by : cap_by);
    // Pass B.  The staged strobe flush (R <= 8) needs 34 KiB more LDS, hence its own launch.  Neither
    // launch fills the GPU by itself (a lane walks a whole run: 64 workgroups per channel), so when both
    // kinds of channel are present the staged launch runs beside the other one on a second stream of the
    // object (fork after the state scan, join before the run-total prefix); with only small decimations
    // it pays once those channels fill the GPU by themselves, otherwise the scattered stores are cheaper
    // than the smaller grid.
    const long fill = (long) in.num_cus * 4 * 2 * 64;
    bool staged = (long) P.small.size() * P.nruns >= fill;
    if (in.staged.set) staged = in.staged.v != 0 && !P.small.empty();
    const bool beside = side && !P.small.empty() && !P.rest.empty();
    // The entries above R = 8 by the form they need (DDC_NARROW / DDC_WIDE: fewer registers, more waves per SIMD) -- as two
    // launches when each of them fills the GPU by itself (a bank of receivers), as one launch of the general form otherwise
    // (configs[2]'s five and three such channels: two half-empty launches one after the other would lose more than the
    // waves gain).
    const int nmid = P.nmid, nbig = (int) P.rest.size() - nmid;
    P.split = (nmid == 0 || (long) nmid * P.nruns >= fill) && (nbig == 0 || (long) nbig * P.nruns >= fill);
    P.nb = 0;
    auto add = [&](int sel, int first, int count, int mode, bool stg, bool on_side) {
        const ddc_plan_launch l = {sel, first, count, mode, stg, on_side};
        if (count) P.b[P.nb++] = l;
    };
    auto add_rest = [&]() {
        if (!P.split) { add(DDC_SEL_REST, 0, (int) P.rest.size(), DDC_PLAN_ALL, false, false); return; }
        add(DDC_SEL_REST, 0, nmid, DDC_PLAN_NARROW, false, false);
        add(DDC_SEL_REST, nmid, nbig, DDC_PLAN_WIDE, false, false);
    };
    P.b_form = beside ? DDC_B_BESIDE : staged ? DDC_B_STAGED : !P.small.empty() ? DDC_B_ONE : !P.run.empty() ? DDC_B_REST : DDC_B_NONE;
    if (P.b_form == DDC_B_BESIDE || P.b_form == DDC_B_STAGED) {
        add(DDC_SEL_SMALL, 0, (int) P.small.size(), DDC_PLAN_ALL, true, beside);
        add_rest();
    } else if (P.b_form == DDC_B_ONE) {
        add(DDC_SEL_RUN, 0, (int) P.run.size(), DDC_PLAN_ALL, false, false);      // a few R <= 8 entries, not staged: everything in one launch
    } else if (P.b_form == DDC_B_REST) {
        add_rest();
    }
}

// nlist >= 1 entries, in.n >= 1.  P may be one that an earlier call filled: every field is set again.
static inline void ddc_plan_make(const ddc_plan_entry *e, int nlist, const ddc_plan_in &in, ddc_plan &P)
{
    long n_run_max, n_run_sum;
    P.refusal = DDC_REFUSE_NONE; P.bad = -1;
    P.block.clear();
    if (!ddc_plan_entries(e, nlist, in, P, &n_run_max, &n_run_sum)) return;
    if (!ddc_plan_runs(nlist, in, P, n_run_max, n_run_sum)) return;
    ddc_plan_launches(in, P);
    std::vector<unsigned char> &b = P.block;
    P.o_c0off = ddc_plan_put(b, P.c0off.data(), sizeof(long) * nlist); P.o_nouts = ddc_plan_put(b, P.nouts.data(), sizeof(long) * nlist);
    P.o_nlim = ddc_plan_put(b, P.nlim.data(), sizeof(long) * nlist); P.o_pdelta = ddc_plan_put(b, P.pdelta.data(), sizeof(uint64_t) * nlist);
    P.o_list = ddc_plan_put(b, P.list.data(), sizeof(int) * nlist);
    P.o_wgoff = ddc_plan_put(b, P.wgoff.data(), sizeof(int) * (nlist + 1));
    P.o_bypass = ddc_plan_put(b, P.bypass.data(), sizeof(int) * P.bypass.size());
    P.o_run = ddc_plan_put(b, P.run.data(), sizeof(int) * P.run.size());
    P.o_small = ddc_plan_put(b, P.small.data(), sizeof(int) * P.small.size());
    P.o_rest = ddc_plan_put(b, P.rest.data(), sizeof(int) * P.rest.size());
    P.o_reset = ddc_plan_put(b, P.reset.data(), sizeof(int) * nlist); P.o_outoff = ddc_plan_put(b, P.outoff.data(), sizeof(long) * nlist);
}
