// kg_ext.h -- host-side plumbing of the per-connection extension objects (kg_fftext, kg_iqd, kg_lorc, kg_fax, kg_cw): how one is
// created, how a handle and an index are checked, what a valid connection list is.  Host only.  DESIGN.md 6.9 lists what a
// further extension adds.
#pragma once

#include "kg_common.h"

#include <new>
#include <vector>

// A create: context in use, *out cleared, count in range, the object itself, then begin(obj) -- the caller's part: the count, how a
// connection's host state begins, the device state and whether it is zeroed (kg_ext_zero) -- and a failed begin torn down.
// `noun`: what the count is called in the refusal ("nconn", "nchan").
template <typename T, typename Begin> static inline int kg_ext_create(kg_ctx *ctx, int count, int max, const char *who, const char *noun, T **out, Begin begin)
{
    KG_TRY(kg_ctx_use(ctx));
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "%s: out is null", who);
    *out = nullptr;
    KG_REQUIRE(count >= 1 && count <= max, KG_ERR_INVALID, "%s: %s %d (1..%d)", who, noun, count, max);
    T *obj = new (std::nothrow) T();
    KG_REQUIRE(obj != nullptr, KG_ERR_NOMEM, "%s: alloc", who);
    obj->ctx = ctx;
    const int rc = begin(obj);
    if (rc) { kg_drain_delete(obj); return rc; }
    *out = obj;
    return KG_OK;
}

// n elements of a new object's device state zeroed in stream order (inside a create's begin)
template <typename D> static inline int kg_ext_zero(kg_ctx *ctx, D *d, size_t n, const char *who)
{
    KG_REQUIRE(hipMemsetAsync(d, 0, sizeof(D) * n, ctx->stream) == hipSuccess, KG_ERR_HIP, "%s: hipMemsetAsync failed", who);
    return KG_OK;
}

// The head of a command: the handle, then index idx of its `count` connections or channels (`noun`).
#define KG_EXT_INDEX(who, obj, idx, count, noun)                                                      \
    KG_REQUIRE((obj) != nullptr, KG_ERR_INVALID, who ": null handle");                                \
    KG_REQUIRE((idx) >= 0 && (idx) < (count), KG_ERR_INVALID, who ": " noun " %d of %d", idx, count)

// Entry i of a list of nlist connections, each listed once (`listed`: one char per connection of the object, zero before entry 0):
// the index c in range and not listed before, nblk in range, the stride at least the entry's nblk blocks of blk_len samples
// (a list of one has no stride, nor has one whose entries are `placed` by offsets of their own), and `at`, the entry's
// offset or row, not negative.  The two names are what the caller's refusals call its stride and `at`.
static inline int kg_ext_list_entry(const char *who, std::vector<char> &listed, int nlist, int i, int c, int nblk, int max_blk, const char *stride_name, size_t stride,
                                    size_t blk_len, bool placed, const char *at_name, long long at)
{
    const int count = (int) listed.size();
    KG_REQUIRE(c >= 0 && c < count, KG_ERR_INVALID, "%s: conns[%d] = %d of %d", who, i, c, count);
    KG_REQUIRE(!listed[c], KG_ERR_INVALID, "%s: connection %d is listed twice", who, c);
    listed[c] = 1;
    KG_REQUIRE(nblk >= 0 && nblk <= max_blk, KG_ERR_INVALID, "%s: nblk[%d] = %d (0..%d)", who, i, nblk, max_blk);
    KG_REQUIRE(nblk <= 0 || nlist == 1 || placed || stride >= blk_len * nblk, KG_ERR_INVALID, "%s: %s %zu below the %d blocks of entry %d", who, stride_name, stride,
               nblk, i);
    KG_REQUIRE(at >= 0, KG_ERR_INVALID, "%s: %s %lld of entry %d", who, at_name, at, i);
    return KG_OK;
}
