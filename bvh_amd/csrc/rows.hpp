// rows.hpp — what the batches share whose result is one variable-length row per query, as a CSR.  Its users are allhits.hip, within.hip,
// instances_allhits.hip and instances_within.hip, which bring their kernels and call rows_batch / rows_run below, and region.hip (both its
// entries), which schedules (region, chunk) units, has no sort and calls the scan (rows.hip) itself.  Here: the scan's interface, the sort
// network of the long rows, the empty result such a batch starts from, and the host schedule of a batch.
#pragma once

#include <type_traits>

#include "engine.hpp"

namespace bvhgpu {

constexpr uint32_t ROWS_SORT_THREADS = 256;   // workgroup of a family's k_*_sort_row
constexpr uint32_t ROWS_SCAN_ITEMS = 4;
constexpr uint32_t ROWS_SCAN_BLOCK = 256 * ROWS_SCAN_ITEMS;   // counts per workgroup of the scan

// A family keeps its own thresholds (rows up to LANE_ROW_MAX are sorted by the lane that fills them, up to LDS_ROW_MAX in LDS, longer
// ones in global memory) and hands them to the scan as arguments.  Its LDS_ROW_MAX has to pass this: a row sorted in LDS fits a
// workgroup's LDS (an f64 key, a position and a shape per element), and the LDS tier pads a row to a power of two inside its arrays
constexpr bool rows_lds_row_max_ok(uint32_t m) { return m * (sizeof(double) + 8u) <= 64u * 1024u && (m & (m - 1)) == 0; }

// rows.hip: the scan around a family's two walks, on h->ctx's stream, in h->rows_counts / rows_sums / rows_work.  In order:
//   rows_begin    reserves the three buffers (rows_work only with_work: a sorted batch) and zeroes the scan's meta words; returns the
//                 n counts that the family's count kernel, launched next, has to write
//   rows_scan     block sums, worklist (lane_max != 0: the queries with more than lane_max candidates; those above lds_max counted) and the
//                 scan of the sums, then the batch's ONE host read.  Throws Fail::Overflow for a total above 2^32 - 1; with a total of 0
//                 it zeroes h->offsets[0 .. n] and there is nothing left to do
//   rows_offsets  h->offsets[0 .. n] from the counts (needs a total != 0)
// h->offsets holds n + 1 words before rows_scan.  What a family reserves by the total goes between the last two where it likes.
struct RowsTotals { unsigned long long total; uint32_t n_long, n_beyond_lds; };
uint32_t* rows_begin(bvhgpu_hits* h, size_t n, bool with_work);
RowsTotals rows_scan(bvhgpu_hits* h, size_t n, uint32_t lane_max, uint32_t lds_max);
void rows_offsets(bvhgpu_hits* h, size_t n);

// the result object becomes an (empty) rows result of the kind `flags` (TRAVERSE_ALLHITS, _WITHIN, _REGION, _INST_ALLHITS, _INST_WITHIN):
// whatever fails behind this leaves it consistent
inline void rows_reset(bvhgpu_hits* h, bvhgpu_ctx* ctx, int dtype, unsigned flags, int row_leaf, bool count_only) {
    h->ctx = ctx; h->dtype = dtype; h->flags = flags; h->row_leaf = row_leaf; h->count_only = count_only; h->n_rays = 0; h->total = 0;
    h->rg_inst = REGION_INST_NONE;
    h->stats = bvhgpu_traverse_stats{0, 0, 0, 0, 0};
    h->pend_tree = nullptr; h->pend_rays = nullptr; h->pend_async = false;
    h->pend_wide = false; h->pend_staged = false; h->pend_rec8 = false; h->pend_guide = false; h->pend_qwide = false;
}

// The all-ascending bitonic network on len elements padded (virtually) to P = 2^k >= len; element e: key (kd[e * stride], kp[e]), payload
// ks[e].  First step of every merge mirrors, the others shift: every comparator leaves the smaller key at the lower index, so the slots
// between the row's length and P — (+inf, UINT32_MAX) by definition — never move and need no storage.  Every thread of the workgroup
// (ROWS_SORT_THREADS) calls it with the same len and P.  GLOBAL: the arrays are in global memory (a fence in front of the barrier).
template <typename T, bool GLOBAL>
__device__ __forceinline__ void rows_bitonic(T* kd, uint32_t stride, uint32_t* kp, uint32_t* ks, uint32_t len, uint32_t P) {
    const uint32_t half = P >> 1;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (uint32_t t = threadIdx.x; t < half; t += ROWS_SORT_THREADS) {
                const uint32_t lo = 2 * j * (t / j) + (t % j);
                const uint32_t hi = mirror ? 2 * j * (t / j) + (2 * j - 1 - (t % j)) : lo + j;
                if (hi < len) {   // (lo < hi; a slot beyond the row is the largest key: nothing to exchange)
                    const T dl = kd[(size_t)lo * stride], dh = kd[(size_t)hi * stride];
                    const uint32_t pl = kp[lo], ph = kp[hi];
                    if (dh < dl || (dh == dl && ph < pl)) {
                        kd[(size_t)lo * stride] = dh; kd[(size_t)hi * stride] = dl;
                        kp[lo] = ph; kp[hi] = pl;
                        const uint32_t sl = ks[lo], sh = ks[hi];
                        ks[lo] = sh; ks[hi] = sl;
                    }
                }
            }
            if (GLOBAL) __threadfence_block();
            __syncthreads();
        }
    }
}

// ---- the host schedule of a batch with a sort (all-hits, within and their instances forms) ---------------------------------------------------
// What a family's launches are handed: the CSR's columns in the result object (instance, list_shape and pos are NULL where the batch has
// none) and the worklist of the long rows.  vals is the family's T.
struct RowsOut {
    uint32_t *offsets, *instance, *shape;
    void* vals;
    uint32_t *list_shape, *pos;
    const uint32_t* work;
};
struct RowsPlan {
    bool sorted, count_only;        // rows sorted by key (else in list order); offsets and the total alone
    uint32_t lane_max, lds_max;     // the family's LANE_ROW_MAX / LDS_ROW_MAX
    size_t val_bytes;               // of one element's values
    bool with_instance, with_list;  // an instance column beside the shapes; the long rows' shapes wait in a scratch row for the sort
};

// count walk, scan, ONE host read, offsets, fill walk, a workgroup per long row (rows.hip has the stages).  count(counts) launches the
// family's count kernel, fill(out, std::true_type / std::false_type) its fill kernel in the SORTED / list-order instantiation,
// sort(out, n_long) its sort-row kernel.  h->offsets holds n + 1 words; sets h->total.
template <typename Count, typename Fill, typename Sort>
void rows_run(bvhgpu_hits* h, size_t n, const RowsPlan& p, Count&& count, Fill&& fill, Sort&& sort) {
    const bool rows_sorted = p.sorted && !p.count_only;
    count(rows_begin(h, n, rows_sorted));
    const RowsTotals rows = rows_scan(h, n, rows_sorted ? p.lane_max : 0u, p.lds_max);
    if (rows.total == 0) return;   // every row is empty
    rows_offsets(h, n);
    if (!p.count_only) {
        const size_t total = (size_t)rows.total;
        RowsOut o = {h->offsets.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, nullptr, h->rows_work.as<uint32_t>()};
        if (p.with_instance) { h->row_instance.reserve(total * 4); o.instance = h->row_instance.as<uint32_t>(); }
        h->indices.reserve(total * 4);
        h->row_vals.reserve(total * p.val_bytes);
        if (p.with_list && rows.n_long) { h->row_list_shape.reserve(total * 4); o.list_shape = h->row_list_shape.as<uint32_t>(); }
        if (rows.n_beyond_lds) { h->rows_pos.reserve(total * 4); o.pos = h->rows_pos.as<uint32_t>(); }
        o.shape = h->indices.as<uint32_t>();
        o.vals = h->row_vals.p;
        if (p.sorted) fill(o, std::true_type{});
        else fill(o, std::false_type{});
        // an instances family's sort-row kernel reads both scratch arrays without a test of its own
        if (p.sorted && ((p.with_list && rows.n_long && !o.list_shape) || (rows.n_beyond_lds && !o.pos))) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::None};
        if (p.sorted && rows.n_long) sort(o, rows.n_long);
    }
    BVH_HIP(hipGetLastError());
    h->total = rows.total;
}

// A whole synchronous batch of n queries into h: the result object becomes an empty result of the kind `flags` first, then `kernel` (the
// name bvhgpu_hits_walk_kernel reports) and the offsets are set — in this order: a reserve that throws leaves an empty result of the new
// kind, never the old kind's flags over a new buffer.  empty: no query can have a candidate (no shapes, no instances); else body() walks,
// through rows_run.  The result is complete when this returns.
template <typename Body>
void rows_batch(bvhgpu_hits* h, bvhgpu_ctx* ctx, int dtype, unsigned flags, int row_leaf, bool count_only, size_t n, bool empty, const char* kernel, Body&& body) {
    hipStream_t st = ctx->stream;
    rows_reset(h, ctx, dtype, flags, row_leaf, count_only);
    h->walk_kernel = kernel;
    h->offsets.reserve((n + 1) * 4);
    BVH_HIP(hipMemsetAsync(h->offsets.p, 0, 4, st));
    if (n == 0 || empty) BVH_HIP(hipMemsetAsync(h->offsets.p, 0, (n + 1) * 4, st));   // every row is empty
    else body();
    BVH_HIP(hipStreamSynchronize(st));
    h->n_rays = n;
    h->stats.hits = h->total;
}

}  // namespace bvhgpu
