// rows.hpp — what the batches share whose result is one variable-length sorted row per query (allhits.hip, within.hip): the scan of the
// per-query counts into CSR offsets (rows.hip), the sort network of the long rows, and the empty result such a batch starts from.
#pragma once

#include "engine.hpp"

namespace bvhgpu {

constexpr uint32_t ROWS_SORT_THREADS = 256;   // workgroup of a family's k_*_sort_row
constexpr uint32_t ROWS_SCAN_ITEMS = 4;
constexpr uint32_t ROWS_SCAN_BLOCK = 256 * ROWS_SCAN_ITEMS;   // counts per workgroup of the scan

// A family keeps its own thresholds (rows up to LANE_ROW_MAX are sorted by the lane that fills them, up to LDS_ROW_MAX in LDS, longer
// ones in global memory) and hands them to the scan as arguments.  Its LDS_ROW_MAX has to pass this: a row sorted in LDS fits a
// workgroup's LDS (an f64 key, a position and a shape per element), and the LDS tier pads a row to a power of two inside its arrays
constexpr bool rows_lds_row_max_ok(uint32_t m) { return m * (sizeof(double) + 8u) <= 64u * 1024u && (m & (m - 1)) == 0; }

// rows.hip: the scan around a family's two walks, on h->ctx's stream, in h->ah_counts / ah_sums / ah_work.  In order:
//   rows_begin    reserves the three buffers (ah_work only with_work: a sorted batch) and zeroes the scan's meta words; returns the
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

// the result object becomes an (empty) rows result of the kind `flags` (TRAVERSE_ALLHITS / TRAVERSE_WITHIN): whatever fails behind this
// leaves it consistent
inline void rows_reset(bvhgpu_hits* h, bvhgpu_ctx* ctx, int dtype, unsigned flags, int ah_leaf, bool wi_count_only) {
    h->ctx = ctx; h->dtype = dtype; h->flags = flags; h->ah_leaf = ah_leaf; h->wi_count_only = wi_count_only; h->n_rays = 0; h->total = 0;
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

}  // namespace bvhgpu
