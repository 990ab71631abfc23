// csr.hip — the variable-length output of a batch (Vec<&Shape> per ray) as CSR: exclusive scan of the per-ray counts → offsets
// (reduce + rescan; a scan of the block sums in between for > 2 M rays), then indices[offsets[ray] + k] = shape (+ per-hit values)
// from the walk's hit pool, pair records or staged slots.  csr_enqueue runs these for traverse_enqueue (traverse.hip).
#include <type_traits>

#include "walk.hpp"

namespace bvhgpu {

// ---- exclusive scan of per-ray counts ----------------------------------------------------------

// KIND 1 (pair): every ray was walked as two items (k_traverse_lds split): its count is counts[2r] + counts[2r+1].
// KIND 2 (wide walk): counts[r] is non-zero only for rays with hits and ray_items[r] holds the set of the ray's items that
// reported some; k_scan_final copies that set to ray_mask[r] (for the scatter) and puts the zeros back, so both arrays are
// all zero again for the next batch (the walk then stores nothing for the rays — most of them on a sparse scene — that
// hit nothing).
template <int KIND> __device__ __forceinline__ uint32_t ray_count(const uint32_t* __restrict__ counts, uint32_t r) {
    if (KIND == COUNT_PLAIN || KIND == COUNT_MASKED) return counts[r];
    const uint2 c = reinterpret_cast<const uint2*>(counts)[r];
    return c.x + c.y;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_scan_reduce(const uint32_t* __restrict__ counts, uint32_t n,
                                                     unsigned long long* __restrict__ blocksums) {
    __shared__ unsigned long long ws[4];
    const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) s += (base + j < n) ? ray_count<KIND>(counts, base + j) : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if (lane_id() == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) blocksums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(1024) void k_scan_sums(unsigned long long* __restrict__ blocksums, uint32_t nb,
                                                    unsigned long long* __restrict__ total_out) {
    // exclusive scan of the block sums by ONE workgroup: every thread adds up a contiguous share serially, one 1024-wide scan over
    // the shares, every thread writes its share's prefixes.  (Round 2 looped a 256-wide Hillis-Steele scan with 16 barriers per 256
    // sums: 44 µs for the 2 442 sums of a 10 M-ray batch, 54 µs at 12.5 M — a tenth of the CSR assembly; this form takes ~5 µs.)
    __shared__ unsigned long long ws[16];
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    unsigned long long s = 0;
    for (uint32_t j = lo; j < hi; j++) s += blocksums[j];
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    unsigned long long inc = s;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    if (lane == WAVE - 1) ws[wv] = inc;
    __syncthreads();
    unsigned long long run = inc - s;
    for (int w2 = 0; w2 < wv; w2++) run += ws[w2];
    for (uint32_t j = lo; j < hi; j++) { const unsigned long long v = blocksums[j]; blocksums[j] = run; run += v; }
    if (threadIdx.x == 1023u) *total_out = run;   // (the last thread's running sum ends at the total, whether it owns sums or not)
}

// counts → offsets.  PREFIXED: blocksums already hold exclusive prefixes (k_scan_sums ran, large batches); otherwise
// they are the raw per-block sums of k_scan_reduce and this block adds up its predecessors (one kernel less).
template <int KIND, bool PREFIXED>
__global__ __launch_bounds__(256) void k_scan_final(const uint32_t* __restrict__ counts, uint32_t n,
                                                    const unsigned long long* __restrict__ blocksums,
                                                    unsigned long long* __restrict__ total,
                                                    uint32_t* __restrict__ offsets, uint32_t* __restrict__ ray_items,
                                                    uint16_t* __restrict__ ray_mask, unsigned long long* __restrict__ host_page,
                                                    unsigned long long* __restrict__ other_ctr, const uint32_t* __restrict__ scan_sums,
                                                    uint32_t* __restrict__ other_bsum, uint32_t bsum_cap) {
    __shared__ uint32_t ws[4];
    __shared__ unsigned long long wb[4];
    const uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    const int lane = lane_id();
    unsigned long long before = 0;
    if (PREFIXED) {
        before = blocksums[blockIdx.x];
    } else {
        unsigned long long part = 0;
        if (scan_sums) {   // the walk left the sums (u32) in this batch's set; the other set is zeroed here for the next batch
            for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) part += scan_sums[j];
            if (threadIdx.x == 0) other_bsum[blockIdx.x] = 0u;
            if (blockIdx.x == gridDim.x - 1)   // (a previous, larger batch may have left more behind)
                for (uint32_t j = gridDim.x + threadIdx.x; j < bsum_cap; j += 256) other_bsum[j] = 0u;
        } else {
            for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) part += blocksums[j];
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d);
        if (lane == 0) wb[threadIdx.x >> 6] = part;
    }
    uint32_t v[SCAN_ITEMS];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) { v[j] = (base + j < n) ? ray_count<KIND>(counts, base + j) : 0u; s += v[j]; }
    if (KIND == COUNT_MASKED) {   // rays with hits: keep the item mask for the scatter, zero the word for the next batch
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; j++) {
            if (v[j]) {
                if (ray_items) { ray_mask[base + j] = (uint16_t)ray_items[base + j]; ray_items[base + j] = 0u; }
                const_cast<uint32_t*>(counts)[base + j] = 0u;
            }
        }
    }
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        uint32_t u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    if (lane == WAVE - 1) ws[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (!PREFIXED) before = wb[0] + wb[1] + wb[2] + wb[3];
    uint32_t wbase = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) wbase += ws[w];
    uint32_t run = (uint32_t)before + wbase + inc - s;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; j++) {
        if (base + j < n) offsets[base + j] = run;
        run += v[j];
    }
    if (PREFIXED) {
        if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = (uint32_t)(*total);
    } else if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {   // the last block knows the total
        const unsigned long long t = before + ws[0] + ws[1] + ws[2] + ws[3];
        offsets[n] = (uint32_t)t;
        *total = t;
        // With the total every counter of the batch is final (the scatter only reads them): they go to the result's pinned
        // host page from here, and the OTHER counter set — the previous batch's, whose scatter is long done — is zeroed for
        // the next batch.  k_publish_counters as a launch of its own cost 3.8 µs per batch.  (total = ctr[3] of this set.)
        if (host_page) {
            const unsigned long long* ctr = total - 3;
#pragma unroll
            for (int k = 0; k < 8; k++) { host_page[k] = k == 3 ? t : ctr[k]; other_ctr[k] = 0ull; }
            __threadfence_system();
        }
    }
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void k_hits_scatter(const HitRec* __restrict__ pool, const T* __restrict__ pool_v,
                                                      const unsigned long long* __restrict__ ctr,
                                                      unsigned long long pool_cap, const uint32_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ pair_counts,
                                                      uint32_t* __restrict__ indices, T* __restrict__ vals) {
    const unsigned long long n = ctr[0];
    if (n > pool_cap) return;  // pool overflowed: indices[] is too small as well; the host grows both and replays
    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n;
         j += (unsigned long long)gridDim.x * blockDim.x) {
        const HitRec h = pool[j];
        if (h.ray == NONE) continue;   // unused tail of a per-wave chunk
        // pair_counts: h.ray is an ITEM (2*ray + side); the right item's records follow the left item's
        const uint32_t d = pair_counts ? offsets[h.ray >> 1] + ((h.ray & 1u) ? pair_counts[h.ray - 1] : 0u) + h.k
                                       : offsets[h.ray] + h.k;
        indices[d] = h.shape;
#pragma unroll
        for (int k = 0; k < NV; k++) vals[NV * (size_t)d + k] = pool_v[NV * j + k];
    }
}

// wide walk: a record's `ray` is an item (ray << 5 | j, or the ray itself with one item per ray); the records of item j follow
// those of the ray's earlier items that reported hits (ray_mask) — item_cnt is only valid for those
template <typename T, int NV, int ITEMS_LOG4>
__global__ __launch_bounds__(256) void k_hits_scatter_wide(const HitRec* __restrict__ pool, const T* __restrict__ pool_v,
                                                           const unsigned long long* __restrict__ ctr,
                                                           unsigned long long pool_cap, unsigned long long idx_cap, const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ item_cnt, const uint16_t* __restrict__ ray_mask,
                                                           uint32_t* __restrict__ indices, T* __restrict__ vals) {
    const unsigned long long n = ctr[0];
    if (n > pool_cap || ctr[3] > idx_cap) return;  // pool overflowed / more hits than indices[] holds: the host grows it and replays
    for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n;
         j += (unsigned long long)gridDim.x * blockDim.x) {
        const HitRec h = pool[j];
        if (h.ray == NONE) continue;   // unused tail of a per-wave chunk
        uint32_t d;
        if (ITEMS_LOG4 == 0) {
            d = offsets[h.ray] + h.k;
        } else {
            const uint32_t ray = h.ray >> WIDE_ITEM_BITS, it = h.ray & ((1u << WIDE_ITEM_BITS) - 1u);
            d = offsets[ray] + h.k;
            if (it) {
                const uint32_t mask = ray_mask[ray];
                for (uint32_t i = 0; i < it; i++)
                    if (mask & (1u << i)) d += item_cnt[((size_t)ray << (2 * ITEMS_LOG4)) + i];
            }
        }
        indices[d] = h.shape;
#pragma unroll
        for (int k = 0; k < NV; k++) vals[NV * (size_t)d + k] = pool_v[NV * j + k];
    }
}

// the pair records of a whole-ray index batch (WalkOut::pool_pair) → indices[offsets[ray] + k], + k + 1
__device__ __forceinline__ void scatter_pair_role(uint32_t block, uint32_t nblocks, const uint4* __restrict__ pool, const unsigned long long* __restrict__ ctr,
                                              unsigned long long pool_cap, unsigned long long idx_cap, const uint32_t* __restrict__ offsets,
                                              uint32_t* __restrict__ indices) {
    const unsigned long long n = ctr[0];
    if (n > pool_cap || ctr[3] > idx_cap) return;   // too small: the host grows and replays
    // SCATTER8_UNROLL records per thread and round, loads first: a record costs two dependent reads (the record, then its ray's offset)
    // and the kernel is latency-bound (PMC: 0.40 of the HBM rate, 82 % of wave-time waiting with one record in flight per thread)
    constexpr uint32_t U = SCATTER8_UNROLL;
    const unsigned long long span = (unsigned long long)blockDim.x * U;
    for (unsigned long long j0 = block * span + threadIdx.x; j0 < n; j0 += (unsigned long long)nblocks * span) {
        uint4 h[U];
        uint32_t o[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const unsigned long long j = j0 + (unsigned long long)u * blockDim.x;
            h[u] = j < n ? pool[j] : make_uint4(NONE, 0u, 0u, 0u);   // (NONE also marks the unused tail of a per-wave chunk)
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) o[u] = h[u].x != NONE ? offsets[h[u].x] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (h[u].x != NONE) {
                // both hits in ONE 8-byte store (dword alignment is all a global dwordx2 store needs).  The kernel is bound by its scattered
                // stores, not by the record or offset loads (configs[3] shard: 267 µs; loads alone 115; stores to computed addresses, no
                // offset gather, 270): −2 … −3 % of the assembly
                if (h[u].w != NONE) *reinterpret_cast<DwordPair*>(indices + o[u] + h[u].y) = DwordPair{h[u].z, h[u].w};
                else indices[o[u] + h[u].y] = h[u].z;
            }
    }
}
__global__ __launch_bounds__(256) void k_hits_scatter_pair(const uint4* __restrict__ pool, const unsigned long long* __restrict__ ctr,
                                                       unsigned long long pool_cap, unsigned long long idx_cap, const uint32_t* __restrict__ offsets,
                                                       uint32_t* __restrict__ indices) {
    scatter_pair_role(blockIdx.x, gridDim.x, pool, ctr, pool_cap, idx_cap, offsets, indices);
}

// Staged hits (WalkOut::raybuf) → CSR: one thread per ray copies the ray's first min(count, 2^shift) shapes from its own 2^shift-word
// slot to indices[offsets[ray] ..]: reads of whole 16-byte quads of the slot, writes that neighbouring threads make contiguous.  The later
// hits of a ray (k >= 2^shift) are pool records — pair records through k_hits_scatter_pair / k_hits_scatter8 (BVHGPU_TUNE_WIDE_REC8, the
// default), else 12-byte records through k_hits_scatter_wide.  Together they replace the
// 12-byte-record round trip (write, read, scatter) that cost configs[2] 0.42 ms for 58.8 M hits.  (Fusing this copy into
// k_scan_final — the thread that computes a ray's offset copies its shapes — was measured and dropped: four rays per thread
// break the contiguity of the writes, 0.31 ms against 0.13 + 0.03.)
#ifndef GATHER_RAYS
#define GATHER_RAYS 1
#endif
#ifndef BVH_GATHER_LDS
#define BVH_GATHER_LDS 1
#endif
template <int SHIFT>
__global__ __launch_bounds__(256) void k_hits_gather_staged(const uint32_t* __restrict__ raybuf, const uint32_t* __restrict__ offsets, uint32_t n_rays,
                                                            const unsigned long long* __restrict__ ctr, unsigned long long idx_cap,
                                                            uint32_t* __restrict__ indices) {
    constexpr uint32_t CAP = 1u << SHIFT, R = GATHER_RAYS;   // R rays per thread, their loads issued together (the copy is latency-bound: 0.49 of the HBM rate)
    if (ctr[3] > idx_cap) return;   // more hits than indices[] holds: the host grows it and replays
    uint32_t o0[R], cnt[R];
#pragma unroll
    for (uint32_t u = 0; u < R; u++) {
        const uint32_t r = (blockIdx.x * R + u) * blockDim.x + threadIdx.x;
        o0[u] = 0u; cnt[u] = 0u;
        if (r < n_rays) { o0[u] = offsets[r]; cnt[u] = offsets[r + 1] - o0[u]; }
    }
    uint32_t v[R][CAP];
#pragma unroll
    for (uint32_t u = 0; u < R; u++) {
        const uint32_t r = (blockIdx.x * R + u) * blockDim.x + threadIdx.x;
        const uint4* src = reinterpret_cast<const uint4*>(raybuf + ((size_t)r << SHIFT));
#pragma unroll
        for (uint32_t q = 0; q < CAP / 4; q++) {
            if (4u * q < cnt[u]) { const uint4 x = src[q]; v[u][4 * q] = x.x; v[u][4 * q + 1] = x.y; v[u][4 * q + 2] = x.z; v[u][4 * q + 3] = x.w; }
        }
    }
#if BVH_GATHER_LDS
    // The workgroup's rays are consecutive, so their CSR ranges form ONE contiguous span of indices[] (≈ 6 shapes x 256 rays = 6 KB on
    // configs[2]).  Written straight from the lanes, a store instruction scatters 64 dwords over that span and the L2 evicts partial
    // lines (PMC: 353 MB written for 165 MB of hits); staged through LDS the span goes out as whole 256-byte rows.  Positions k >= CAP
    // of a long ray are not the slot's: they are left out here and written by k_hits_scatter_pair (which runs behind this kernel).
    if (R == 1) {
        constexpr uint32_t SPAN_MAX = 4096;                     // entries of the staging buffer (16 KB); a denser workgroup stores directly
        __shared__ uint32_t s_out[SPAN_MAX];
        __shared__ uint32_t s_base, s_span;
        const uint32_t r0 = blockIdx.x * blockDim.x;
        if (threadIdx.x == 0) {
            const uint32_t r1 = min(r0 + blockDim.x, n_rays);
            s_base = r0 < n_rays ? offsets[r0] : 0u;
            s_span = r0 < n_rays ? offsets[r1] - s_base : 0u;
        }
        __syncthreads();
        const uint32_t base = s_base, span = s_span;
        if (span <= SPAN_MAX) {                                 // (workgroup-uniform)
            for (uint32_t p = threadIdx.x; p < span; p += blockDim.x) s_out[p] = NONE;
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < CAP; k++)
                if (k < cnt[0]) s_out[o0[0] - base + k] = v[0][k];
            __syncthreads();
            for (uint32_t p = threadIdx.x; p < span; p += blockDim.x) {
                const uint32_t x = s_out[p];
                if (x != NONE) indices[base + p] = x;           // (NONE: a long ray's later hits — k_hits_scatter_pair's)
            }
            return;
        }
    }
#endif
#pragma unroll
    for (uint32_t u = 0; u < R; u++) {
#pragma unroll
        for (uint32_t k = 0; k < CAP; k++)
            if (k < cnt[u]) indices[o0[u] + k] = v[u][k];
    }
}

// The 8 walk / scan counters go to the context's pinned host page and are zeroed for the next call: one 64-thread
// launch instead of the runtime's copy kernel plus its fill kernel (≈4.5 µs each on the stream).
__global__ void k_publish_counters(unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ host_page) {
    if (threadIdx.x < 8) {
        host_page[threadIdx.x] = ctr[threadIdx.x];
        ctr[threadIdx.x] = 0;
    }
    __threadfence_system();
}

void publish_counters(hipStream_t st, unsigned long long* ctr, unsigned long long* host_page) {
    hipLaunchKernelGGL(k_publish_counters, dim3(1), dim3(64), 0, st, ctr, host_page);
}

// counts → offsets → indices (+ values) of the batch whose walk has just been enqueued with `w`
template <typename T>
void csr_enqueue(bvhgpu_hits* h, size_t n_rays, const WalkOut<T>& w, const CsrArgs& a) {
    bvhgpu_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const bool use_wide = a.count_kind == COUNT_MASKED;
    unsigned long long* bs = h->blocksums.as<unsigned long long>();
    uint32_t* offs = h->offsets.as<uint32_t>();
    uint16_t* rmask = h->ray_mask.as<uint16_t>();
    uint32_t* ritems = (use_wide && a.items_log4) ? h->ray_items.as<uint32_t>() : nullptr;
    const uint32_t nr = (uint32_t)n_rays;
    auto scan = [&](auto kind_tag) {
        constexpr int KD = decltype(kind_tag)::value;
        if (!w.scan_sums) hipLaunchKernelGGL(k_scan_reduce<KD>, dim3(a.nb), dim3(256), 0, st, w.counts, nr, bs);
        if (a.nb > SCAN_FUSED_MAX_BLOCKS) {
            hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, bs, a.nb, w.ctr + 3);
            hipLaunchKernelGGL((k_scan_final<KD, true>), dim3(a.nb), dim3(256), 0, st, w.counts, nr, bs, w.ctr + 3, offs, ritems, rmask,
                               (unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
        } else {
            hipLaunchKernelGGL((k_scan_final<KD, false>), dim3(a.nb), dim3(256), 0, st, w.counts, nr, bs, w.ctr + 3, offs, ritems, rmask, a.pin, a.ctr_other,
                               (const uint32_t*)w.scan_sums, a.bsum_other, (uint32_t)SCAN_FUSED_MAX_BLOCKS);
        }
    };
    if (a.count_kind == COUNT_MASKED) scan(std::integral_constant<int, COUNT_MASKED>{});
    else if (a.count_kind == COUNT_PAIR) scan(std::integral_constant<int, COUNT_PAIR>{});
    else scan(std::integral_constant<int, COUNT_PLAIN>{});
    const uint32_t* pair_counts = a.count_kind == COUNT_PAIR ? w.counts : nullptr;
    const int sgrid = (int)std::min<size_t>((a.cap + 255) / 256, (size_t)ctx->n_cu * 8);
    T* vals = a.nv == 2 ? h->tslice.as<T>() : h->isect.as<T>();
    uint32_t* indices = h->indices.as<uint32_t>();
    if (a.stage_shift) {   // the rays' first 2^shift shapes, straight from their slots; the pool records (later hits) follow below
        const unsigned ggrid = (unsigned)((n_rays + 256 * GATHER_RAYS - 1) / (256 * GATHER_RAYS));
        const unsigned long long icap = h->idx_cap;
        switch (a.stage_shift) {
            case 2: hipLaunchKernelGGL(k_hits_gather_staged<2>, dim3(ggrid), dim3(256), 0, st, w.raybuf, offs, nr, w.ctr, icap, indices); break;
            case 3: hipLaunchKernelGGL(k_hits_gather_staged<3>, dim3(ggrid), dim3(256), 0, st, w.raybuf, offs, nr, w.ctr, icap, indices); break;
            case 4: hipLaunchKernelGGL(k_hits_gather_staged<4>, dim3(ggrid), dim3(256), 0, st, w.raybuf, offs, nr, w.ctr, icap, indices); break;
            default: hipLaunchKernelGGL(k_hits_gather_staged<5>, dim3(ggrid), dim3(256), 0, st, w.raybuf, offs, nr, w.ctr, icap, indices); break;
        }
    }
    if (a.rec8) {
        hipLaunchKernelGGL(k_hits_scatter_pair, dim3(sgrid), dim3(256), 0, st, w.pool_pair, w.ctr, a.cap, (unsigned long long)h->idx_cap, offs, indices);
    } else if (use_wide) {
        const uint32_t* icnt = h->item_cnt.as<uint32_t>();
#define SCATTER_WIDE(NV, L4) hipLaunchKernelGGL((k_hits_scatter_wide<T, NV, L4>), dim3(sgrid), dim3(256), 0, st, w.pool, w.pool_v, w.ctr, a.cap, (unsigned long long)h->idx_cap, offs, icnt, rmask, indices, vals)
        if (a.nv == 3) { if (a.items_log4 == 2) SCATTER_WIDE(3, 2); else if (a.items_log4 == 1) SCATTER_WIDE(3, 1); else SCATTER_WIDE(3, 0); }
        else { if (a.items_log4 == 2) SCATTER_WIDE(0, 2); else if (a.items_log4 == 1) SCATTER_WIDE(0, 1); else SCATTER_WIDE(0, 0); }
#undef SCATTER_WIDE
    } else if (a.nv == 2) {
        hipLaunchKernelGGL((k_hits_scatter<T, 2>), dim3(sgrid), dim3(256), 0, st, w.pool, w.pool_v, w.ctr, a.cap, offs, pair_counts, indices, vals);
    } else if (a.nv == 3) {
        hipLaunchKernelGGL((k_hits_scatter<T, 3>), dim3(sgrid), dim3(256), 0, st, w.pool, w.pool_v, w.ctr, a.cap, offs, pair_counts, indices, vals);
    } else {
        hipLaunchKernelGGL((k_hits_scatter<T, 0>), dim3(sgrid), dim3(256), 0, st, w.pool, w.pool_v, w.ctr, a.cap, offs, pair_counts, indices, vals);
    }
}
template void csr_enqueue<float>(bvhgpu_hits*, size_t, const WalkOut<float>&, const CsrArgs&);
template void csr_enqueue<double>(bvhgpu_hits*, size_t, const WalkOut<double>&, const CsrArgs&);

}  // namespace bvhgpu
