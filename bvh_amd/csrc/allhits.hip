// allhits.hip — every hit of every ray of a batch, in order, as a CSR (bvhgpu_traverse_allhits_*; include/bvh_mi355x.h).
//
// The definition is khits.hip's without the cut to k: ray i has the list L_i = FlatBvh::traverse(&ray_i, shapes) (the engine's CSR row) and
// a segment end tmax[i] (NULL: +inf); the leaf stage LEAF gives every member s of L_i a record of W scalars whose first scalar is its
// DISTANCE (AH_BOX {enter, exit}, AH_TRIANGLE {distance, u, v}, AH_SPHERE {distance, exit}: khits.hip's records, the same device
// functions on the same operands, hence the same bits); s is a candidate iff distance < tmax[i], strict, in T.  Row i is ALL candidates of
// L_i in a stable ascending sort by distance — or, with BVHGPU_ALLHITS_LIST_ORDER, in the order of L_i.  A candidate's distance is never
// NaN (khits.hip's argument), so the sorted order is the total order on (distance, position in L_i): it is unique whatever produces it.
// No pruning: both walks visit all of L_i (§4e's inverted-box reason).
//
// The batch is two walks with a scan between them; every walk is k_ray_khits' loop, one ray per lane (allhits_walk):
//   k_allhits_count       counts[q] = the candidates of ray q
//   k_allhits_block_sums  64-bit sum per block of ALLHITS_SCAN_BLOCK counts; the rays of a sorted batch whose rows are longer than
//                         ALLHITS_LANE_ROW_MAX are appended to the long-row worklist (any order), those above ALLHITS_LDS_ROW_MAX counted
//   k_allhits_scan_sums   exclusive scan of the block sums (one workgroup); the batch's 64-bit total
//   ... ONE host read {total, long rows, rows beyond LDS}: BVHGPU_OVERFLOW before anything is sized by the total ...
//   k_allhits_scan_final  offsets[q] = block base + exclusive scan inside the block, offsets[n] = total
//   k_allhits_fill        walks again; lane q owns [offsets[q], offsets[q + 1]).  A row of a sorted batch up to ALLHITS_LANE_ROW_MAX is
//                         built by k_ray_khits' insertion (search from the back with the strict <: stable) on its own region — the key of
//                         element e lives in vals[e * W] — and the whole records are then computed again from the ray and the shape.  A
//                         LIST_ORDER row gets its records appended as the walk meets them.  A longer row of a sorted batch gets (distance,
//                         shape) appended in list order (and its positions, beyond ALLHITS_LDS_ROW_MAX) and is left to
//   k_allhits_sort_row    one workgroup per long row: a bitonic network on the keys (distance, position) with the shape as payload, in LDS
//                         up to ALLHITS_LDS_ROW_MAX elements, in place in global memory beyond; then the records of the row.
// The network is the all-ascending form (first step of every merge mirrors, the others shift): every comparator leaves the smaller key at
// the lower index, so the slots between the row's length and the next power of two — (+inf, UINT32_MAX) by definition — never move and need
// no storage.  The row length is uniform per workgroup: every loop bound and every barrier below depends on it alone.
#include <cstdio>

#include "walk.hpp"

namespace bvhgpu {

enum : int { AH_BOX = BVHGPU_LEAF_BOX, AH_TRIANGLE = BVHGPU_LEAF_TRIANGLE, AH_SPHERE = BVHGPU_LEAF_SPHERE };

// Thresholds.  ALLHITS_LANE_ROW_MAX: a lane's insertion into global memory costs up to len^2 / 2 element moves that no other lane of the
// wave shares; 32 keeps that below the cost of the walk itself on the scenes measured (§4h: rows there have at most 20 candidates).
// ALLHITS_LDS_ROW_MAX: 2048 x (8 + 4 + 4) bytes = 32 KB in f64, 24 KB in f32 — five (six) workgroups share a CU's 160 KB of LDS.
constexpr uint32_t ALLHITS_LANE_ROW_MAX = 32;
constexpr uint32_t ALLHITS_LDS_ROW_MAX = 2048;
constexpr uint32_t ALLHITS_SORT_THREADS = 256;
constexpr uint32_t ALLHITS_SCAN_ITEMS = 4;
constexpr uint32_t ALLHITS_SCAN_BLOCK = 256 * ALLHITS_SCAN_ITEMS;   // counts per workgroup of the scan
static_assert(ALLHITS_LDS_ROW_MAX * (sizeof(double) + 8u) <= 64u * 1024u, "a row sorted in LDS must fit a workgroup's LDS");
static_assert((ALLHITS_LDS_ROW_MAX & (ALLHITS_LDS_ROW_MAX - 1)) == 0, "the LDS tier pads a row to a power of two inside its arrays");

// what the host reads between the scan and the fill (the first 16 bytes of the sums buffer)
struct AllhitsMeta { unsigned long long total; uint32_t n_long, n_beyond_lds; };

template <int LEAF> struct AllhitsVals { static constexpr uint32_t W = LEAF == AH_TRIANGLE ? 3u : 2u; };

// khits.hip khits_record: the record of shape s for the ray; prims is t->aabbs (n x 6), t->tris (n x 9) or t->spheres (n x 4) by LEAF
template <typename T, int LEAF>
__device__ __forceinline__ void allhits_record(const T o[3], const T d[3], const T inv[3], const T* __restrict__ prims, uint32_t s, T out[3]) {
    out[2] = 0;
    if (LEAF == AH_TRIANGLE) {
        ray_triangle<T>(o, d, prims + 9 * (size_t)s, out);
    } else if (LEAF == AH_SPHERE) {
        ray_sphere<T>(o, d, prims + 4 * (size_t)s, out);
    } else {
        const T* b = prims + 6 * (size_t)s;
        const T mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
        T t0, t1;
        const bool hit = slab_hit<T>(o, inv, mn, mx, t0, t1);
        out[0] = hit ? t0 : Traits<T>::inf(); out[1] = hit ? t1 : (T)0;
    }
}

template <typename T, int LEAF> struct AllhitsRay {
    T o[3], d[3], inv[3], tmax;
    bool fast;   // the NaN-free slab test is exact for this ray (it returns no slice)
    __device__ __forceinline__ void load(const typename Traits<T>::Ray* rp, const T* __restrict__ tmaxs, uint32_t q) {
        for (int c = 0; c < 3; c++) { o[c] = rp->o[c]; inv[c] = rp->inv[c]; d[c] = LEAF != AH_BOX ? rp->d[c] : (T)0; }
        tmax = tmaxs ? tmaxs[q] : Traits<T>::inf();
        fast = LEAF != AH_BOX && ray_is_finite<T>(o, inv);
    }
};

// k_ray_khits' loop: load_node, slab test, i = hit ? i + 1 : exit; on_candidate(shape, distance) for every member of L_i below tmax
template <typename T, int LEAF, typename F>
__device__ __forceinline__ void allhits_walk(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ prims, const AllhitsRay<T, LEAF>& r,
                                             F&& on_candidate) {
    uint32_t i = 0;
    while (i < n_trav) {
        const NodeRegs<T> nd = load_node(nodes + i);
        T t0 = 0, t1 = 0;
        const bool hit = r.fast ? slab_hit_finite<T>(r.o, r.inv, nd.mn, nd.mx) : slab_hit<T>(r.o, r.inv, nd.mn, nd.mx, t0, t1);
        if (hit && trav_is_leaf(nd.shape)) {
            T dist = t0;   // box: the leaf entry is the shape's own box
            if (LEAF != AH_BOX) {
                T rec[3];
                allhits_record<T, LEAF>(r.o, r.d, r.inv, prims, nd.shape, rec);
                dist = rec[0];
            }
            if (dist < r.tmax) on_candidate(nd.shape, dist);
        }
        i = hit ? i + 1 : nd.exit;   // a leaf's exit IS i+1
    }
}

template <typename T, int LEAF>
__global__ __launch_bounds__(256) void k_allhits_count(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ prims,
                                                       const typename Traits<T>::Ray* __restrict__ rays, const T* __restrict__ tmaxs, uint32_t n,
                                                       uint32_t* __restrict__ counts) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    AllhitsRay<T, LEAF> r;
    r.load(rays + q, tmaxs, q);
    uint32_t cnt = 0;
    allhits_walk<T, LEAF>(nodes, n_trav, prims, r, [&](uint32_t, T) { cnt++; });
    counts[q] = cnt;
}

// ---- the scan of the counts ---------------------------------------------------------------------------------------------------------
// sums[b] = the counts of block b, in 64 bits; the long rows of a sorted batch (lane_max != 0) go to the worklist
__global__ __launch_bounds__(256) void k_allhits_block_sums(const uint32_t* __restrict__ counts, uint32_t n, unsigned long long* __restrict__ sums,
                                                            AllhitsMeta* __restrict__ meta, uint32_t* __restrict__ work, uint32_t lane_max, uint32_t lds_max) {
    __shared__ unsigned long long part[256];
    const uint32_t base = blockIdx.x * ALLHITS_SCAN_BLOCK + threadIdx.x * ALLHITS_SCAN_ITEMS;
    unsigned long long s = 0;
    for (uint32_t j = 0; j < ALLHITS_SCAN_ITEMS; j++) {
        const uint32_t q = base + j;
        if (q < n) {   // (base + j cannot wrap: n < 2^32 - 1 and the grid covers n)
            const uint32_t c = counts[q];
            s += c;
            if (lane_max != 0 && c > lane_max) {
                work[atomicAdd(&meta->n_long, 1u)] = q;   // (at most n entries: one per ray)
                if (c > lds_max) atomicAdd(&meta->n_beyond_lds, 1u);
            }
        }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// one workgroup: sums[b] becomes the sum of the blocks in front of b; meta->total
__global__ __launch_bounds__(256) void k_allhits_scan_sums(unsigned long long* __restrict__ sums, uint32_t nb, AllhitsMeta* __restrict__ meta) {
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += 256) {   // (nb is uniform: every thread runs every barrier)
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long own = b < nb ? sums[b] : 0ull;
        part[threadIdx.x] = own;
        __syncthreads();
        for (uint32_t w = 1; w < 256; w <<= 1) {
            const unsigned long long add = threadIdx.x >= w ? part[threadIdx.x - w] : 0ull;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const unsigned long long carry = carry_s;
        if (b < nb) sums[b] = carry + part[threadIdx.x] - own;
        __syncthreads();
        if (threadIdx.x == 255) carry_s = carry + part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) meta->total = carry_s;
}

// offsets[q] for the block's counts (the host has checked that the total fits 32 bits)
__global__ __launch_bounds__(256) void k_allhits_scan_final(const uint32_t* __restrict__ counts, uint32_t n, const unsigned long long* __restrict__ sums,
                                                            const AllhitsMeta* __restrict__ meta, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * ALLHITS_SCAN_BLOCK + threadIdx.x * ALLHITS_SCAN_ITEMS;
    uint32_t c[ALLHITS_SCAN_ITEMS], own = 0;
    for (uint32_t j = 0; j < ALLHITS_SCAN_ITEMS; j++) {
        c[j] = base + j < n ? counts[base + j] : 0u;
        own += c[j];
    }
    part[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t w = 1; w < 256; w <<= 1) {
        const uint32_t add = threadIdx.x >= w ? part[threadIdx.x - w] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = (uint32_t)sums[blockIdx.x] + part[threadIdx.x] - own;
    for (uint32_t j = 0; j < ALLHITS_SCAN_ITEMS; j++) {
        if (base + j < n) offsets[base + j] = run;
        run += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = (uint32_t)meta->total;
}

// ---- the second walk ----------------------------------------------------------------------------------------------------------------
// pos: NULL, or total u32 — the list positions of the rows beyond ALLHITS_LDS_ROW_MAX (a sorted batch that has such rows)
template <typename T, int LEAF, bool SORTED>
__global__ __launch_bounds__(256) void k_allhits_fill(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ prims,
                                                      const typename Traits<T>::Ray* __restrict__ rays, const T* __restrict__ tmaxs, uint32_t n,
                                                      const uint32_t* __restrict__ offsets, uint32_t* __restrict__ shape, T* __restrict__ vals,
                                                      uint32_t* __restrict__ pos) {
    constexpr uint32_t W = AllhitsVals<LEAF>::W;
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;
    if (len == 0) return;   // (the count pass walked this ray: nothing to write)
    AllhitsRay<T, LEAF> r;
    r.load(rays + q, tmaxs, q);
    uint32_t* __restrict__ rs = shape + beg;
    T* __restrict__ rv = vals + (size_t)beg * W;
    const bool insert = SORTED && len <= ALLHITS_LANE_ROW_MAX;
    const bool with_pos = SORTED && pos != nullptr && len > ALLHITS_LDS_ROW_MAX;
    uint32_t cnt = 0;
    allhits_walk<T, LEAF>(nodes, n_trav, prims, r, [&](uint32_t s, T dist) {
        if (cnt >= len) return;   // (never: this walk is the count pass's; a lane stays inside its own region whatever happens)
        if (insert) {
            // ascending list: the first element e with dist < e is where a scan from the back stops, so search and shift are one loop
            uint32_t hole = cnt;
#pragma unroll 1
            while (hole > 0) {
                const T e = rv[(size_t)(hole - 1) * W];
                if (!(dist < e)) break;
                rv[(size_t)hole * W] = e;
                rs[hole] = rs[hole - 1];
                hole--;
            }
            rv[(size_t)hole * W] = dist;
            rs[hole] = s;
        } else if (SORTED) {   // a long row: (distance, shape) in list order for k_allhits_sort_row
            rv[(size_t)cnt * W] = dist;
            rs[cnt] = s;
            if (with_pos) pos[beg + cnt] = cnt;
        } else {               // list order: the record as the walk meets it
            T rec[3];
            allhits_record<T, LEAF>(r.o, r.d, r.inv, prims, s, rec);
            rs[cnt] = s;
#pragma unroll
            for (uint32_t c = 0; c < W; c++) rv[(size_t)cnt * W + c] = rec[c];
        }
        cnt++;
    });
    if (insert) {
        // the whole record of every element, computed again from the ray and the shape
#pragma unroll 1
        for (uint32_t j = 0; j < cnt; j++) {
            T rec[3];
            allhits_record<T, LEAF>(r.o, r.d, r.inv, prims, rs[j], rec);
#pragma unroll
            for (uint32_t c = 0; c < W; c++) rv[(size_t)j * W + c] = rec[c];
        }
    }
}

// the all-ascending bitonic network on len elements padded (virtually) to P = 2^k >= len; element e: key (kd[e * stride], kp[e]), payload ks[e].
// Every thread of the workgroup calls it with the same len and P.  GLOBAL: the arrays are in global memory (a fence in front of the barrier).
template <typename T, bool GLOBAL>
__device__ __forceinline__ void allhits_bitonic(T* kd, uint32_t stride, uint32_t* kp, uint32_t* ks, uint32_t len, uint32_t P) {
    const uint32_t half = P >> 1;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (uint32_t t = threadIdx.x; t < half; t += ALLHITS_SORT_THREADS) {
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

// one workgroup per long row of a sorted batch
template <typename T, int LEAF>
__global__ __launch_bounds__(ALLHITS_SORT_THREADS) void k_allhits_sort_row(const uint32_t* __restrict__ work, const T* __restrict__ prims,
                                                                          const typename Traits<T>::Ray* __restrict__ rays,
                                                                          const uint32_t* __restrict__ offsets, uint32_t* shape, T* vals, uint32_t* pos) {
    constexpr uint32_t W = AllhitsVals<LEAF>::W;
    __shared__ T ld[ALLHITS_LDS_ROW_MAX];
    __shared__ uint32_t lp[ALLHITS_LDS_ROW_MAX];
    __shared__ uint32_t ls[ALLHITS_LDS_ROW_MAX];
    const uint32_t q = work[blockIdx.x];
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;   // uniform over the workgroup
    uint32_t P = 1;
    while (P < len) P <<= 1;
    uint32_t* rs = shape + beg;
    T* rv = vals + (size_t)beg * W;
    const bool in_lds = len <= ALLHITS_LDS_ROW_MAX;
    if (in_lds) {
        for (uint32_t e = threadIdx.x; e < len; e += ALLHITS_SORT_THREADS) { ld[e] = rv[(size_t)e * W]; lp[e] = e; ls[e] = rs[e]; }
        __syncthreads();
        allhits_bitonic<T, false>(ld, 1u, lp, ls, len, P);
    } else if (pos != nullptr) {   // (the host passes the positions whenever a row is this long)
        __threadfence_block();
        __syncthreads();
        allhits_bitonic<T, true>(rv, W, pos + beg, rs, len, P);
    }
    // the records of the row, from the ray and the sorted shapes (the network ended with a barrier)
    AllhitsRay<T, LEAF> r;
    r.load(rays + q, nullptr, q);
    for (uint32_t e = threadIdx.x; e < len; e += ALLHITS_SORT_THREADS) {
        const uint32_t s = in_lds ? ls[e] : rs[e];
        T rec[3];
        allhits_record<T, LEAF>(r.o, r.d, r.inv, prims, s, rec);
        if (in_lds) rs[e] = s;
#pragma unroll
        for (uint32_t c = 0; c < W; c++) rv[(size_t)e * W + c] = rec[c];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int LEAF>
static void allhits_launch(bvhgpu_tree* t, const T* prims, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, bool sorted, bvhgpu_hits* h) {
    constexpr uint32_t W = AllhitsVals<LEAF>::W;
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    const uint32_t n_trav = (uint32_t)t->n_trav, n32 = (uint32_t)n;
    const dim3 rgrid((unsigned)((n + 255) / 256)), block(256);
    const uint32_t nb = (uint32_t)((n + ALLHITS_SCAN_BLOCK - 1) / ALLHITS_SCAN_BLOCK);
    h->ah_counts.reserve(n * 4);
    h->ah_sums.reserve(sizeof(AllhitsMeta) + (size_t)nb * sizeof(unsigned long long));
    if (sorted) h->ah_work.reserve(n * 4);
    AllhitsMeta* meta = h->ah_sums.as<AllhitsMeta>();
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(meta + 1);
    uint32_t* counts = h->ah_counts.as<uint32_t>();
    uint32_t* offsets = h->offsets.as<uint32_t>();
    BVH_HIP(hipMemsetAsync(meta, 0, sizeof(AllhitsMeta), st));
    hipLaunchKernelGGL((k_allhits_count<T, LEAF>), rgrid, block, 0, st, nodes, n_trav, prims, rays_dev, tmax_dev, n32, counts);
    hipLaunchKernelGGL(k_allhits_block_sums, dim3(nb), block, 0, st, counts, n32, sums, meta, h->ah_work.as<uint32_t>(), sorted ? ALLHITS_LANE_ROW_MAX : 0u,
                       ALLHITS_LDS_ROW_MAX);
    hipLaunchKernelGGL(k_allhits_scan_sums, dim3(1), block, 0, st, sums, nb, meta);
    BVH_HIP(hipGetLastError());
    AllhitsMeta* got = static_cast<AllhitsMeta*>(ctx->pinned);
    BVH_HIP(hipMemcpyAsync(got, meta, sizeof(AllhitsMeta), hipMemcpyDeviceToHost, st));
    BVH_HIP(hipStreamSynchronize(st));
    const unsigned long long total = got->total;
    const uint32_t n_long = got->n_long, n_beyond = got->n_beyond_lds;
    if (total > 0xFFFFFFFFull) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::Overflow};
    if (total == 0) {   // every row is empty
        BVH_HIP(hipMemsetAsync(offsets, 0, (n + 1) * 4, st));
        return;
    }
    h->indices.reserve((size_t)total * 4);
    h->ah_vals.reserve((size_t)total * W * sizeof(T));
    uint32_t* pos = nullptr;
    if (n_beyond) { h->ah_pos.reserve((size_t)total * 4); pos = h->ah_pos.as<uint32_t>(); }
    uint32_t* shape = h->indices.as<uint32_t>();
    T* vals = h->ah_vals.as<T>();
    hipLaunchKernelGGL(k_allhits_scan_final, dim3(nb), block, 0, st, counts, n32, sums, meta, offsets);
    if (sorted) hipLaunchKernelGGL((k_allhits_fill<T, LEAF, true>), rgrid, block, 0, st, nodes, n_trav, prims, rays_dev, tmax_dev, n32, offsets, shape, vals, pos);
    else hipLaunchKernelGGL((k_allhits_fill<T, LEAF, false>), rgrid, block, 0, st, nodes, n_trav, prims, rays_dev, tmax_dev, n32, offsets, shape, vals, pos);
    if (sorted && n_long)
        hipLaunchKernelGGL((k_allhits_sort_row<T, LEAF>), dim3(n_long), dim3(ALLHITS_SORT_THREADS), 0, st, h->ah_work.as<uint32_t>(), prims, rays_dev, offsets, shape,
                           vals, pos);
    BVH_HIP(hipGetLastError());
    h->total = total;
}

template <typename T>
void allhits_batch(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, int leaf, unsigned flags, bvhgpu_hits* h) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const bool sorted = (flags & BVHGPU_ALLHITS_LIST_ORDER) == 0;
    // the result object becomes an (empty) all-hits result first: whatever fails below leaves it consistent
    h->offsets.reserve((n + 1) * 4);
    h->ctx = ctx; h->dtype = Traits<T>::dtype; h->flags = TRAVERSE_ALLHITS; h->ah_leaf = leaf; h->n_rays = 0; h->total = 0;
    h->stats = bvhgpu_traverse_stats{0, 0, 0, 0, 0};
    h->pend_tree = nullptr; h->pend_rays = nullptr; h->pend_async = false;
    h->pend_wide = false; h->pend_staged = false; h->pend_rec8 = false; h->pend_guide = false; h->pend_qwide = false;
    char name[96];
    std::snprintf(name, sizeof name, "bvhgpu::k_allhits_fill<%s, %d, %s>", walk_type_name<T>(), leaf, sorted ? "true" : "false");
    h->walk_kernel = name;
    BVH_HIP(hipMemsetAsync(h->offsets.p, 0, 4, st));
    if (n == 0 || t->n == 0) {   // no rays, or an empty hierarchy: every row is empty
        BVH_HIP(hipMemsetAsync(h->offsets.p, 0, (n + 1) * 4, st));
    } else {
        ensure_flat_arrays(t);
        if (leaf == AH_TRIANGLE) allhits_launch<T, AH_TRIANGLE>(t, (const T*)t->tris.as<T>(), rays_dev, tmax_dev, n, sorted, h);
        else if (leaf == AH_SPHERE) allhits_launch<T, AH_SPHERE>(t, (const T*)t->spheres.as<T>(), rays_dev, tmax_dev, n, sorted, h);
        else allhits_launch<T, AH_BOX>(t, (const T*)t->aabbs.as<T>(), rays_dev, tmax_dev, n, sorted, h);
    }
    BVH_HIP(hipStreamSynchronize(st));   // the result is complete when the call returns
    h->n_rays = n;
    h->stats.hits = h->total;
}
template void allhits_batch<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, const float*, size_t, int, unsigned, bvhgpu_hits*);
template void allhits_batch<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, const double*, size_t, int, unsigned, bvhgpu_hits*);

}  // namespace bvhgpu
