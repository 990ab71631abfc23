// allhits.hip — every hit of every ray of a batch, in order, as a CSR (bvhgpu_traverse_allhits_*; include/bvh_mi355x.h).
//
// The definition is khits.hip's without the cut to k: ray i has the list L_i = FlatBvh::traverse(&ray_i, shapes) (the engine's CSR row) and
// a segment end tmax[i] (NULL: +inf); the leaf stage LEAF gives every member s of L_i a record of W scalars whose first scalar is its
// DISTANCE (LEAF_BOX {enter, exit}, LEAF_TRIANGLE {distance, u, v}, LEAF_SPHERE {distance, exit}: khits.hip's records: walk.hpp's leaf_record is
// khits_record's text on the same operands, hence the same bits); s is a candidate iff distance < tmax[i], strict, in T.  Row i is ALL candidates of
// L_i in a stable ascending sort by distance — or, with BVHGPU_ALLHITS_LIST_ORDER, in the order of L_i.  A candidate's distance is never
// NaN (khits.hip's argument), so the sorted order is the total order on (distance, position in L_i): it is unique whatever produces it.
// No pruning: both walks visit all of L_i (§4e's inverted-box reason).
//
// The batch is rows.hip's schedule (count walk, scan, ONE host read, offsets, fill walk, a workgroup per long row); every walk is
// k_ray_khits' loop, one ray per lane (allhits_walk).  What this family puts into it:
//   k_allhits_count       counts[q] = the candidates of ray q
//   k_allhits_fill        A row of a sorted batch up to ALLHITS_LANE_ROW_MAX is built by k_ray_khits' insertion (search from the back with
//                         the strict <: stable) on its own region — the key of element e lives in vals[e * W] — and the whole records are
//                         then computed again from the ray and the shape.  A LIST_ORDER row gets its records appended as the walk meets
//                         them.  A longer row of a sorted batch gets (distance, shape) appended in list order (and its positions, beyond
//                         ALLHITS_LDS_ROW_MAX) and is left to
//   k_allhits_sort_row    rows_bitonic on the keys (distance, position) with the shape as payload, in LDS up to ALLHITS_LDS_ROW_MAX
//                         elements, in place in global memory beyond; then the records of the row.
// The row length is uniform per workgroup of k_allhits_sort_row: every loop bound and every barrier there depends on it alone.
#include <cstdio>

#include "rows.hpp"
#include "walk.hpp"

namespace bvhgpu {

// Thresholds.  ALLHITS_LANE_ROW_MAX: a lane's insertion into global memory costs up to len^2 / 2 element moves that no other lane of the
// wave shares; 32 keeps that below the cost of the walk itself on the scenes measured (§4h: rows there have at most 20 candidates).
// ALLHITS_LDS_ROW_MAX: 2048 x (8 + 4 + 4) bytes = 32 KB in f64, 24 KB in f32 — five (six) workgroups share a CU's 160 KB of LDS.
constexpr uint32_t ALLHITS_LANE_ROW_MAX = 32;
constexpr uint32_t ALLHITS_LDS_ROW_MAX = 2048;
static_assert(rows_lds_row_max_ok(ALLHITS_LDS_ROW_MAX), "a row sorted in LDS must fit a workgroup's LDS, padded to a power of two");

template <typename T, int LEAF> struct AllhitsRay {
    T o[3], d[3], inv[3], tmax;
    bool fast;   // the NaN-free slab test is exact for this ray (it returns no slice)
    __device__ __forceinline__ void load(const typename Traits<T>::Ray* rp, const T* __restrict__ tmaxs, uint32_t q) {
        for (int c = 0; c < 3; c++) { o[c] = rp->o[c]; inv[c] = rp->inv[c]; d[c] = LEAF != LEAF_BOX ? rp->d[c] : (T)0; }
        tmax = tmaxs ? tmaxs[q] : Traits<T>::inf();
        fast = LEAF != LEAF_BOX && ray_is_finite<T>(o, inv);
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
            if (LEAF != LEAF_BOX) {
                T rec[3];
                leaf_record<T, LEAF>(r.o, r.d, r.inv, prims, nd.shape, rec);
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

// ---- the second walk ----------------------------------------------------------------------------------------------------------------
// pos: NULL, or total u32 — the list positions of the rows beyond ALLHITS_LDS_ROW_MAX (a sorted batch that has such rows)
template <typename T, int LEAF, bool SORTED>
__global__ __launch_bounds__(256) void k_allhits_fill(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ prims,
                                                      const typename Traits<T>::Ray* __restrict__ rays, const T* __restrict__ tmaxs, uint32_t n,
                                                      const uint32_t* __restrict__ offsets, uint32_t* __restrict__ shape, T* __restrict__ vals,
                                                      uint32_t* __restrict__ pos) {
    constexpr uint32_t W = LeafVals<LEAF>::W;
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
            leaf_record<T, LEAF>(r.o, r.d, r.inv, prims, s, rec);
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
            leaf_record<T, LEAF>(r.o, r.d, r.inv, prims, rs[j], rec);
#pragma unroll
            for (uint32_t c = 0; c < W; c++) rv[(size_t)j * W + c] = rec[c];
        }
    }
}

// one workgroup per long row of a sorted batch
template <typename T, int LEAF>
__global__ __launch_bounds__(ROWS_SORT_THREADS) void k_allhits_sort_row(const uint32_t* __restrict__ work, const T* __restrict__ prims,
                                                                       const typename Traits<T>::Ray* __restrict__ rays,
                                                                       const uint32_t* __restrict__ offsets, uint32_t* shape, T* vals, uint32_t* pos) {
    constexpr uint32_t W = LeafVals<LEAF>::W;
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
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) { ld[e] = rv[(size_t)e * W]; lp[e] = e; ls[e] = rs[e]; }
        __syncthreads();
        rows_bitonic<T, false>(ld, 1u, lp, ls, len, P);
    } else if (pos != nullptr) {   // (the host passes the positions whenever a row is this long)
        __threadfence_block();
        __syncthreads();
        rows_bitonic<T, true>(rv, W, pos + beg, rs, len, P);
    }
    // the records of the row, from the ray and the sorted shapes (the network ended with a barrier)
    AllhitsRay<T, LEAF> r;
    r.load(rays + q, nullptr, q);
    for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) {
        const uint32_t s = in_lds ? ls[e] : rs[e];
        T rec[3];
        leaf_record<T, LEAF>(r.o, r.d, r.inv, prims, s, rec);
        if (in_lds) rs[e] = s;
#pragma unroll
        for (uint32_t c = 0; c < W; c++) rv[(size_t)e * W + c] = rec[c];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int LEAF>
static void allhits_launch(bvhgpu_tree* t, const T* prims, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, bool sorted, bvhgpu_hits* h) {
    hipStream_t st = t->ctx->stream;
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    const uint32_t n_trav = (uint32_t)t->n_trav, n32 = (uint32_t)n;
    const dim3 rgrid((unsigned)((n + 255) / 256)), block(256);
    const RowsPlan plan = {sorted, false, ALLHITS_LANE_ROW_MAX, ALLHITS_LDS_ROW_MAX, LeafVals<LEAF>::W * sizeof(T), false, false};
    rows_run(h, n, plan,
             [&](uint32_t* counts) { hipLaunchKernelGGL((k_allhits_count<T, LEAF>), rgrid, block, 0, st, nodes, n_trav, prims, rays_dev, tmax_dev, n32, counts); },
             [&](const RowsOut& o, auto SORTED) {
                 hipLaunchKernelGGL((k_allhits_fill<T, LEAF, decltype(SORTED)::value>), rgrid, block, 0, st, nodes, n_trav, prims, rays_dev, tmax_dev, n32, o.offsets,
                                    o.shape, static_cast<T*>(o.vals), o.pos);
             },
             [&](const RowsOut& o, uint32_t n_long) {
                 hipLaunchKernelGGL((k_allhits_sort_row<T, LEAF>), dim3(n_long), dim3(ROWS_SORT_THREADS), 0, st, o.work, prims, rays_dev, o.offsets, o.shape,
                                    static_cast<T*>(o.vals), o.pos);
             });
}

template <typename T>
void allhits_batch(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, int leaf, unsigned flags, bvhgpu_hits* h) {
    const bool sorted = (flags & BVHGPU_ALLHITS_LIST_ORDER) == 0;
    char name[96];
    std::snprintf(name, sizeof name, "bvhgpu::k_allhits_fill<%s, %d, %s>", walk_type_name<T>(), leaf, sorted ? "true" : "false");
    rows_batch(h, t->ctx, Traits<T>::dtype, TRAVERSE_ALLHITS, leaf, false, n, t->n == 0, name, [&] {   // (empty: an empty hierarchy)
        ensure_flat_arrays(t);
        if (leaf == LEAF_TRIANGLE) allhits_launch<T, LEAF_TRIANGLE>(t, (const T*)t->tris.as<T>(), rays_dev, tmax_dev, n, sorted, h);
        else if (leaf == LEAF_SPHERE) allhits_launch<T, LEAF_SPHERE>(t, (const T*)t->spheres.as<T>(), rays_dev, tmax_dev, n, sorted, h);
        else allhits_launch<T, LEAF_BOX>(t, (const T*)t->aabbs.as<T>(), rays_dev, tmax_dev, n, sorted, h);
    });
}
template void allhits_batch<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, const float*, size_t, int, unsigned, bvhgpu_hits*);
template void allhits_batch<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, const double*, size_t, int, unsigned, bvhgpu_hits*);

}  // namespace bvhgpu
