// within.hip — every shape within max_dist of every query point of a batch, in order, as a CSR (bvhgpu_within_*; include/bvh_mi355x.h,
// DESIGN.md §4i).
//
// The definition is <FlatBvh as BoundingHierarchy>::nearest_to's loop (flat_bvh.rs:524-558) with the moving `best_dist` replaced by a
// fixed limit.  Point p_i comes with m = max_dist[i] in the tree's dtype T; r2 = m * m is ONE multiplication in T.  A negative or NaN m
// (!(m >= 0)) gives an empty row without a walk.
//   i = 0
//   while i < len(flat):
//     non-leaf entry: md = aabb.min_distance_squared(p);  i = (md <= r2) ? entry_index : exit_index
//     leaf entry:     d  = shape.distance_squared(p);     if d <= r2: candidate (d, shape);  i = exit_index
// shape.distance_squared is kind 0, the shape's own Aabb::min_distance_squared, or kind 1, the triangle (point_dist.hpp, unchanged: the
// bits of k_knearest).  Every comparison is T's <= as written, so the limit itself is inside: m = 0 keeps the shapes at distance 0,
// m = +inf (r2 = +inf) keeps every shape whose distance is not NaN, and a NaN d is never a candidate — a candidate's key is never NaN and
// the sorted order below is a total order.  aabb_min_dist2 ends every axis with max(0), which turns NaN into 0: a NaN coordinate of the
// point contributes 0 on its axis to every box distance (a point that is all NaN is at distance 0 of every box), an infinite coordinate
// gives +inf against a finite box (entered only with m = +inf) and, against a box that is infinite on that axis, NaN -> 0.  The triangle
// distance has no such guard: a NaN or infinite point gives it NaN (never a candidate) or +inf.
//   Row i, default: ALL candidates in a stable ascending sort by d; equal d stay in the order the loop met them (leaf pre-order).  The
//   output distance is sqrt(d), as in the k-nearest rows.
//   Row i with BVHGPU_WITHIN_LIST_ORDER: the candidates in the order the loop met them, no sort pass.
//   BVHGPU_WITHIN_COUNT_ONLY: only `offsets` (and the total); the fill and sort passes do not run.
// The threshold never moves, so the candidate set does not depend on the order a walk visits nodes in: it is "every box on the shape's
// path passes md <= r2 and the shape passes d <= r2".  Nearest-first descent buys nothing here; the 32 / 64-byte `trav` entries are the
// array to walk.
//
// The batch is rows.hip's schedule (count walk, scan, ONE host read, offsets, fill walk, a workgroup per long row) with a point per
// lane; every walk is k_knearest's loop (within_walk), and no walk has a cross-lane operation.  What this family puts into it:
//   k_within_count       counts[q] = the candidates of point q (lanes with a negative or NaN limit do not walk)
//   k_within_fill        A row of a sorted batch up to WITHIN_LANE_ROW_MAX is built by k_knearest's insertion (search from the back with
//                        the strict <: stable) on its own region — the key of element e lives in dist[e] — and a final per-lane pass
//                        turns the keys into sqrt.  A LIST_ORDER row gets (shape, sqrt(d)) appended as the walk meets them.  A longer row
//                        of a sorted batch gets (d, shape) appended in list order (and its positions, beyond WITHIN_LDS_ROW_MAX) and is
//                        left to
//   k_within_sort_row    rows_bitonic on the keys (d, position) with the shape as payload, in LDS up to WITHIN_LDS_ROW_MAX elements, in
//                        place in global memory beyond; then sqrt.
// The row length is uniform per workgroup of k_within_sort_row: every loop bound and every barrier there depends on it alone.
//
// Which array is walked.  `trav` folds a leaf's navigator entry and its leaf entry into one entry that carries the shape's own box: for
// a tree built here that box is bit-identical to the navigator box — except below a split without SAH winner (t->exact_only), whose two
// child boxes are Aabb::empty().  min_distance_squared of the empty box is 0 for every point (NaN -> 0 on every axis), so the reference
// enters such a leaf whatever the point, while the folded entry would test the shape's box.  With kind 0 that is the same decision (d IS
// that box distance); with kind 1 it is not where rounding puts the box distance above the triangle distance (a point on a vertex,
// m = 0).  A built tree with such a split is therefore walked over an unfolded mirror of its FlatNode array (k_within_unfold, written into
// the result object per batch; query.hip walks the FlatNode array itself for the same reason), with the UNFOLDED rule.
//
// The sphere kind (bvhgpu_within_sphere_*): shape.distance_squared is point_dist.hpp's sphere_dist2 on the shape's sphere —
// NaN for a NaN point or sphere, hence never a candidate.  It is not the box distance either, so it takes kind 1's rule for the array
// (the mirror above).  Nodes are pruned by their boxes: a sphere that reaches outside its shape's box can be missed.
#ifndef WITHIN_KERNEL_TEXT
#include <cstdio>

#include "point_dist.hpp"
#include "rows.hpp"
#include "unfold.hpp"   // k_within_unfold (shared with region.hip)

namespace bvhgpu {

// Thresholds (rows.hpp): allhits.hip's values.  DESIGN.md §4i: on radius rows of about 20 and 200 a lane tier ending at 8 or at 128 is slower than
// 32; the LDS limit has not been varied (no measured row comes near it).  WITHIN_LANE_ROW_MAX: a lane's insertion into global memory costs up to len^2 / 2
// element moves that no other lane of the wave shares.  WITHIN_LDS_ROW_MAX: 2048 x (8 + 4 + 4) bytes = 32 KB in f64, 24 KB in f32 — five
// (six) workgroups share a CU's 160 KB of LDS.
#ifndef BVH_WITHIN_LANE_ROW_MAX   // (developer builds, build_ext.py --variant: tools/within_bench.py against other thresholds)
#define BVH_WITHIN_LANE_ROW_MAX 32
#endif
#ifndef BVH_WITHIN_LDS_ROW_MAX
#define BVH_WITHIN_LDS_ROW_MAX 2048
#endif
constexpr uint32_t WITHIN_LANE_ROW_MAX = BVH_WITHIN_LANE_ROW_MAX;
constexpr uint32_t WITHIN_LDS_ROW_MAX = BVH_WITHIN_LDS_ROW_MAX;
static_assert(rows_lds_row_max_ok(WITHIN_LDS_ROW_MAX), "a row sorted in LDS must fit a workgroup's LDS, padded to a power of two");

template <typename T> struct WithinPoint {
    T p[3], r2;
    bool walk;   // the limit is neither negative nor NaN
    __device__ __forceinline__ void load(const T* __restrict__ points, const T* __restrict__ max_dist, uint32_t q) {
        for (int c = 0; c < 3; c++) p[c] = points[3 * (size_t)q + c];
        const T m = max_dist[q];
        r2 = m * m;
        walk = m >= (T)0;
    }
};

// k_knearest's loop with the fixed threshold: on_candidate(shape, d) for every shape the definition keeps, in the order it meets them
// KIND: the shape distance — 0 the shape's box, 1 its triangle, 2 its sphere; `prims` is the array of that kind (not read for the box)
template <typename T, int KIND, bool UNFOLDED, typename F>
__device__ __forceinline__ void within_walk(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ shape_aabbs,
                                            const T* __restrict__ prims, const WithinPoint<T>& pt, F&& on_candidate) {
    uint32_t i = 0;
    while (i < n_trav) {
        const NodeRegs<T> nd = load_node(nodes + i);
        const bool leaf = trav_is_leaf(nd.shape);
        bool enter = true;
        if (!(UNFOLDED && leaf)) {   // (a leaf entry of an unfolded array has no navigator test)
            const T md = aabb_min_dist2<T>(nd.mn, nd.mx, pt.p);
            enter = md <= pt.r2;
        }
        if (leaf) {
            if (enter) {
                T d;
                if (KIND == 2) d = sphere_dist2<T>(prims + 4 * (size_t)nd.shape, pt.p);
                else if (KIND == 1) d = triangle_dist2<T>(prims + 9 * (size_t)nd.shape, pt.p);
                else {
                    const T* sb = shape_aabbs + 6 * (size_t)nd.shape;
                    const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
                    d = aabb_min_dist2<T>(mn, mx, pt.p);
                }
                if (d <= pt.r2) on_candidate(nd.shape, d);
            }
            i = nd.exit;
        } else {
            i = enter ? i + 1 : nd.exit;
        }
    }
}

// The text of the two walk kernels stands at the end of this file, behind WITHIN_KERNEL_TEXT, and is compiled twice by the two includes of
// this file below (knn.hip's arrangement): as k_within_count<T, TRIANGLE, UNFOLDED> and k_within_fill<T, TRIANGLE, UNFOLDED,
// SORTED>, names, template heads and instructions as they were, and as k_within_count_sphere<T, UNFOLDED> and k_within_fill_sphere<T,
// UNFOLDED, SORTED>.  The sort pass reads keys only and serves every kind.
#define WITHIN_KERNEL_TEXT
#define POINT_K(name) name
#define POINT_KIND_TPARAM bool TRIANGLE,
#define POINT_KIND_VALUE (TRIANGLE ? 1 : 0)
#include "within.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#define POINT_K(name) name##_sphere
#define POINT_KIND_TPARAM
#define POINT_KIND_VALUE 2
#include "within.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#undef WITHIN_KERNEL_TEXT

// one workgroup per long row of a sorted batch
template <typename T>
__global__ __launch_bounds__(ROWS_SORT_THREADS) void k_within_sort_row(const uint32_t* __restrict__ work, const uint32_t* __restrict__ offsets,
                                                                         uint32_t* shape, T* dist, uint32_t* pos) {
    __shared__ T ld[WITHIN_LDS_ROW_MAX];
    __shared__ uint32_t lp[WITHIN_LDS_ROW_MAX];
    __shared__ uint32_t ls[WITHIN_LDS_ROW_MAX];
    const uint32_t q = work[blockIdx.x];
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;   // uniform over the workgroup
    uint32_t P = 1;
    while (P < len) P <<= 1;
    uint32_t* rs = shape + beg;
    T* rd = dist + beg;
    if (len <= WITHIN_LDS_ROW_MAX) {
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) { ld[e] = rd[e]; lp[e] = e; ls[e] = rs[e]; }
        __syncthreads();
        rows_bitonic<T, false>(ld, 1u, lp, ls, len, P);
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) { rd[e] = sqrt(ld[e]); rs[e] = ls[e]; }
    } else if (pos != nullptr) {   // (the host passes the positions whenever a row is this long)
        __threadfence_block();
        __syncthreads();
        rows_bitonic<T, true>(rd, 1u, pos + beg, rs, len, P);
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) rd[e] = sqrt(rd[e]);   // (the network ended with a barrier)
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int KIND, bool UNFOLDED>
static void within_launch(bvhgpu_tree* t, const TravNode<T>* nodes, uint32_t n_trav, const T* points_dev, const T* max_dist_dev, size_t n, bool sorted,
                          bool count_only, bvhgpu_hits* h) {
    hipStream_t st = t->ctx->stream;
    const T* aabbs = t->aabbs.as<T>();
    const T* prims = KIND == POINT_KIND_SPHERE ? t->spheres.as<T>() : t->tris.as<T>();
    const uint32_t n32 = (uint32_t)n;
    const dim3 pgrid((unsigned)((n + 255) / 256)), block(256);
    const RowsPlan plan = {sorted, count_only, WITHIN_LANE_ROW_MAX, WITHIN_LDS_ROW_MAX, sizeof(T), false, false};
    rows_run(h, n, plan,
             [&](uint32_t* counts) {
                 if constexpr (KIND == POINT_KIND_SPHERE)
                     hipLaunchKernelGGL((k_within_count_sphere<T, UNFOLDED>), pgrid, block, 0, st, nodes, n_trav, aabbs, prims, points_dev, max_dist_dev, n32, counts);
                 else
                     hipLaunchKernelGGL((k_within_count<T, KIND == 1, UNFOLDED>), pgrid, block, 0, st, nodes, n_trav, aabbs, prims, points_dev, max_dist_dev, n32, counts);
             },
             [&](const RowsOut& o, auto SORTED) {
                 if constexpr (KIND == POINT_KIND_SPHERE)
                     hipLaunchKernelGGL((k_within_fill_sphere<T, UNFOLDED, decltype(SORTED)::value>), pgrid, block, 0, st, nodes, n_trav, aabbs, prims, points_dev,
                                        max_dist_dev, n32, o.offsets, o.shape, static_cast<T*>(o.vals), o.pos);
                 else
                     hipLaunchKernelGGL((k_within_fill<T, KIND == 1, UNFOLDED, decltype(SORTED)::value>), pgrid, block, 0, st, nodes, n_trav, aabbs, prims, points_dev,
                                        max_dist_dev, n32, o.offsets, o.shape, static_cast<T*>(o.vals), o.pos);
             },
             [&](const RowsOut& o, uint32_t n_long) {
                 hipLaunchKernelGGL((k_within_sort_row<T>), dim3(n_long), dim3(ROWS_SORT_THREADS), 0, st, o.work, o.offsets, o.shape, static_cast<T*>(o.vals), o.pos);
             });
}

template <typename T>
void within_batch(bvhgpu_tree* t, const T* points_dev, const T* max_dist_dev, size_t n, int kind, unsigned flags, bvhgpu_hits* h) {
    const bool count_only = (flags & BVHGPU_WITHIN_COUNT_ONLY) != 0;
    const bool sorted = (flags & BVHGPU_WITHIN_LIST_ORDER) == 0;
    const bool mirror = t->exact_only && t->built && !t->unfolded && t->n >= 2;   // (see "Which array is walked" at the top)
    const bool unfolded = t->unfolded || t->n == 1 || mirror;   // a single-shape tree has one (leaf) entry and no navigator
    char name[112];
    const char* tri = kind == 1 ? "true" : "false";
    const char* unf = unfolded ? "true" : "false";
    if (kind == POINT_KIND_SPHERE) {
        if (count_only) std::snprintf(name, sizeof name, "bvhgpu::k_within_count_sphere<%s, %s>", walk_type_name<T>(), unf);
        else std::snprintf(name, sizeof name, "bvhgpu::k_within_fill_sphere<%s, %s, %s>", walk_type_name<T>(), unf, sorted ? "true" : "false");
    } else if (count_only) std::snprintf(name, sizeof name, "bvhgpu::k_within_count<%s, %s, %s>", walk_type_name<T>(), tri, unf);
    else std::snprintf(name, sizeof name, "bvhgpu::k_within_fill<%s, %s, %s, %s>", walk_type_name<T>(), tri, unf, sorted ? "true" : "false");
    rows_batch(h, t->ctx, Traits<T>::dtype, TRAVERSE_WITHIN, 0, count_only, n, t->n == 0, name, [&] {   // (empty: an empty hierarchy)
        hipStream_t st = t->ctx->stream;
        ensure_flat_arrays(t);
        const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
        uint32_t n_trav = (uint32_t)t->n_trav;
        if (mirror) {
            n_trav = (uint32_t)t->n_flat;
            h->unfold.reserve((size_t)n_trav * sizeof(TravNode<T>));
            hipLaunchKernelGGL((k_within_unfold<T>), dim3((n_trav + 255) / 256), dim3(256), 0, st, t->flat.as<typename Traits<T>::Flat>(), n_trav,
                               h->unfold.as<TravNode<T>>());
            BVH_HIP(hipGetLastError());
            nodes = h->unfold.as<TravNode<T>>();
        }
#define WITHIN_LAUNCH(KIND) do { if (unfolded) within_launch<T, KIND, true>(t, nodes, n_trav, points_dev, max_dist_dev, n, sorted, count_only, h); \
                                 else within_launch<T, KIND, false>(t, nodes, n_trav, points_dev, max_dist_dev, n, sorted, count_only, h); } while (0)
        if (kind == POINT_KIND_SPHERE) WITHIN_LAUNCH(POINT_KIND_SPHERE);
        else if (kind == 1) WITHIN_LAUNCH(1);
        else WITHIN_LAUNCH(0);
#undef WITHIN_LAUNCH
    });
}
template void within_batch<float>(bvhgpu_tree*, const float*, const float*, size_t, int, unsigned, bvhgpu_hits*);
template void within_batch<double>(bvhgpu_tree*, const double*, const double*, size_t, int, unsigned, bvhgpu_hits*);

}  // namespace bvhgpu

#else   // WITHIN_KERNEL_TEXT: the text of the walk kernels, inside namespace bvhgpu (see the includes of this file above)

template <typename T, POINT_KIND_TPARAM bool UNFOLDED>
__global__ __launch_bounds__(256) void POINT_K(k_within_count)(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ shape_aabbs,
                                                      const T* __restrict__ prims, const T* __restrict__ points,
                                                      const T* __restrict__ max_dist, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    WithinPoint<T> pt;
    pt.load(points, max_dist, q);
    uint32_t cnt = 0;
    if (pt.walk) within_walk<T, POINT_KIND_VALUE, UNFOLDED>(nodes, n_trav, shape_aabbs, prims, pt, [&](uint32_t, T) { cnt++; });
    counts[q] = cnt;
}

// ---- the second walk ----------------------------------------------------------------------------------------------------------------
// pos: NULL, or total u32 — the list positions of the rows beyond WITHIN_LDS_ROW_MAX (a sorted batch that has such rows)
template <typename T, POINT_KIND_TPARAM bool UNFOLDED, bool SORTED>
__global__ __launch_bounds__(256) void POINT_K(k_within_fill)(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ shape_aabbs,
                                                     const T* __restrict__ prims, const T* __restrict__ points, const T* __restrict__ max_dist,
                                                     uint32_t n, const uint32_t* __restrict__ offsets, uint32_t* __restrict__ shape,
                                                     T* __restrict__ dist, uint32_t* __restrict__ pos) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;
    if (len == 0) return;   // (the count pass walked this point, or refused its limit: nothing to write)
    WithinPoint<T> pt;
    pt.load(points, max_dist, q);
    uint32_t* __restrict__ rs = shape + beg;
    T* __restrict__ rd = dist + beg;
    const bool insert = SORTED && len <= WITHIN_LANE_ROW_MAX;
    const bool with_pos = SORTED && pos != nullptr && len > WITHIN_LDS_ROW_MAX;
    uint32_t cnt = 0;
    within_walk<T, POINT_KIND_VALUE, UNFOLDED>(nodes, n_trav, shape_aabbs, prims, pt, [&](uint32_t s, T d) {
        if (cnt >= len) return;   // (never: this walk is the count pass's; a lane stays inside its own region whatever happens)
        if (insert) {
            // ascending list: the first element e with d < e is where a scan from the back stops, so search and shift are one loop
            uint32_t hole = cnt;
#pragma unroll 1
            while (hole > 0) {
                const T e = rd[hole - 1];
                if (!(d < e)) break;
                rd[hole] = e;
                rs[hole] = rs[hole - 1];
                hole--;
            }
            rd[hole] = d;
            rs[hole] = s;
        } else if (SORTED) {   // a long row: (d, shape) in list order for k_within_sort_row
            rd[cnt] = d;
            rs[cnt] = s;
            if (with_pos) pos[beg + cnt] = cnt;
        } else {               // list order: the distance as the walk meets it
            rd[cnt] = sqrt(d);
            rs[cnt] = s;
        }
        cnt++;
    });
    if (insert) {
#pragma unroll 1
        for (uint32_t j = 0; j < cnt; j++) rd[j] = sqrt(rd[j]);
    }
}

#endif   // WITHIN_KERNEL_TEXT
