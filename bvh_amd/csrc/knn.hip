// knn.hip — the k nearest shapes of every query point of a batch (bvhgpu_knearest_*).
//
// The reference has no k-nearest query; the engine defines it as the smallest change to <FlatBvh as BoundingHierarchy>::nearest_to
// (flat_bvh.rs:524-558): `best_element` becomes a list L of at most k pairs (dist2, shape), ascending.
//   full  = len(L) == k,  bound = L[last].dist2
//   navigator (:546-556): md = aabb.min_distance_squared(query); entry_index iff !full || md < bound, else exit_index
//   leaf      (:533-544): d = shape.distance_squared(query); accepted iff !full || d < bound.  An accepted candidate drops L[last] of a full
//                         list and goes in front of the first element e with d < e.dist2, or to the end when there is none; then exit_index
// Every comparison is the strict < of T: a NaN distance is accepted only while the list is not full, lands behind everything the list
// holds at that moment, and as L[last] of a full list it is never replaced (what nearest_to does with a NaN best_dist).  Rows without a NaN
// are ascending; equal distances stay in the order the walk met them (leaf pre-order).
// Output row i: shape[i][j] = L[j].shape, dist[i][j] = sqrt(L[j].dist2) (:561) for j < len(L); the other k - len(L) slots hold NONE and +inf.
//
// k_knearest: one query point per lane, the stackless walk of k_nearest (traverse.hip) over the folded array `trav`.  Per lane `len` and
// `bound` live in registers, so a step of the walk touches the list only when a candidate is accepted — rare once the list is full.  The
// list lives in LDS, dynamic size block x k x (sizeof(T) + 4) bytes from the ACTUAL k, slot-major: slot j of lane l is element j x block + l
// of two arrays (distances, then shapes).  A wave's access to one slot is 64 consecutive 4-byte (8-byte) words: conflict-free under both LDS
// banking rules.  A lane only ever touches its own column, so the kernel has no barrier.
// Block size: walk.hpp's topk_block.
// Shape distance: kind 0 the shape's own box, kind 1 its triangle (bvhgpu_knearest_*), or its sphere (bvhgpu_knearest_sphere_*, point_dist.hpp's
// sphere_dist2).  The nodes are pruned by their boxes whatever the kind, as the reference prunes any PointDistance shape by its
// Aabb.  The sphere distance is not the box distance, so the array is chosen by kind 1's rule: UNFOLDED for t->unfolded || t->n == 1.
#ifndef KNN_KERNEL_TEXT
#include "point_dist.hpp"

namespace bvhgpu {

static_assert(topk_fits(BVHGPU_KNN_MAX_K), "the k-nearest lists of 64 lanes must fit a workgroup's LDS");

// The kernel text stands at the end of this file, behind KNN_KERNEL_TEXT, and is compiled twice by the two includes of this file below
// (DESIGN.md §4t's way, §4u): once as k_knearest<T, TRIANGLE, UNFOLDED> — the same text under the same name and template head as before
// there was a sphere distance, hence the same instructions — and once as k_knearest_sphere<T, UNFOLDED>.  POINT_K(name): the kernel's
// name; POINT_KIND_TPARAM: the kind's place in its template head; POINT_KIND_VALUE: its shape distance, 0 box, 1 triangle, 2 sphere.
// `prims` is the array of that kind: the triangles (9 T per shape), the spheres (4 T per shape), not read for the box.
#define KNN_KERNEL_TEXT
#define POINT_K(name) name
#define POINT_KIND_TPARAM bool TRIANGLE,
#define POINT_KIND_VALUE (TRIANGLE ? 1 : 0)
#include "knn.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#define POINT_K(name) name##_sphere
#define POINT_KIND_TPARAM
#define POINT_KIND_VALUE 2
#include "knn.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#undef KNN_KERNEL_TEXT

// an empty hierarchy: every slot is padding (+inf is no byte pattern, so no memset)
template <typename T>
__global__ __launch_bounds__(256) void k_knn_fill(uint32_t* __restrict__ out_shape, T* __restrict__ out_dist, uint32_t total) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out_shape[e] = NONE;
    out_dist[e] = (T)INFINITY;
}

template <typename T>
void knearest_batch(bvhgpu_tree* t, const T* points_dev, size_t n, int kind, uint32_t k, uint32_t* out_shape_dev, T* out_dist_dev) {
    if (!n) return;
    hipStream_t st = t->ctx->stream;
    if (t->n == 0) {
        const size_t total = n * k;   // (the caller has checked n x k < 2^32)
        hipLaunchKernelGGL((k_knn_fill<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out_shape_dev, out_dist_dev, (uint32_t)total);
        BVH_HIP(hipGetLastError());
        return;
    }
    const unsigned bs = topk_block<T>(k);
    const dim3 grid((unsigned)((n + bs - 1) / bs)), block(bs);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 4);
    ensure_flat_arrays(t);
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    const uint32_t n_trav = (uint32_t)t->n_trav;
    const bool unfolded = t->unfolded || t->n == 1;   // a single-shape tree has one (leaf) entry and no navigator
#define LAUNCH_KNEAREST_K(K, PRIMS) hipLaunchKernelGGL(K, grid, block, lds, st, nodes, n_trav, t->aabbs.as<T>(), PRIMS, points_dev, (uint32_t)n, k, \
                                                      out_shape_dev, out_dist_dev)
#define LAUNCH_KNEAREST(TRI, UNF) LAUNCH_KNEAREST_K((k_knearest<T, TRI, UNF>), t->tris.as<T>())
    if (kind == POINT_KIND_SPHERE) {
        if (unfolded) LAUNCH_KNEAREST_K((k_knearest_sphere<T, true>), t->spheres.as<T>());
        else LAUNCH_KNEAREST_K((k_knearest_sphere<T, false>), t->spheres.as<T>());
    } else if (kind == 1) { if (unfolded) LAUNCH_KNEAREST(true, true); else LAUNCH_KNEAREST(true, false); }
    else { if (unfolded) LAUNCH_KNEAREST(false, true); else LAUNCH_KNEAREST(false, false); }
#undef LAUNCH_KNEAREST
#undef LAUNCH_KNEAREST_K
    BVH_HIP(hipGetLastError());
}
template void knearest_batch<float>(bvhgpu_tree*, const float*, size_t, int, uint32_t, uint32_t*, float*);
template void knearest_batch<double>(bvhgpu_tree*, const double*, size_t, int, uint32_t, uint32_t*, double*);

}  // namespace bvhgpu

#else   // KNN_KERNEL_TEXT: the kernel text, inside namespace bvhgpu (see the includes of this file above)

template <typename T, POINT_KIND_TPARAM bool UNFOLDED>
__global__ __launch_bounds__(256) void POINT_K(k_knearest)(const TravNode<T>* __restrict__ nodes, uint32_t n_trav,
                                                  const T* __restrict__ shape_aabbs, const T* __restrict__ prims,
                                                  const T* __restrict__ points, uint32_t n, uint32_t k, uint32_t* __restrict__ out_shape,
                                                  T* __restrict__ out_dist) {
    constexpr int KIND = POINT_KIND_VALUE;
    extern __shared__ __align__(16) unsigned char knn_lds[];
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(knn_lds) + threadIdx.x;                                        // slot j: ld[j * block]
    uint32_t* __restrict__ ls = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(knn_lds) + (size_t)k * block) + threadIdx.x;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    if (q >= n) return;
    const T p[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};
    uint32_t len = 0;
    bool full = false;       // len == k
    bool has_nan = false;    // the list holds a NaN: it need not be sorted any more
    T bound = 0;             // L[k - 1].dist2 of a full list
    uint32_t i = 0;
    while (i < n_trav) {
        const NodeRegs<T> nd = load_node(nodes + i);
        const bool leaf = trav_is_leaf(nd.shape);
        bool enter = true;
        if (!(UNFOLDED && leaf)) {
            const T md = aabb_min_dist2<T>(nd.mn, nd.mx, p);
            enter = !full || md < bound;
        }
        if (leaf) {
            if (enter) {
                T d;
                if (KIND == 2) d = sphere_dist2<T>(prims + 4 * (size_t)nd.shape, p);
                else if (KIND == 1) d = triangle_dist2<T>(prims + 9 * (size_t)nd.shape, p);
                else {
                    const T* sb = shape_aabbs + 6 * (size_t)nd.shape;
                    const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
                    d = aabb_min_dist2<T>(mn, mx, p);
                }
                if (!full || d < bound) {
                    uint32_t hole = full ? k - 1 : len;   // a full list drops its last element
                    uint32_t pos;                         // in front of the first element e with d < e
                    if (!has_nan) {
                        // ascending list: that element is where a scan from the back stops, so search and shift are one loop
#pragma unroll 1
                        while (hole > 0) {
                            const T e = ld[(hole - 1) * block];
                            if (!(d < e)) break;
                            ld[hole * block] = e;
                            ls[hole * block] = ls[(hole - 1) * block];
                            hole--;
                        }
                        pos = hole;
                    } else {
                        // a NaN compares false with everything, so elements in front of it may still be larger than d: search from the front
                        pos = 0;
#pragma unroll 1
                        while (pos < hole && !(d < ld[pos * block])) pos++;
#pragma unroll 1
                        for (; hole > pos; hole--) {
                            ld[hole * block] = ld[(hole - 1) * block];
                            ls[hole * block] = ls[(hole - 1) * block];
                        }
                    }
                    ld[pos * block] = d;
                    ls[pos * block] = nd.shape;
                    has_nan = has_nan || d != d;
                    if (!full) { len++; full = len == k; }
                    if (full) bound = ld[(k - 1) * block];
                }
            }
            i = nd.exit;
        } else {
            i = enter ? i + 1 : nd.exit;
        }
    }
    // row q: the distances (not squared, :561), then the padding
    uint32_t* os = out_shape + (size_t)q * k;
    T* od = out_dist + (size_t)q * k;
#pragma unroll 1
    for (uint32_t j = 0; j < len; j++) { os[j] = ls[j * block]; od[j] = sqrt(ld[j * block]); }
#pragma unroll 1
    for (uint32_t j = len; j < k; j++) { os[j] = NONE; od[j] = (T)INFINITY; }
}

#endif   // KNN_KERNEL_TEXT
