// nearest.hip — nearest_to point queries over the folded array (k_nearest), one query point per lane.
#include "point_dist.hpp"
#include "walk.hpp"

namespace bvhgpu {

// ------------------------------------------------------------------------------------------------
// <FlatBvh as BoundingHierarchy>::nearest_to (flat_bvh.rs:513-562) for a batch of query points.
// The two shape distances (aabb_min_dist2, triangle_dist2) live in point_dist.hpp, shared with k_knearest (knn.hip).
// ------------------------------------------------------------------------------------------------
// one query point per lane, the same loop as flat_bvh.rs:533-558 over the folded array: a folded leaf entry
// stands for the navigator (min_distance_squared test of its box) followed by the leaf (exact shape distance)
template <typename T, bool TRIANGLE, bool UNFOLDED>
__global__ __launch_bounds__(256) void k_nearest(const TravNode<T>* __restrict__ nodes, uint32_t n_trav,
                                                 const T* __restrict__ shape_aabbs, const T* __restrict__ tris,
                                                 const T* __restrict__ points, uint32_t n, uint32_t* __restrict__ out_shape,
                                                 T* __restrict__ out_dist) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const T p[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};
    bool has = false;
    T best = 0;
    uint32_t bs = NONE;
    uint32_t i = 0;
    while (i < n_trav) {
        const NodeRegs<T> nd = load_node(nodes + i);
        const bool leaf = trav_is_leaf(nd.shape);
        bool enter = true;
        if (!(UNFOLDED && leaf)) {
            const T md = aabb_min_dist2<T>(nd.mn, nd.mx, p);
            enter = !has || md < best;                           // :550
        }
        if (leaf) {
            if (enter) {
                T d;
                if (TRIANGLE) d = triangle_dist2<T>(tris + 9 * (size_t)nd.shape, p);
                else {
                    const T* sb = shape_aabbs + 6 * (size_t)nd.shape;
                    const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
                    d = aabb_min_dist2<T>(mn, mx, p);
                }
                if (!has || d < best) { has = true; best = d; bs = nd.shape; }   // :540-542
            }
            i = nd.exit;
        } else {
            i = enter ? i + 1 : nd.exit;
        }
    }
    out_shape[q] = bs;
    out_dist[q] = has ? sqrt(best) : (T)0;                       // :561
}

template <typename T>
void nearest_batch(bvhgpu_tree* t, const T* points_dev, size_t n, int kind, uint32_t* out_shape_dev, T* out_dist_dev) {
    if (!n) return;
    hipStream_t st = t->ctx->stream;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    ensure_flat_arrays(t);
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    const uint32_t n_trav = (uint32_t)t->n_trav;
    const bool unfolded = t->unfolded || t->n == 1;   // a single-shape tree has one (leaf) entry and no navigator
#define LAUNCH_NEAREST(TRI, UNF) hipLaunchKernelGGL((k_nearest<T, TRI, UNF>), grid, block, 0, st, nodes, n_trav, t->aabbs.as<T>(), \
                                                    t->tris.as<T>(), points_dev, (uint32_t)n, out_shape_dev, out_dist_dev)
    if (kind == 1) { if (unfolded) LAUNCH_NEAREST(true, true); else LAUNCH_NEAREST(true, false); }
    else { if (unfolded) LAUNCH_NEAREST(false, true); else LAUNCH_NEAREST(false, false); }
#undef LAUNCH_NEAREST
    BVH_HIP(hipGetLastError());
}
template void nearest_batch<float>(bvhgpu_tree*, const float*, size_t, int, uint32_t*, float*);
template void nearest_batch<double>(bvhgpu_tree*, const double*, size_t, int, uint32_t*, double*);

}  // namespace bvhgpu
