// knn_tree.hip — the k nearest shapes of every query point, found nearest child first (bvhgpu_knearest_tree_*): the "tree form" of the
// point queries beside knn.hip's "flat form".
//
// Definition: BvhNode::nearest_to_recursive (bvh_node.rs:327-374, reached from Bvh::nearest_to, bvh_impl.rs:221-238) over the BvhNode array,
// with `best_candidate` replaced by knn.hip's list L of at most k pairs (dist2, shape) and an optional per-point limit m = max_dist[i]:
//   full = len(L) == k,  bound = L[last].dist2,  r2 = m * m (one multiplication in T)
//   admit(x) = (max_dist == NULL || (m >= 0 && x <= r2)) && (!full || x < bound)
//   visit(node):                                             root = node 0
//     Leaf{shape}:  d = shape.distance_squared(p); if admit(d): drop L[last] of a full list, insert (d, shape) in front of the first e
//                   with d < e.dist2, else at the end
//     Node{l, l_aabb, r, r_aabb}:  c = [(l, l_aabb.min_distance_squared(p)), (r, r_aabb.min_distance_squared(p))]
//                   if c[0].1 > c[1].1: swap                 strict >: ties and NaN keep the left child first
//                   for (idx, cd) in c: if admit(cd): visit(idx)      the second test sees the list as the first subtree left it
// Every comparison is T's <, > or <= as written; what a NaN does follows from that (knn.hip: a row that holds a NaN need not be sorted).
// Equal distances stay in the order THIS walk meets them, which is not leaf pre-order: the flat and the tree form may order ties
// differently and pick differently among ties at the k-th distance.  Row i as for bvhgpu_knearest_*: shape[i][j] = L[j].shape,
// dist[i][j] = sqrt(L[j].dist2), the other slots NONE and +inf; an empty hierarchy, a negative or a NaN max_dist[i] give a row of padding.
// With k = 1 and no max_dist a row is bit for bit what Bvh::nearest_to returns (the empty hierarchy's distance excepted: +inf here).
//
// k_knearest_tree: one query point per lane over t->nodes, the BvhNode image (64 B in f32, 112 B in f64: both child boxes, l, r, parent
// and shape in one record).  No stack, no depth limit, no per-lane memory outside registers and the list: the walk returns through the
// records' parent words.  Arriving at an inner node from above it orders the two children and enters the first one that admit() passes;
// coming back from child c it computes the same two distances again — same inputs, same bits, same order — and tests the second child if
// c was the first, otherwise goes further up; it ends when it comes back to node 0 with nothing left.  A step is one record load and two
// aabb_min_dist2 (point_dist.hpp, unchanged: the oracle's bits).  len / bound / full / has_nan live in registers, r2 and m >= 0 are
// evaluated once per lane.  The list is knn.hip's: dynamic LDS, block x k x (sizeof(T) + 4) bytes, slot-major, topk_block's block sizes,
// no barrier.  The insertion below is a copy of k_knearest's (k_ray_khits holds a third, without the NaN branch).  Sharing it has been tried
// twice; the second time as a __forceinline__ template taking ld, ls, block, k and references to len / full / has_nan / bound: it changed
// the instruction text of 17 of the 22 kernels that hold the insertion and the register counts of several, so it stays restated.
// Shape distance: kind 0 / 1 (bvhgpu_knearest_tree_*), or the shape's sphere (bvhgpu_knearest_tree_sphere_*, point_dist.hpp's sphere_dist2;
// DESIGN.md §4u): only d at a leaf changes, the child boxes prune as before.
#ifndef KNN_TREE_KERNEL_TEXT
#include "point_dist.hpp"
#include "tree_node.hpp"

namespace bvhgpu {

static_assert(topk_fits(BVHGPU_KNN_MAX_K), "the k-nearest lists of 64 lanes must fit a workgroup's LDS");

// The kernel text stands at the end of this file, behind KNN_TREE_KERNEL_TEXT, and is compiled twice by the two includes of this file
// below (knn.hip's arrangement): as k_knearest_tree<T, TRIANGLE>, name, template head and instructions as they were, and
// as k_knearest_tree_sphere<T>.  POINT_KIND_VALUE: 0 box, 1 triangle, 2 sphere; `prims` is the array of that kind.
#define KNN_TREE_KERNEL_TEXT
#define POINT_K(name) name
#define POINT_KIND_TPARAM , bool TRIANGLE
#define POINT_KIND_VALUE (TRIANGLE ? 1 : 0)
#include "knn_tree.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#define POINT_K(name) name##_sphere
#define POINT_KIND_TPARAM
#define POINT_KIND_VALUE 2
#include "knn_tree.hip"
#undef POINT_K
#undef POINT_KIND_TPARAM
#undef POINT_KIND_VALUE
#undef KNN_TREE_KERNEL_TEXT

template <typename T>
void knearest_tree_batch(bvhgpu_tree* t, const T* points_dev, size_t n, int kind, uint32_t k, const T* max_dist_dev, uint32_t* out_shape_dev,
                         T* out_dist_dev) {
    if (!n) return;
    using Node = typename Traits<T>::Node;
    hipStream_t st = t->ctx->stream;
    const unsigned bs = topk_block<T>(k);
    const dim3 grid((unsigned)((n + bs - 1) / bs)), block(bs);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 4);
    const uint32_t n_nodes = t->n ? (uint32_t)t->n_nodes : 0u;
    if (kind == POINT_KIND_SPHERE)
        hipLaunchKernelGGL((k_knearest_tree_sphere<T>), grid, block, lds, st, t->nodes.as<Node>(), n_nodes, t->aabbs.as<T>(), t->spheres.as<T>(),
                           points_dev, (uint32_t)n, k, max_dist_dev, out_shape_dev, out_dist_dev);
    else if (kind == 1)
        hipLaunchKernelGGL((k_knearest_tree<T, true>), grid, block, lds, st, t->nodes.as<Node>(), n_nodes, t->aabbs.as<T>(), t->tris.as<T>(),
                           points_dev, (uint32_t)n, k, max_dist_dev, out_shape_dev, out_dist_dev);
    else
        hipLaunchKernelGGL((k_knearest_tree<T, false>), grid, block, lds, st, t->nodes.as<Node>(), n_nodes, t->aabbs.as<T>(), t->tris.as<T>(),
                           points_dev, (uint32_t)n, k, max_dist_dev, out_shape_dev, out_dist_dev);
    BVH_HIP(hipGetLastError());
}
template void knearest_tree_batch<float>(bvhgpu_tree*, const float*, size_t, int, uint32_t, const float*, uint32_t*, float*);
template void knearest_tree_batch<double>(bvhgpu_tree*, const double*, size_t, int, uint32_t, const double*, uint32_t*, double*);

}  // namespace bvhgpu

#else   // KNN_TREE_KERNEL_TEXT: the kernel text, inside namespace bvhgpu (see the includes of this file above)

template <typename T POINT_KIND_TPARAM>
__global__ __launch_bounds__(256) void POINT_K(k_knearest_tree)(const typename Traits<T>::Node* __restrict__ nodes, uint32_t n_nodes,
                                                       const T* __restrict__ shape_aabbs, const T* __restrict__ prims,
                                                       const T* __restrict__ points, uint32_t n, uint32_t k,
                                                       const T* __restrict__ max_dist, uint32_t* __restrict__ out_shape,
                                                       T* __restrict__ out_dist) {
    constexpr int KIND = POINT_KIND_VALUE;
    extern __shared__ __align__(16) unsigned char knn_tree_lds[];
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(knn_tree_lds) + threadIdx.x;                                   // slot j: ld[j * block]
    uint32_t* __restrict__ ls = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(knn_tree_lds) + (size_t)k * block) + threadIdx.x;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    if (q >= n) return;
    const T p[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};
    uint32_t len = 0;
    bool full = false;       // len == k
    bool has_nan = false;    // the list holds a NaN: it need not be sorted any more
    T bound = 0;             // L[k - 1].dist2 of a full list
    const bool limited = max_dist != nullptr;
    T r2 = 0;
    bool walk = n_nodes != 0;                    // an empty hierarchy: the row is padding
    if (limited) {
        const T m = max_dist[q];
        r2 = m * m;
        walk = walk && m >= (T)0;                // a negative or NaN limit admits nothing
    }
#define ADMIT(x) ((!limited || (x) <= r2) && (!full || (x) < bound))
    uint32_t cur = 0;        // the record the lane is at
    uint32_t from = NONE;    // the child it came back from; NONE: it arrived from above
    while (walk) {
        const TreeRegs<T> nd = load_tree_node(nodes + cur);
        uint32_t next = NONE;
        if (nd.shape != NONE) {
            T d;
            if (KIND == 2) d = sphere_dist2<T>(prims + 4 * (size_t)nd.shape, p);
            else if (KIND == 1) d = triangle_dist2<T>(prims + 9 * (size_t)nd.shape, p);
            else {
                const T* sb = shape_aabbs + 6 * (size_t)nd.shape;
                const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
                d = aabb_min_dist2<T>(mn, mx, p);
            }
            if (ADMIT(d)) {
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
        } else {
            const T dl = aabb_min_dist2<T>(nd.lmn, nd.lmx, p), dr = aabb_min_dist2<T>(nd.rmn, nd.rmx, p);
            const bool swap = dl > dr;
            const uint32_t first = swap ? nd.r : nd.l, second = swap ? nd.l : nd.r;
            const T d1 = swap ? dr : dl, d2 = swap ? dl : dr;
            if (from == NONE && ADMIT(d1)) next = first;                // from above: the nearer child, if it passes
            else if (from != second && ADMIT(d2)) next = second;        // ... else, or back from the nearer one: the other child
        }
        if (next != NONE) { cur = next; from = NONE; }
        else {
            if (cur == 0) break;                                        // back at the root with nothing left
            from = cur;
            cur = nd.parent;
        }
        if (cur >= n_nodes) break;                                      // (never in a tree the builder wrote)
    }
#undef ADMIT
    // row q: the distances (not squared), then the padding
    uint32_t* os = out_shape + (size_t)q * k;
    T* od = out_dist + (size_t)q * k;
#pragma unroll 1
    for (uint32_t j = 0; j < len; j++) { os[j] = ls[j * block]; od[j] = sqrt(ld[j * block]); }
#pragma unroll 1
    for (uint32_t j = len; j < k; j++) { os[j] = NONE; od[j] = (T)INFINITY; }
}

#endif   // KNN_TREE_KERNEL_TEXT
