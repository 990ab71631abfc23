// instances_knn.hip — the k nearest (instance, shape) pairs of every query point over an instance set (bvhgpu_instances_knearest_*;
// include/bvh_mi355x.h).
//
// The definition is knn.hip's loop twice.  Per point p a list L of at most k triples (d, instance, shape), ascending in d, the squared WORLD
// distance in T; full = len(L) == k, bound = L[last].d; every comparison is the strict < of T; insertion is bvhgpu_knearest_*'s (a full list
// drops its last element, the new one goes in front of the first element e with d < e.d, else to the end).
//   top level (the FlatNode array over the world boxes, with p):
//     non-leaf entry: md = aabb.min_distance_squared(p); entry_index iff !full || md < bound, else exit_index
//     leaf entry (instance i): walk instance i, then exit_index
//   instance i (member t = tree_of[i]):
//     q[k] = row4(Y_i[k], p)                                                         the point in the object's frame
//     F    = (row3(Y_i[0], Y_i[0]) + row3(Y_i[1], Y_i[1])) + row3(Y_i[2], Y_i[2])    the squared Frobenius norm of Y_i's 3x3 part
//     member t's array with q: a non-leaf entry is entered iff !full || md < bound * F — ONE multiplication in T, made again whenever
//     `bound` changes and on entry to the instance; a leaf entry (shape s) is decided in WORLD space:
//       w[v][k] = row4(X_i[k], tri_s[v]);   d = triangle_dist2(w, p);   accepted iff !full || d < bound.
// |p - X v| >= |q - v| / ||Y||_F, so a member box with md >= bound * F holds no triangle with d < bound and a world box with md >= bound
// holds none either: acceptance is strict, so what a prune skips could not have been accepted (in exact arithmetic), and a row is the list
// built by offering EVERY pair in the double order (instances in the top level's list order, within each the shapes in the member's) with
// no tree at all.  Equal distances stay in the double order; a candidate equal to `bound` of a full list is refused, so a tie at the k-th
// distance keeps the pairs met first.  A NaN d is accepted only while the list is not full and as `bound` of a full list it is never
// replaced; a NaN bound * F passes no box test.
//   Row j, padded to k: out_instance / out_shape / out_dist[j * k + m] = L[m].instance, L[m].shape, sqrt(L[m].d) for m < len(L); the other
//   slots hold NONE, NONE and +inf.
//
// k_instances_knearest: one query point per lane, ONE loop — instances_within.hip's state machine (a lane is either in the top-level array
// or in a member's) with k_knearest's step and list.  `len`, `full`, `bound`, the object-frame limit and `has_nan` live in registers: a step
// touches the list only when a candidate is accepted.  The lists live in LDS, dynamic size block x k x (sizeof(T) + 8) bytes from the ACTUAL
// k, slot-major: slot m of lane l is element m x block + l of three arrays (distances, then instances, then shapes) — conflict-free, and a
// lane only ever touches its own column, so the kernel has no barrier.  Block size: topk_block's rule for this element size
// (instances_knn_block).  Which arrays are walked: instances_arrays.hpp's table, owned by the set and reused between calls.
//
// MASKED (bvhgpu_instances_knearest_masked_*): point j carries a mask P[j]; the walk passes over an instance whose mask shares
// no bit with it, at its top-level leaf (one 4-byte load: no record, no X_i, no member table), so the list — and with it the bound that
// prunes — only ever sees visible pairs: the row is the incremental list over the double order without the hidden instances' rows.  A point
// whose mask is 0 does not walk: its row is padding.
#include "instances_arrays.hpp"
#include "point_dist.hpp"

namespace bvhgpu {

// the largest of 256 / 128 / 64 lanes whose lists fit 32 KB of LDS, 64 lanes above that
template <typename T> inline unsigned instances_knn_block(uint32_t k) {
    const size_t per_lane = (size_t)k * (sizeof(T) + 8);
    if (256 * per_lane <= 32 * 1024) return 256;
    if (128 * per_lane <= 32 * 1024) return 128;
    return 64;
}
// 64 lanes, the largest k, f64: exactly the 64 KB of dynamic LDS a launch gets without a function attribute (the kernel has no static LDS)
static_assert(BVHGPU_INSTANCES_KNN_MAX_K * 64u * (sizeof(double) + 8u) <= 64u * 1024u, "the lists of 64 lanes must fit a workgroup's LDS");

// what the walk reads of the set
template <typename T> struct InstKnnScene {
    const InstWithinArr<T>* arrs;   // n_trees + 1 rows
    const InstRec<T>* recs;
    const T* xforms;                // n x 12: X_i as committed
    uint32_t top;                   // the top level's row of `arrs`
};

template <typename T, bool MASKED = false>
__global__ __launch_bounds__(256) void k_instances_knearest(InstKnnScene<T> sc, const T* __restrict__ points, uint32_t n, uint32_t k,
                                                            uint32_t* __restrict__ out_instance, uint32_t* __restrict__ out_shape,
                                                            T* __restrict__ out_dist, InstMasks mk) {
    extern __shared__ __align__(16) unsigned char iknn_lds[];
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(iknn_lds) + threadIdx.x;                                        // slot m: ld[m * block]
    uint32_t* __restrict__ li = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(iknn_lds) + (size_t)k * block) + threadIdx.x;
    uint32_t* __restrict__ ls = li + (size_t)k * block;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    if (q >= n) return;
    const T pw[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};   // the world point
    uint32_t len = 0;
    bool full = false;       // len == k
    bool has_nan = false;    // the list holds a NaN: it need not be sorted any more
    T bound = 0;             // L[k - 1].d of a full list
    T lim = 0;               // what a box test compares with: bound at the top level, bound * fn inside an instance
    T fn = 0;                // F of the instance the lane is in
    const InstWithinArr<T> top = sc.arrs[sc.top];
    const TravNode<T>* nodes = top.nodes;
    const T* tris = nullptr;
    T p[3] = {pw[0], pw[1], pw[2]};
    T xr[12] = {};           // X_i of the instance the lane is in
    uint32_t i = 0, end = top.n_trav, unfolded = top.unfolded, inst = NONE, top_next = 0;
    uint32_t pmask = 0xFFFFFFFFu;
    if constexpr (MASKED) {
        if (mk.ray) pmask = mk.ray[q];
        if (pmask == 0u) end = 0;   // (no instance is visible: no walk)
    }
    while (i < end) {
        const NodeRegs<T> nd = load_node(nodes + i);
        const bool leaf = trav_is_leaf(nd.shape);
        bool enter = true;
        if (!(unfolded != 0u && leaf)) {   // (a leaf entry of an unfolded array has no navigator test)
            const T md = aabb_min_dist2<T>(nd.mn, nd.mx, p);
            enter = !full || md < lim;
        }
        i = (leaf || !enter) ? nd.exit : i + 1;
        if (leaf && enter) {
            if (inst != NONE) {   // a triangle of the member: the pair (inst, shape), decided in world space
                const T* tri = tris + 9 * (size_t)nd.shape;
                T w[9];
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const T tv[3] = {tri[3 * v], tri[3 * v + 1], tri[3 * v + 2]};
#pragma unroll
                    for (int c = 0; c < 3; c++) w[3 * v + c] = row4<T>(xr + 4 * c, tv);
                }
                const T d = triangle_dist2<T>(w, pw);
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
                            li[hole * block] = li[(hole - 1) * block];
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
                            li[hole * block] = li[(hole - 1) * block];
                            ls[hole * block] = ls[(hole - 1) * block];
                        }
                    }
                    ld[pos * block] = d;
                    li[pos * block] = inst;
                    ls[pos * block] = nd.shape;
                    has_nan = has_nan || d != d;
                    if (!full) { len++; full = len == k; }
                    if (full) { bound = ld[(k - 1) * block]; lim = bound * fn; }
                }
            } else {              // an instance: into its member with the point and the limit in the object's frame
                bool visible = true;
                if constexpr (MASKED) visible = (mk.inst[nd.shape] & pmask) != 0u;   // (hidden: the lane stays here and goes on at nd.exit)
                if (visible) {
                    top_next = i;
                    inst = nd.shape;
                    const InstRec<T> rec = load_rec<T>(sc.recs + inst);
                    const InstWithinArr<T> a = sc.arrs[rec.tree];
                    T f[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) { p[c] = row4<T>(rec.y + 4 * c, pw); f[c] = row3<T>(rec.y + 4 * c, rec.y + 4 * c); }
                    const T f01 = f[0] + f[1];
                    fn = f01 + f[2];
                    lim = bound * fn;
                    const T* x = sc.xforms + 12 * (size_t)inst;
#pragma unroll
                    for (int c = 0; c < 12; c++) xr[c] = x[c];
                    nodes = a.nodes; tris = a.tris; i = 0; end = a.n_trav; unfolded = a.unfolded;
                }
            }
        }
        if (inst != NONE && i >= end) {   // the member's array has ended: back to the top level, behind the leaf that sent the lane here
#pragma unroll
            for (int c = 0; c < 3; c++) p[c] = pw[c];
            lim = bound;
            nodes = top.nodes; i = top_next; end = top.n_trav; unfolded = top.unfolded; inst = NONE;
        }
    }
    // row q: the distances (not squared), then the padding
    uint32_t* oi = out_instance + (size_t)q * k;
    uint32_t* os = out_shape + (size_t)q * k;
    T* od = out_dist + (size_t)q * k;
#pragma unroll 1
    for (uint32_t m = 0; m < len; m++) { oi[m] = li[m * block]; os[m] = ls[m * block]; od[m] = sqrt(ld[m * block]); }
#pragma unroll 1
    for (uint32_t m = len; m < k; m++) { oi[m] = NONE; os[m] = NONE; od[m] = (T)INFINITY; }
}

// a set without instances: every slot is padding (+inf is no byte pattern, so no memset)
template <typename T>
__global__ __launch_bounds__(256) void k_instances_knn_fill(uint32_t* __restrict__ out_instance, uint32_t* __restrict__ out_shape, T* __restrict__ out_dist,
                                                            uint32_t total) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out_instance[e] = NONE;
    out_shape[e] = NONE;
    out_dist[e] = (T)INFINITY;
}

// the points of a batch over a committed instance set (the caller has checked commit, staleness, the members' kinds and n x k < 2^32)
// masked: bvhgpu_instances_knearest_masked_* — the set's masks against point_mask_dev (NULL: all ones); otherwise point_mask_dev is not looked at
template <typename T>
void instances_knearest_batch(bvhgpu_instances* s, const T* points_dev, size_t n, uint32_t k, uint32_t* out_instance_dev, uint32_t* out_shape_dev,
                              T* out_dist_dev, bool masked, const uint32_t* point_mask_dev) {
    if (!n) return;
    hipStream_t st = s->ctx->stream;
    if (s->n == 0 || s->top == nullptr || s->top->n == 0) {   // no instance (with a finite world box): every row is padding
        const size_t total = n * k;
        hipLaunchKernelGGL((k_instances_knn_fill<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out_instance_dev, out_shape_dev, out_dist_dev,
                           (uint32_t)total);
        BVH_HIP(hipGetLastError());
        return;
    }
    const InstWithinArr<T>* arrs = instances_array_table<T>(s, s->kn_unfold, s->kn_arrs, s->kn_arrs_host);
    const InstKnnScene<T> sc = {arrs, s->recs.as<InstRec<T>>(), s->xforms.as<T>(), (uint32_t)s->trees.size()};
    const unsigned bs = instances_knn_block<T>(k);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 8);
    const dim3 grid((unsigned)((n + bs - 1) / bs));
    if (masked) {
        const InstMasks mk = {s->masks.as<uint32_t>(), point_mask_dev};
        hipLaunchKernelGGL((k_instances_knearest<T, true>), grid, dim3(bs), lds, st, sc, points_dev, (uint32_t)n, k, out_instance_dev, out_shape_dev, out_dist_dev, mk);
    } else {
        hipLaunchKernelGGL((k_instances_knearest<T, false>), grid, dim3(bs), lds, st, sc, points_dev, (uint32_t)n, k, out_instance_dev, out_shape_dev, out_dist_dev,
                           InstMasks{nullptr, nullptr});
    }
    BVH_HIP(hipGetLastError());
}
template void instances_knearest_batch<float>(bvhgpu_instances*, const float*, size_t, uint32_t, uint32_t*, uint32_t*, float*, bool, const uint32_t*);
template void instances_knearest_batch<double>(bvhgpu_instances*, const double*, size_t, uint32_t, uint32_t*, uint32_t*, double*, bool, const uint32_t*);

}  // namespace bvhgpu
