// khits.hip — the k nearest hits of every ray of a batch (bvhgpu_traverse_khits_*; include/bvh_mi355x.h).
//
// Ray i has the list L_i = FlatBvh::traverse(&ray_i, shapes) (flat_bvh.rs:396-431, in its order: the engine's CSR row) and a segment end
// tmax[i] (NULL: +inf).  The leaf stage LEAF gives every member s of L_i a record whose first scalar is its DISTANCE:
//   KH_BOX       {enter, exit}        Ray::intersection_slice_for_aabb on s's own AABB (slab_hit's slice: what BVHGPU_TRAVERSE_T_SLICE returns)
//   KH_TRIANGLE  {distance, u, v}     walk.hpp ray_triangle on t->tris (what BVHGPU_TRAVERSE_TRIANGLES returns)
//   KH_SPHERE    {distance, exit}     walk.hpp ray_sphere on t->spheres (§4f)
// s is a candidate iff distance < tmax[i] — strict, in T: a miss (+inf) is none, and a NaN, zero or negative tmax admits nothing.  Row i is
// the candidates of L_i in a stable ascending sort by distance, cut to the first k: equal distances stay in the order of L_i (which is not
// shape-index order).  The other slots hold NONE and the no-candidate record {+inf, 0} / {+inf, 0, 0}.
// The kernel runs the incremental form, knn.hip's list with the strict < of T: while the list is not full every candidate enters; a full
// list accepts d iff d < L[k-1] and drops L[k-1]; an accepted d goes in front of the first element e with d < e, else to the end.  A later
// candidate never passes an equal earlier one, and an equal candidate never evicts one: that is the stable sort cut to k.
// No NaN branch: a candidate's distance is never NaN — it passed `distance < tmax`, and before that `enter` is max(tmn, 0) of a slab test
// that rejects NaN, and ray_triangle / ray_sphere return either +inf or a value > eps.  So the list is always sorted and the search from
// the back that knn.hip keeps for NaN-free lists is the only one.
// No pruning: the walk visits all of L_i, as CLOSEST does.  Skipping a subtree whose box starts behind the k-th distance would be inexact
// on trees with an inverted shape box (§4e's counterexample).
//
// k_ray_khits: one ray per lane, a plain per-lane loop over the folded array `trav` with exactly k_traverse's step (walk_binary.hip):
// load_node, slab test, i = hit ? i + 1 : exit, a leaf is reported when hit && trav_is_leaf.  Hit decisions are k_traverse's: the box kind
// needs the slice of every leaf and runs the NaN-aware slab_hit throughout (as the box modes do); the other kinds take the slab_hit_finite
// shortcut for a ray with ray_is_finite — per lane, where k_traverse decides per wave; both tests give the same boolean for such a ray.
// No cross-lane operation, no barrier: a lane only ever touches its own column of the list.
// The list is (distance, shape) pairs in dynamic LDS, slot-major as in knn.hip: slot j of lane l is element j x block + l of two arrays
// (distances, then shapes); block x k x (sizeof(T) + 4) bytes from the ACTUAL k; block size by knn_block's rule (256 / 128 / 64 lanes, the
// largest whose lists fit 32 KB; 64 above that).  Write-out: the whole record of every list element is computed again from the ray and the
// shape — the same device function on the same operands, hence the same bits (k_box_resolve and k_sphere_resolve do the same); the box kind
// reads t->aabbs, which is what the leaf entry holds in folded and in unfolded arrays.  Then the padding.
#include "walk.hpp"

namespace bvhgpu {

enum : int { KH_BOX = BVHGPU_LEAF_BOX, KH_TRIANGLE = BVHGPU_LEAF_TRIANGLE, KH_SPHERE = BVHGPU_LEAF_SPHERE };

static_assert(BVHGPU_KHITS_MAX_K * 64u * (sizeof(double) + 4u) <= 64u * 1024u, "the k-hit lists of 64 lanes must fit a workgroup's LDS");

// knn.hip knn_block's rule
template <typename T> static unsigned khits_block(uint32_t k) {
    const size_t per_lane = (size_t)k * (sizeof(T) + 4);
    if (256 * per_lane <= 32 * 1024) return 256;
    if (128 * per_lane <= 32 * 1024) return 128;
    return 64;
}

template <int LEAF> struct KhitsVals { static constexpr uint32_t W = LEAF == KH_TRIANGLE ? 3u : 2u; };

// the record of shape s for the ray: prims is t->aabbs (n x 6), t->tris (n x 9) or t->spheres (n x 4) by LEAF
template <typename T, int LEAF>
__device__ __forceinline__ void khits_record(const T o[3], const T d[3], const T inv[3], const T* __restrict__ prims, uint32_t s, T out[3]) {
    out[2] = 0;
    if (LEAF == KH_TRIANGLE) {
        ray_triangle<T>(o, d, prims + 9 * (size_t)s, out);
    } else if (LEAF == KH_SPHERE) {
        ray_sphere<T>(o, d, prims + 4 * (size_t)s, out);
    } else {
        const T* b = prims + 6 * (size_t)s;
        const T mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
        T t0, t1;
        const bool hit = slab_hit<T>(o, inv, mn, mx, t0, t1);
        out[0] = hit ? t0 : Traits<T>::inf(); out[1] = hit ? t1 : (T)0;
    }
}

template <typename T, int LEAF>
__global__ __launch_bounds__(256) void k_ray_khits(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ prims,
                                                   const typename Traits<T>::Ray* __restrict__ rays, const T* __restrict__ tmaxs, uint32_t n,
                                                   uint32_t k, uint32_t* __restrict__ out_shape, T* __restrict__ out_vals) {
    extern __shared__ __align__(16) unsigned char khits_lds[];
    constexpr uint32_t W = KhitsVals<LEAF>::W;
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(khits_lds) + threadIdx.x;                                        // slot j: ld[j * block]
    uint32_t* __restrict__ ls = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(khits_lds) + (size_t)k * block) + threadIdx.x;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    if (q >= n) return;
    const typename Traits<T>::Ray* rp = rays + q;
    const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, inv[3] = {rp->inv[0], rp->inv[1], rp->inv[2]};
    T d[3] = {0, 0, 0};
    if (LEAF != KH_BOX) { d[0] = rp->d[0]; d[1] = rp->d[1]; d[2] = rp->d[2]; }
    const T tmax = tmaxs ? tmaxs[q] : Traits<T>::inf();
    const bool fast = LEAF != KH_BOX && ray_is_finite<T>(o, inv);   // the NaN-free slab test is exact for this ray (it returns no slice)
    uint32_t len = 0;
    bool full = false;   // len == k
    T bound = 0;         // L[k - 1].distance of a full list
    uint32_t i = 0;
    while (i < n_trav) {
        const NodeRegs<T> nd = load_node(nodes + i);
        T t0 = 0, t1 = 0;
        const bool hit = fast ? slab_hit_finite<T>(o, inv, nd.mn, nd.mx) : slab_hit<T>(o, inv, nd.mn, nd.mx, t0, t1);
        if (hit && trav_is_leaf(nd.shape)) {
            T dist = t0;   // box: the leaf entry is the shape's own box
            if (LEAF != KH_BOX) {
                T rec[3];
                khits_record<T, LEAF>(o, d, inv, prims, nd.shape, rec);
                dist = rec[0];
            }
            if (dist < tmax && (!full || dist < bound)) {
                uint32_t hole = full ? k - 1 : len;   // a full list drops its last element
                // ascending list: the first element e with dist < e is where a scan from the back stops, so search and shift are one loop
#pragma unroll 1
                while (hole > 0) {
                    const T e = ld[(hole - 1) * block];
                    if (!(dist < e)) break;
                    ld[hole * block] = e;
                    ls[hole * block] = ls[(hole - 1) * block];
                    hole--;
                }
                ld[hole * block] = dist;
                ls[hole * block] = nd.shape;
                if (!full) { len++; full = len == k; }
                if (full) bound = ld[(k - 1) * block];
            }
        }
        i = hit ? i + 1 : nd.exit;   // a leaf's exit IS i+1
    }
    // row q: the records, then the padding
    uint32_t* os = out_shape + (size_t)q * k;
    T* ov = out_vals + (size_t)q * k * W;
#pragma unroll 1
    for (uint32_t j = 0; j < len; j++) {
        const uint32_t s = ls[j * block];
        T rec[3];
        khits_record<T, LEAF>(o, d, inv, prims, s, rec);
        os[j] = s;
#pragma unroll
        for (uint32_t c = 0; c < W; c++) ov[j * W + c] = rec[c];
    }
#pragma unroll 1
    for (uint32_t j = len; j < k; j++) {
        os[j] = NONE;
        ov[j * W] = Traits<T>::inf();
#pragma unroll
        for (uint32_t c = 1; c < W; c++) ov[j * W + c] = 0;
    }
}

// an empty hierarchy: every slot is padding (+inf is no byte pattern, so no memset); w = scalars per record
template <typename T>
__global__ __launch_bounds__(256) void k_khits_fill(uint32_t* __restrict__ out_shape, T* __restrict__ out_vals, uint32_t total, uint32_t w) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out_shape[e] = NONE;
    T* v = out_vals + (size_t)e * w;
    v[0] = Traits<T>::inf();
    for (uint32_t c = 1; c < w; c++) v[c] = 0;
}

template <typename T>
void khits_batch(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, int leaf, uint32_t k,
                 uint32_t* out_shape_dev, T* out_vals_dev) {
    if (!n) return;
    hipStream_t st = t->ctx->stream;
    if (t->n == 0) {
        const size_t total = n * k;   // (the caller has checked n x k < 2^32)
        hipLaunchKernelGGL((k_khits_fill<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out_shape_dev, out_vals_dev, (uint32_t)total,
                           leaf == KH_TRIANGLE ? 3u : 2u);
        BVH_HIP(hipGetLastError());
        return;
    }
    const unsigned bs = khits_block<T>(k);
    const dim3 grid((unsigned)((n + bs - 1) / bs)), block(bs);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 4);
    ensure_flat_arrays(t);
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    const uint32_t n_trav = (uint32_t)t->n_trav;
#define LAUNCH_KHITS(LEAF, PRIMS) hipLaunchKernelGGL((k_ray_khits<T, LEAF>), grid, block, lds, st, nodes, n_trav, (const T*)t->PRIMS.as<T>(), rays_dev, \
                                                     tmax_dev, (uint32_t)n, k, out_shape_dev, out_vals_dev)
    if (leaf == KH_TRIANGLE) LAUNCH_KHITS(KH_TRIANGLE, tris);
    else if (leaf == KH_SPHERE) LAUNCH_KHITS(KH_SPHERE, spheres);
    else LAUNCH_KHITS(KH_BOX, aabbs);
#undef LAUNCH_KHITS
    BVH_HIP(hipGetLastError());
}
template void khits_batch<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, const float*, size_t, int, uint32_t, uint32_t*, float*);
template void khits_batch<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, const double*, size_t, int, uint32_t, uint32_t*, double*);

}  // namespace bvhgpu
