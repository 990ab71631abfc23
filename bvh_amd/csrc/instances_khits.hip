// instances_khits.hip — the k nearest hits of every ray over an instance set, in fixed-width padded rows (bvhgpu_instances_khits_*;
// include/bvh_mi355x.h).
//
// The definition is the candidate table of bvhgpu_instances_trace_* (instances.hip): ray j meets the pairs (instance, shape) in the double
// order — the instances in the order of the top level's list, within each the shapes in the order of the member's list — and (i, s) is a
// candidate iff its distance < tmax[j], strict, in T.  Row j is the candidates in a stable ascending sort by distance, cut to the first k:
// the head of bvhgpu_instances_allhits_*'s sorted row.  The kernel runs the incremental form, khits.hip's list with the strict < of T: while
// the list is not full every candidate enters; a full list accepts d iff d < L[k-1] and drops L[k-1]; an accepted d goes in front of the
// first element e with d < e, else to the end.  A candidate's distance is never NaN (it passed a strict <), so the list is always sorted and
// there is no NaN branch.  No pruning: the walk visits the whole double order (§4e's inverted-box reason, §4j).
//
// k_instances_khits: one ray per lane, ONE loop — instances_walk's step and state machine (instances_allhits.hip; restated here, the
// translation units are compiled separately and that file's device code stays what it was), with the wave-uniform choice between
// slab_hit_finite and slab_hit.  The list is k_instances_knearest's: three slot-major arrays in dynamic LDS (distance in T, instance, shape),
// slot m of lane l is element m x block + l, block x k x (sizeof(T) + 8) bytes from the ACTUAL k — conflict-free, a lane only ever touches
// its own column, only the walk's __any votes cross lanes: no barrier.  `len`, `full` and `bound` live in registers; the list is touched
// only when a candidate is accepted.  Write-out: the whole record of every list element is computed again from the world ray and (instance,
// shape) by inst_record's sequence — the device functions and the operands of bvhgpu_instances_allhits_*, hence its bits.
//
// MASKED (bvhgpu_instances_khits_masked_*): inst_mask is the set's n u32, ray_mask NULL (all ones) or one u32 per ray; an
// instance whose mask shares no bit with the ray's is passed over at its top-level leaf — no record, no re-expressed ray, no member node —
// and the lane goes on at i + 1.  The write-out sees only pairs that are in the list: no mask.  Without MASKED neither pointer is read.
#ifndef INSTANCES_KHITS_KERNEL_TEXT
#include "instances.hpp"
#include "walk.hpp"

namespace bvhgpu {

// instances_knn_block's rule for the same element size: the largest of 256 / 128 / 64 lanes whose lists fit 32 KB of LDS, 64 lanes above that
template <typename T> inline unsigned instances_khits_block(uint32_t k) {
    const size_t per_lane = (size_t)k * (sizeof(T) + 8);
    if (256 * per_lane <= 32 * 1024) return 256;
    if (128 * per_lane <= 32 * 1024) return 128;
    return 64;
}
// 64 lanes, the largest k, f64: exactly the 64 KB of dynamic LDS a launch gets without a function attribute (the kernel has no static LDS)
static_assert(BVHGPU_INSTANCES_KHITS_MAX_K * 64u * (sizeof(double) + 8u) <= 64u * 1024u, "the lists of 64 lanes must fit a workgroup's LDS");

// what the walk reads of the set (instances_allhits.hip's InstScene)
template <typename T> struct InstKhitsScene {
    const TravNode<T>* top;
    uint32_t n_top;
    const InstRec<T>* recs;
    const InstTree<T>* tbl;
};

// The kernel text stands at the end of this file, behind INSTANCES_KHITS_KERNEL_TEXT, and is compiled twice by the two includes of this file below:
// once under the kernels' own names with the TRIANGLE leaf stage — the same text under the same names and template heads as before a set had
// a leaf kind, hence the same instructions — and once as the *_leaf kernels with a LEAF template argument for BOX and SPHERE sets
// (DESIGN.md §4t).  INST_K(name): the kernel's name; INST_LEAF_TPARAM: the end of its template head; INST_LEAF_VALUE: its leaf kind.
#define INSTANCES_KHITS_KERNEL_TEXT
#define INST_K(name) name
#define INST_LEAF_TPARAM
#define INST_LEAF_VALUE LEAF_TRIANGLE
#include "instances_khits.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#define INST_K(name) name##_leaf
#define INST_LEAF_TPARAM , int LEAF_ARG
#define INST_LEAF_VALUE LEAF_ARG
#include "instances_khits.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#undef INSTANCES_KHITS_KERNEL_TEXT

// a set without instances: every slot is padding (+inf is no byte pattern, so no memset)
template <typename T>
__global__ __launch_bounds__(256) void k_instances_khits_fill(uint32_t* __restrict__ out_instance, uint32_t* __restrict__ out_shape, T* __restrict__ out_vals,
                                                              uint32_t total) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out_instance[e] = NONE;
    out_shape[e] = NONE;
    T* v = out_vals + (size_t)e * 3;
    v[0] = Traits<T>::inf(); v[1] = 0; v[2] = 0;
}
// ... of a BOX or SPHERE set: records 2 scalars wide
template <typename T>
__global__ __launch_bounds__(256) void k_instances_khits_fill2(uint32_t* __restrict__ out_instance, uint32_t* __restrict__ out_shape, T* __restrict__ out_vals,
                                                               uint32_t total) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    out_instance[e] = NONE;
    out_shape[e] = NONE;
    T* v = out_vals + (size_t)e * 2;
    v[0] = Traits<T>::inf(); v[1] = 0;
}

// the rays of a batch over a committed instance set (the caller has checked commit, staleness and n x k < 2^32)
// masked: bvhgpu_instances_khits_masked_* — the set's masks against ray_mask_dev (NULL: all ones); otherwise ray_mask_dev is not looked at
template <typename T>
void instances_khits_batch(bvhgpu_instances* s, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, uint32_t k,
                           uint32_t* out_instance_dev, uint32_t* out_shape_dev, T* out_vals_dev, bool masked, const uint32_t* ray_mask_dev) {
    if (!n) return;
    hipStream_t st = s->ctx->stream;
    if (s->n == 0 || s->top == nullptr || s->top->n_trav == 0) {   // no instance, or an empty top level: every row is padding
        const size_t total = n * k;
        if (s->leaf == BVHGPU_LEAF_TRIANGLE)
            hipLaunchKernelGGL((k_instances_khits_fill<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out_instance_dev, out_shape_dev,
                               out_vals_dev, (uint32_t)total);
        else
            hipLaunchKernelGGL((k_instances_khits_fill2<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out_instance_dev, out_shape_dev,
                               out_vals_dev, (uint32_t)total);
        BVH_HIP(hipGetLastError());
        return;
    }
    const InstKhitsScene<T> sc = {s->top->trav.as<TravNode<T>>(), (uint32_t)s->top->n_trav, s->recs.as<InstRec<T>>(), s->table.as<InstTree<T>>()};
    const unsigned bs = instances_khits_block<T>(k);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 8);
    const dim3 grid((unsigned)((n + bs - 1) / bs)), block(bs);
#define INST_KHITS_K(K, M)                                                                                                             \
    hipLaunchKernelGGL(K, grid, block, lds, st, sc, rays_dev, tmax_dev, (uint32_t)n, k, out_instance_dev, out_shape_dev, out_vals_dev, \
                       M ? s->masks.as<uint32_t>() : nullptr, M ? ray_mask_dev : nullptr)
#define INST_KHITS(M)                                                                                              \
    do {                                                                                                           \
        if (s->leaf == BVHGPU_LEAF_TRIANGLE) INST_KHITS_K((k_instances_khits<T, M>), M);                           \
        else if (s->leaf == BVHGPU_LEAF_SPHERE) INST_KHITS_K((k_instances_khits_leaf<T, M, LEAF_SPHERE>), M);      \
        else INST_KHITS_K((k_instances_khits_leaf<T, M, LEAF_BOX>), M);                                            \
    } while (0)
    if (masked) INST_KHITS(true); else INST_KHITS(false);
#undef INST_KHITS
#undef INST_KHITS_K
    BVH_HIP(hipGetLastError());
}
template void instances_khits_batch<float>(bvhgpu_instances*, const bvhgpu_ray_f32*, const float*, size_t, uint32_t, uint32_t*, uint32_t*, float*, bool,
                                           const uint32_t*);
template void instances_khits_batch<double>(bvhgpu_instances*, const bvhgpu_ray_f64*, const double*, size_t, uint32_t, uint32_t*, uint32_t*, double*, bool,
                                            const uint32_t*);

}  // namespace bvhgpu

#else   // INSTANCES_KHITS_KERNEL_TEXT: the kernel text, inside namespace bvhgpu (see the includes of this file above)

template <typename T, bool MASKED INST_LEAF_TPARAM>
__global__ __launch_bounds__(256) void INST_K(k_instances_khits)(InstKhitsScene<T> sc, const typename Traits<T>::Ray* __restrict__ rays,
                                                                 const T* __restrict__ tmaxs, uint32_t n, uint32_t k, uint32_t* __restrict__ out_instance,
                                                                 uint32_t* __restrict__ out_shape, T* __restrict__ out_vals,
                                                                 const uint32_t* __restrict__ inst_mask, const uint32_t* __restrict__ ray_mask) {
    constexpr int LEAF = INST_LEAF_VALUE;
    constexpr uint32_t W = LeafVals<LEAF>::W;
    extern __shared__ __align__(16) unsigned char ikh_lds[];
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(ikh_lds) + threadIdx.x;                                        // slot m: ld[m * block]
    uint32_t* __restrict__ li = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(ikh_lds) + (size_t)k * block) + threadIdx.x;
    uint32_t* __restrict__ ls = li + (size_t)k * block;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    const bool active = q < n;   // (a lane beyond the batch walks nothing and writes nothing, but takes part in the wave's votes)
    const typename Traits<T>::Ray* rp = rays + (active ? q : 0u);
    const T tm = active && tmaxs ? tmaxs[q] : Traits<T>::inf();
    uint32_t rmask = 0xFFFFFFFFu;
    if constexpr (MASKED) { if (active && ray_mask) rmask = ray_mask[q]; }
    T o[3] = {0, 0, 0}, d[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
    bool fin = true, wfin = true;   // the current ray / the world ray passes ray_is_finite (the NaN-free slab test is exact for it)
    if (active) {
#pragma unroll
        for (int c = 0; c < 3; c++) { o[c] = rp->o[c]; d[c] = rp->d[c]; inv[c] = rp->inv[c]; }
        wfin = ray_is_finite<T>(o, inv);
        fin = wfin;
    }
    uint32_t len = 0;
    bool full = false;   // len == k
    T bound = 0;         // L[k - 1].distance of a full list
    const TravNode<T>* nodes = sc.top;
    const T* prims = nullptr;
    uint32_t i = 0, end = active ? sc.n_top : 0u, inst = NONE, top_next = 0;
    while (true) {
        const bool run = i < end;
        if (!__any(run)) break;
        const bool fast = !__any(run && !fin);   // wave-uniform
        if (run) {
            const NodeRegs<T> nd = load_node(nodes + i);
            T t0, t1;
            const bool hit = fast ? slab_hit_finite<T>(o, inv, nd.mn, nd.mx) : slab_hit<T>(o, inv, nd.mn, nd.mx, t0, t1);
            const bool leaf = trav_is_leaf(nd.shape);
            i = hit ? i + 1 : nd.exit;   // a leaf's exit IS i+1
            if (hit && leaf) {
                if (inst != NONE) {   // a shape of the member: the pair (inst, shape), its record by the set's leaf kind
                    T v[3];
                    if constexpr (LEAF == LEAF_TRIANGLE) ray_triangle<T>(o, d, prims + 9 * (size_t)nd.shape, v);   // (leaf_record's triangle stage, spelt out)
                    else leaf_record<T, LEAF>(o, d, inv, prims, nd.shape, v);
                    const T dist = v[0];
                    if (dist < tm && (!full || dist < bound)) {
                        uint32_t hole = full ? k - 1 : len;   // a full list drops its last element
                        // ascending list: the first element e with dist < e is where a scan from the back stops, so search and shift are one loop
#pragma unroll 1
                        while (hole > 0) {
                            const T e = ld[(hole - 1) * block];
                            if (!(dist < e)) break;
                            ld[hole * block] = e;
                            li[hole * block] = li[(hole - 1) * block];
                            ls[hole * block] = ls[(hole - 1) * block];
                            hole--;
                        }
                        ld[hole * block] = dist;
                        li[hole * block] = inst;
                        ls[hole * block] = nd.shape;
                        if (!full) { len++; full = len == k; }
                        if (full) bound = ld[(k - 1) * block];
                    }
                } else {              // an instance's world box: into its tree with the ray in the object's frame
                    bool visible = true;
                    if constexpr (MASKED) visible = (inst_mask[nd.shape] & rmask) != 0u;   // (hidden: the lane stays here and goes on at i + 1)
                    if (visible) {
                        top_next = i;
                        inst = nd.shape;
                        const InstRec<T> rec = load_rec<T>(sc.recs + inst);
                        const InstTree<T> t = sc.tbl[rec.tree];
                        T oo[3], dd[3];
#pragma unroll
                        for (int c = 0; c < 3; c++) { oo[c] = row4<T>(rec.y + 4 * c, o); dd[c] = row3<T>(rec.y + 4 * c, d); }
#pragma unroll
                        for (int c = 0; c < 3; c++) { o[c] = oo[c]; d[c] = dd[c]; inv[c] = (T)1 / dd[c]; }
                        fin = ray_is_finite<T>(o, inv);
                        nodes = t.trav; prims = t.prims; i = 0; end = t.n_trav;
                    }
                }
            }
            if (inst != NONE && i >= end) {   // the member's array has ended: back to the top level, behind the leaf that sent the lane here
#pragma unroll
                for (int c = 0; c < 3; c++) { o[c] = rp->o[c]; d[c] = rp->d[c]; inv[c] = rp->inv[c]; }
                fin = wfin;
                nodes = sc.top; i = top_next; end = sc.n_top; inst = NONE;
            }
        }
    }
    if (!active) return;
    // row q: the whole record of every element, computed again from the world ray and (instance, shape) — inst_record's sequence
    // (instances_allhits.hip) — then the padding
#pragma unroll
    for (int c = 0; c < 3; c++) { o[c] = rp->o[c]; d[c] = rp->d[c]; }
    uint32_t* oi = out_instance + (size_t)q * k;
    uint32_t* os = out_shape + (size_t)q * k;
    T* ov = out_vals + (size_t)q * k * (W == 3 ? 3 : 2);
#pragma unroll 1
    for (uint32_t m = 0; m < len; m++) {
        const uint32_t in = li[m * block], s = ls[m * block];
        const InstRec<T> rec = load_rec<T>(sc.recs + in);
        const InstTree<T> t = sc.tbl[rec.tree];
        T oo[3], dd[3], v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { oo[c] = row4<T>(rec.y + 4 * c, o); dd[c] = row3<T>(rec.y + 4 * c, d); }
        if constexpr (LEAF == LEAF_TRIANGLE) {
            ray_triangle<T>(oo, dd, t.prims + 9 * (size_t)s, v);
        } else {
            if (LEAF == LEAF_BOX) {   // (only the box stage reads the inverse: the walk's, from the object-space direction)
#pragma unroll
                for (int c = 0; c < 3; c++) inv[c] = (T)1 / dd[c];
            }
            leaf_record<T, LEAF>(oo, dd, inv, t.prims, s, v);
        }
        oi[m] = in;
        os[m] = s;
        if constexpr (W == 3) { ov[3 * m] = v[0]; ov[3 * m + 1] = v[1]; ov[3 * m + 2] = v[2]; }
        else { ov[2 * m] = v[0]; ov[2 * m + 1] = v[1]; }
    }
#pragma unroll 1
    for (uint32_t m = len; m < k; m++) {
        oi[m] = NONE;
        os[m] = NONE;
        if constexpr (W == 3) { ov[3 * m] = Traits<T>::inf(); ov[3 * m + 1] = 0; ov[3 * m + 2] = 0; }
        else { ov[2 * m] = Traits<T>::inf(); ov[2 * m + 1] = 0; }
    }
}

#endif   // INSTANCES_KHITS_KERNEL_TEXT
