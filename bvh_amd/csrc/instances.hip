// instances.hip — instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_*): a top-level tree over the world boxes of n instances, each
// of which is (member tree, 3x4 transform), and the two-level walk over it.  Definition and order of operations: the header.
//   k_instances_prep<T, 0>   B_t: the join of member tree t's shape AABBs (one workgroup per tree)
//   k_instances_prep<T, 1>   Y_i (the inverse transform) and W_i (the world box) of instance i (one lane per instance)
//   k_instances_trace        one ray per lane over the top-level array; a top-level leaf sends the lane, with the ray re-expressed in the
//                            object's frame, into that member's array — the same loop, another array — and the lane comes back to the
//                            entry behind that leaf when the member's array ends.  MASKED (bvhgpu_instances_trace_masked_*, DESIGN.md
//                            §4r): an instance whose mask shares no bit with the ray's is passed over at its top-level leaf
// Node fetch, slab test and triangle test are walk.hpp's and common.hpp's, unchanged: that is what makes the bits those of the
// single-tree walks.  Nothing is pruned.
//   k_instances_trace_leaf   the same text for a set of BOX or SPHERE leaves (bvhgpu_instances_create_leaf_*): the leaf
//                            stage is walk.hpp's leaf_record on the object-space ray, the record 2 scalars wide
#ifndef INSTANCES_TRACE_KERNEL_TEXT
#include "instances.hpp"
#include "walk.hpp"

namespace bvhgpu {

template <typename T> __device__ __forceinline__ T cof(T a, T b, T c, T d) {   // a*b - c*d: two rounded products, one subtraction
    const T p = a * b, q = c * d;
    return p - q;
}

// ------------------------------------------------------------------------------------------------
// PHASE 0: grid = member trees.  PHASE 1: grid = ceil(n / 256), behind phase 0 on the stream.
// ------------------------------------------------------------------------------------------------
template <typename T, int PHASE>
__global__ __launch_bounds__(256) void k_instances_prep(const InstTree<T>* __restrict__ tbl, T* __restrict__ bounds, const uint32_t* __restrict__ tree_of,
                                                        const T* __restrict__ xforms, uint32_t n, InstRec<T>* __restrict__ recs, T* __restrict__ wboxes) {
    if (PHASE == 0) {
        __shared__ T part[4][6];
        const InstTree<T> t = tbl[blockIdx.x];
        T mn[3], mx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { mn[k] = Traits<T>::inf(); mx[k] = -Traits<T>::inf(); }
        for (uint32_t s = threadIdx.x; s < t.n; s += 256u) {
            const T* b = t.aabbs + 6 * (size_t)s;
#pragma unroll
            for (int k = 0; k < 3; k++) { mn[k] = join_min(mn[k], b[k]); mx[k] = join_max(mx[k], b[3 + k]); }
        }
        // min / max are exact and order -0 < +0 (common.hpp join_min): any association gives the same bits on NaN-free boxes
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; k++) { mn[k] = join_min(mn[k], __shfl_xor(mn[k], d)); mx[k] = join_max(mx[k], __shfl_xor(mx[k], d)); }
        }
        if (lane_id() == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) { part[threadIdx.x >> 6][k] = mn[k]; part[threadIdx.x >> 6][3 + k] = mx[k]; }
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            const int k = (int)threadIdx.x;
            T v = part[0][k];
            for (int w = 1; w < 4; w++) v = k < 3 ? join_min(v, part[w][k]) : join_max(v, part[w][k]);
            bounds[6 * (size_t)blockIdx.x + k] = v;
        }
        return;
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = xforms[12 * (size_t)i + k];
    // cofactors of the 3x3 part: C[j][k] belongs to m[j][k] (m[j][k] is m[4*j + k])
    T C[3][3];
    C[0][0] = cof<T>(m[5], m[10], m[6], m[9]);
    C[0][1] = cof<T>(m[6], m[8], m[4], m[10]);
    C[0][2] = cof<T>(m[4], m[9], m[5], m[8]);
    C[1][0] = cof<T>(m[2], m[9], m[1], m[10]);
    C[1][1] = cof<T>(m[0], m[10], m[2], m[8]);
    C[1][2] = cof<T>(m[1], m[8], m[0], m[9]);
    C[2][0] = cof<T>(m[1], m[6], m[2], m[5]);
    C[2][1] = cof<T>(m[2], m[4], m[0], m[6]);
    C[2][2] = cof<T>(m[0], m[5], m[1], m[4]);
    const T d0 = m[0] * C[0][0], d1 = m[1] * C[0][1], d2 = m[2] * C[0][2];
    const T d01 = d0 + d1;
    const T det = d01 + d2;
    const T r = (T)1 / det;
    InstRec<T> rec;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++) rec.y[4 * k + j] = C[j][k] * r;
        const T a = rec.y[4 * k] * m[3], b = rec.y[4 * k + 1] * m[7], c = rec.y[4 * k + 2] * m[11];
        const T ab = a + b;
        const T abc = ab + c;
        rec.y[4 * k + 3] = -abc;
    }
    const uint32_t slot = tree_of[i];
    rec.tree = slot; rec._pad[0] = 0; rec._pad[1] = 0; rec._pad[2] = 0;
    recs[i] = rec;
    // W_i: min / max over the 8 corners of B_slot, bit k of the corner number picks the max on axis k
    const T* B = bounds + 6 * (size_t)slot;
    T wmn[3], wmx[3];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        T p[3];
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = ((c >> k) & 1) ? B[3 + k] : B[k];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const T w = row4<T>(m + 4 * k, p);
            wmn[k] = c == 0 ? w : join_min(wmn[k], w);
            wmx[k] = c == 0 ? w : join_max(wmx[k], w);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { wboxes[6 * (size_t)i + k] = wmn[k]; wboxes[6 * (size_t)i + 3 + k] = wmx[k]; }
}

// ------------------------------------------------------------------------------------------------
// the two-level walk: one ray per lane, ONE loop.  A lane's state is (array, index, end, ray): inst == NONE means the top-level array
// and the world ray, otherwise member `inst`'s array and the object-space ray.  No loop is nested inside a top-level leaf, so the lanes of
// a wave keep stepping together whatever level each of them is on.
// MASKED: inst_mask is the set's n u32, ray_mask NULL (all ones) or n_rays u32; instance i is visible to the ray iff the two share a bit.  An
// invisible instance costs its mask's load: no record, no re-expressed ray, no member node — the lane goes on at i + 1 in the top level.
// Without MASKED neither pointer is read and the test is not compiled.
// ------------------------------------------------------------------------------------------------
// The kernel text stands at the end of this file, behind INSTANCES_TRACE_KERNEL_TEXT, and is compiled twice by the two includes of this file below:
// once under the kernels' own names with the TRIANGLE leaf stage — the same text under the same names and template heads as before a set had
// a leaf kind, hence the same instructions — and once as the *_leaf kernels with a LEAF template argument for BOX and SPHERE sets
// (DESIGN.md §4t).  INST_K(name): the kernel's name; INST_LEAF_TPARAM: the end of its template head; INST_LEAF_VALUE: its leaf kind.
#define INSTANCES_TRACE_KERNEL_TEXT
#define INST_K(name) name
#define INST_LEAF_TPARAM
#define INST_LEAF_VALUE LEAF_TRIANGLE
#include "instances.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#define INST_K(name) name##_leaf
#define INST_LEAF_TPARAM , int LEAF_ARG
#define INST_LEAF_VALUE LEAF_ARG
#include "instances.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#undef INSTANCES_TRACE_KERNEL_TEXT

// ------------------------------------------------------------------------------------------------
template <typename T> void instances_commit(bvhgpu_instances* s) {
    bvhgpu_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    s->committed = false;
    const size_t nt = s->trees.size(), n = s->n;
    s->seen.resize(nt);
    s->table_host.resize(nt * sizeof(InstTree<T>));
    InstTree<T>* host = reinterpret_cast<InstTree<T>*>(s->table_host.data());
    for (size_t k = 0; k < nt; k++) {
        bvhgpu_tree* t = s->trees[k];
        ensure_flat_arrays(t);   // (a lazy flatten owes the binary array)
        join_flat(t);
        // the array the set's leaf kind reads: the staleness check (capi.hip instances_current) watches this one; a BOX set reads aabbs alone
        const DevBuf* prims = s->leaf == BVHGPU_LEAF_TRIANGLE ? &t->tris : (s->leaf == BVHGPU_LEAF_SPHERE ? &t->spheres : &t->aabbs);
        s->seen[k] = bvhgpu_instances::Seen{t->trav.p, t->aabbs.p, s->leaf == BVHGPU_LEAF_BOX ? nullptr : prims->p, t->n, t->n_trav, t->gen};
        host[k] = InstTree<T>{t->trav.as<TravNode<T>>(), prims->as<T>(), t->aabbs.as<T>(), (uint32_t)t->n_trav, (uint32_t)t->n};
    }
    if (n && nt) {
        s->table.reserve(nt * sizeof(InstTree<T>));
        s->bounds.reserve(nt * 6 * sizeof(T));
        s->recs.reserve(n * sizeof(InstRec<T>));
        s->wboxes.reserve(n * 6 * sizeof(T));
        BVH_HIP(hipMemcpyAsync(s->table.p, host, nt * sizeof(InstTree<T>), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((k_instances_prep<T, 0>), dim3((unsigned)nt), dim3(256), 0, st, s->table.as<InstTree<T>>(), s->bounds.as<T>(),
                           s->tree_of.as<uint32_t>(), s->xforms.as<T>(), (uint32_t)n, s->recs.as<InstRec<T>>(), s->wboxes.as<T>());
        hipLaunchKernelGGL((k_instances_prep<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->table.as<InstTree<T>>(),
                           s->bounds.as<T>(), s->tree_of.as<uint32_t>(), s->xforms.as<T>(), (uint32_t)n, s->recs.as<InstRec<T>>(),
                           s->wboxes.as<T>());
    }
    build_tree<T>(s->top, s->wboxes.as<T>(), n, true);   // (throws Fail::NonFinite on a NaN / infinite world box: the set stays uncommitted)
    ensure_flat_arrays(s->top);
    join_flat(s->top);
    BVH_HIP(hipStreamSynchronize(st));
    s->committed = true;
}

// masked: bvhgpu_instances_trace_masked_* — the set's masks against ray_mask_dev (NULL: all ones); otherwise ray_mask_dev is not looked at
template <typename T>
void instances_trace(bvhgpu_instances* s, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n_rays, bool first, T* out_vals_dev,
                     uint32_t* out_instance_dev, uint32_t* out_shape_dev, bool masked, const uint32_t* ray_mask_dev) {
    if (!n_rays) return;
    hipStream_t st = s->ctx->stream;
    const bvhgpu_tree* top = s->top;
    const uint32_t n_top = s->n ? (uint32_t)top->n_trav : 0u;
    const dim3 grid((unsigned)((n_rays + 255) / 256)), block(256);
#define INST_TRACE_K(K, M)                                                                                                                     \
    hipLaunchKernelGGL(K, grid, block, 0, st, top->trav.as<TravNode<T>>(), n_top, s->recs.as<InstRec<T>>(),                                    \
                       s->table.as<InstTree<T>>(), rays_dev, tmax_dev, (uint32_t)n_rays, out_vals_dev, out_instance_dev, out_shape_dev,       \
                       M ? s->masks.as<uint32_t>() : nullptr, M ? ray_mask_dev : nullptr)
#define INST_TRACE(F, M)                                                                                                                       \
    do {                                                                                                                                       \
        if (s->leaf == BVHGPU_LEAF_TRIANGLE) INST_TRACE_K((k_instances_trace<T, F, M>), M);                                                    \
        else if (s->leaf == BVHGPU_LEAF_SPHERE) INST_TRACE_K((k_instances_trace_leaf<T, F, M, LEAF_SPHERE>), M);                               \
        else INST_TRACE_K((k_instances_trace_leaf<T, F, M, LEAF_BOX>), M);                                                                     \
    } while (0)
    if (masked) { if (first) INST_TRACE(true, true); else INST_TRACE(false, true); }
    else { if (first) INST_TRACE(true, false); else INST_TRACE(false, false); }
#undef INST_TRACE
#undef INST_TRACE_K
    BVH_HIP(hipGetLastError());
}

template void instances_commit<float>(bvhgpu_instances*);
template void instances_commit<double>(bvhgpu_instances*);
template void instances_trace<float>(bvhgpu_instances*, const bvhgpu_ray_f32*, const float*, size_t, bool, float*, uint32_t*, uint32_t*, bool,
                                     const uint32_t*);
template void instances_trace<double>(bvhgpu_instances*, const bvhgpu_ray_f64*, const double*, size_t, bool, double*, uint32_t*, uint32_t*, bool,
                                      const uint32_t*);

}  // namespace bvhgpu

#else   // INSTANCES_TRACE_KERNEL_TEXT: the kernel text, inside namespace bvhgpu (see the includes of this file above)

template <typename T, bool FIRST, bool MASKED INST_LEAF_TPARAM>
__global__ __launch_bounds__(256) void INST_K(k_instances_trace)(const TravNode<T>* __restrict__ top, uint32_t n_top, const InstRec<T>* __restrict__ recs,
                                                                 const InstTree<T>* __restrict__ tbl, const typename Traits<T>::Ray* __restrict__ rays,
                                                                 const T* __restrict__ tmax, uint32_t n_rays, T* __restrict__ out_vals,
                                                                 uint32_t* __restrict__ out_instance, uint32_t* __restrict__ out_shape,
                                                                 const uint32_t* __restrict__ inst_mask, const uint32_t* __restrict__ ray_mask) {
    constexpr int LEAF = INST_LEAF_VALUE;
    constexpr uint32_t W = LeafVals<LEAF>::W;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < n_rays;
    uint32_t rmask = 0xFFFFFFFFu;
    if constexpr (MASKED) { if (active && ray_mask) rmask = ray_mask[r]; }
    T o[3] = {0, 0, 0}, d[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
    T best[3] = {Traits<T>::inf(), 0, 0};
    uint32_t best_inst = NONE, best_shape = NONE;
    T tm = Traits<T>::inf();
    bool fin = true, wfin = true;   // the current ray / the world ray passes ray_is_finite (the NaN-free slab test is exact for it)
    if (active) {
        const typename Traits<T>::Ray* rp = rays + r;
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; inv[k] = rp->inv[k]; }
        if (tmax) tm = tmax[r];
        wfin = ray_is_finite<T>(o, inv);
        fin = wfin;
    }
    const TravNode<T>* nodes = top;
    const T* prims = nullptr;
    uint32_t i = 0, end = active ? n_top : 0u, inst = NONE, top_next = 0;
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
                if (inst != NONE) {   // a shape of the member: candidate (inst, shape), its record by the set's leaf kind
                    T v[3];
                    if constexpr (LEAF == LEAF_TRIANGLE) ray_triangle<T>(o, d, prims + 9 * (size_t)nd.shape, v);   // (leaf_record's triangle stage, spelt out)
                    else leaf_record<T, LEAF>(o, d, inv, prims, nd.shape, v);
                    if (v[0] < tm && (FIRST || v[0] < best[0])) {   // strict: the earlier candidate keeps a tie
                        best[0] = v[0]; best[1] = v[1]; best[2] = v[2]; best_inst = inst; best_shape = nd.shape;
                        if (FIRST) { i = 0; end = 0; inst = NONE; }   // the ray is done
                    }
                } else {              // an instance's world box: into its tree with the ray in the object's frame
                    bool visible = true;
                    if constexpr (MASKED) visible = (inst_mask[nd.shape] & rmask) != 0u;   // (hidden: the lane stays here and goes on at i + 1)
                    if (visible) {
                        top_next = i;
                        inst = nd.shape;
                        const InstRec<T> rec = load_rec<T>(recs + inst);
                        const InstTree<T> t = tbl[rec.tree];
                        T oo[3], dd[3];
#pragma unroll
                        for (int k = 0; k < 3; k++) { oo[k] = row4<T>(rec.y + 4 * k, o); dd[k] = row3<T>(rec.y + 4 * k, d); }
#pragma unroll
                        for (int k = 0; k < 3; k++) { o[k] = oo[k]; d[k] = dd[k]; inv[k] = (T)1 / dd[k]; }
                        fin = ray_is_finite<T>(o, inv);
                        nodes = t.trav; prims = t.prims; i = 0; end = t.n_trav;
                    }
                }
            }
            if (inst != NONE && i >= end) {   // the member's array has ended: back to the top level, behind the leaf that sent the lane here
                const typename Traits<T>::Ray* rp = rays + r;
#pragma unroll
                for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; inv[k] = rp->inv[k]; }
                fin = wfin;
                nodes = top; i = top_next; end = n_top; inst = NONE;
            }
        }
    }
    if (active) {
        if constexpr (W == 3) { out_vals[3 * (size_t)r] = best[0]; out_vals[3 * (size_t)r + 1] = best[1]; out_vals[3 * (size_t)r + 2] = best[2]; }
        else { out_vals[2 * (size_t)r] = best[0]; out_vals[2 * (size_t)r + 1] = best[1]; }
        out_instance[r] = best_inst; out_shape[r] = best_shape;
    }
}

#endif   // INSTANCES_TRACE_KERNEL_TEXT
