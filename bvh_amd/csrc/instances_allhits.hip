// instances_allhits.hip — every hit of every ray over an instance set, in order, as a CSR (bvhgpu_instances_allhits_*; include/bvh_mi355x.h,
// DESIGN.md §4m).
//
// The definition is the candidate table of bvhgpu_instances_trace_* (instances.hip) without the cut to one winner: ray j meets the pairs
// (instance, shape) in the double order — the instances in the order of the top level's list, within each the shapes in the order of the
// member's list — and (i, s) is a candidate iff its distance < tmax[j], strict, in T.  Row j is ALL candidates in a stable ascending sort by
// distance, or with BVHGPU_INSTANCES_ALLHITS_LIST_ORDER in the double order.  A candidate's distance is never NaN (it passed a strict <), so
// the sorted order is the total order on (distance, position in the double order): it is unique whatever produces it.  No pruning: both
// walks visit the whole double order (§4e's inverted-box reason, §4j).
//
// The batch is rows.hip's schedule (count walk, scan, ONE host read, offsets, fill walk, a workgroup per long row); every walk is
// k_instances_trace's loop, one ray per lane (instances_walk).  What this family puts into it:
//   k_instances_allhits_count     counts[q] = the candidates of ray q
//   k_instances_allhits_fill      A row of a sorted batch up to INST_ALLHITS_LANE_ROW_MAX is built by the lane's stable insertion (search from
//                                 the back with the strict <) on its own region — the key of element e lives in vals[e * 3] — and the
//                                 whole records are then computed again from the world ray and (instance, shape).  A LIST_ORDER row gets
//                                 its records appended as the walk meets them.  A longer row of a sorted batch gets (distance, instance)
//                                 appended in the double order, its shapes into a scratch row in the same order (and its positions, beyond
//                                 INST_ALLHITS_LDS_ROW_MAX) and is left to
//   k_instances_allhits_sort_row  rows_bitonic on the keys (distance, position) with the instance as payload, in LDS up to
//                                 INST_ALLHITS_LDS_ROW_MAX elements, in place in global memory beyond; the shape of an element is gathered
//                                 from the scratch row by its position; then the records of the row.
// The row length is uniform per workgroup of k_instances_allhits_sort_row: every loop bound and every barrier there depends on it alone.
//
// MASKED (bvhgpu_instances_allhits_masked_*): instances_walk passes over an instance whose mask shares no bit with the ray's, at
// its top-level leaf.  The count walk and the fill walk read the same two arrays and so take the same decision for every (ray, instance): the
// offsets are what the fill writes.  k_instances_allhits_sort_row and inst_record only ever see pairs that are already in a row: no mask.
#ifndef INSTANCES_ALLHITS_KERNEL_TEXT
#include <cstdio>

#include "instances.hpp"
#include "rows.hpp"
#include "walk.hpp"

namespace bvhgpu {

// Thresholds: all-hits' (allhits.hip), taken over unmeasured for this family.  An element sorted in LDS is an f64 key, a
// position and an instance — rows_lds_row_max_ok's 16 bytes: 32 KB a row in f64, 24 KB in f32; the shapes stay in global memory.
constexpr uint32_t INST_ALLHITS_LANE_ROW_MAX = 32;
constexpr uint32_t INST_ALLHITS_LDS_ROW_MAX = 2048;
static_assert(rows_lds_row_max_ok(INST_ALLHITS_LDS_ROW_MAX), "a row sorted in LDS must fit a workgroup's LDS, padded to a power of two");

// what both walks and the sort-row kernel read of the set
template <typename T> struct InstScene {
    const TravNode<T>* top;
    uint32_t n_top;
    const InstRec<T>* recs;
    const InstTree<T>* tbl;
};

// {distance, u, v} of (inst, s) for the WORLD ray (o, d): the world ray in the instance's frame by k_instances_trace's sequence, then the
// triangle test — the operands and the operations of the walk, hence its bits
template <typename T, int LEAF>
__device__ __forceinline__ void inst_record(const InstScene<T>& sc, const T o[3], const T d[3], uint32_t inst, uint32_t s, T v[3]) {
    const InstRec<T> rec = load_rec<T>(sc.recs + inst);
    const InstTree<T> t = sc.tbl[rec.tree];
    T oo[3], dd[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { oo[k] = row4<T>(rec.y + 4 * k, o); dd[k] = row3<T>(rec.y + 4 * k, d); }
    T ii[3] = {0, 0, 0};
    if (LEAF == LEAF_BOX) {   // (only the box stage reads the inverse: the walk's, from the object-space direction)
#pragma unroll
        for (int k = 0; k < 3; k++) ii[k] = (T)1 / dd[k];
    }
    leaf_record<T, LEAF>(oo, dd, ii, t.prims, s, v);
}

// k_instances_trace's loop: one ray per lane, ONE loop; a lane is either in the top-level array with the world ray (inst == NONE) or in a
// member's array with the object-space ray.  on_candidate(instance, shape, {distance, u, v}) for every pair of the double order whose
// distance is below tm.  Every lane of the wave calls it (the slab test's variant is chosen per wave); a lane with !active walks nothing.
// MASKED: rmask is the ray's mask; an instance with (mk.inst[i] & rmask) == 0 is passed over at its leaf — no record, no re-expressed ray, no
// member node — and the lane goes on at i + 1 in the top level.
template <typename T, bool MASKED, int LEAF, typename F>
__device__ __forceinline__ void instances_walk(const InstScene<T>& sc, const typename Traits<T>::Ray* __restrict__ rp, bool active, T tm,
                                               const uint32_t* __restrict__ inst_mask, uint32_t rmask, F&& on_candidate) {
    T o[3] = {0, 0, 0}, d[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
    bool fin = true, wfin = true;   // the current ray / the world ray passes ray_is_finite (the NaN-free slab test is exact for it)
    if (active) {
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; inv[k] = rp->inv[k]; }
        wfin = ray_is_finite<T>(o, inv);
        fin = wfin;
    }
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
                    leaf_record<T, LEAF>(o, d, inv, prims, nd.shape, v);
                    if (v[0] < tm) on_candidate(inst, nd.shape, v);
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
                        for (int k = 0; k < 3; k++) { oo[k] = row4<T>(rec.y + 4 * k, o); dd[k] = row3<T>(rec.y + 4 * k, d); }
#pragma unroll
                        for (int k = 0; k < 3; k++) { o[k] = oo[k]; d[k] = dd[k]; inv[k] = (T)1 / dd[k]; }
                        fin = ray_is_finite<T>(o, inv);
                        nodes = t.trav; prims = t.prims; i = 0; end = t.n_trav;
                    }
                }
            }
            if (inst != NONE && i >= end) {   // the member's array has ended: back to the top level, behind the leaf that sent the lane here
#pragma unroll
                for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; inv[k] = rp->inv[k]; }
                fin = wfin;
                nodes = sc.top; i = top_next; end = sc.n_top; inst = NONE;
            }
        }
    }
}

// The kernel text stands at the end of this file, behind INSTANCES_ALLHITS_KERNEL_TEXT, and is compiled twice by the two includes of this file below:
// once under the kernels' own names with the TRIANGLE leaf stage — the same text under the same names and template heads as before a set had
// a leaf kind, hence the same instructions — and once as the *_leaf kernels with a LEAF template argument for BOX and SPHERE sets
// (DESIGN.md §4t).  INST_K(name): the kernel's name; INST_LEAF_TPARAM: the end of its template head; INST_LEAF_VALUE: its leaf kind.
#define INSTANCES_ALLHITS_KERNEL_TEXT
#define INST_K(name) name
#define INST_LEAF_TPARAM
#define INST_LEAF_VALUE LEAF_TRIANGLE
#include "instances_allhits.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#define INST_K(name) name##_leaf
#define INST_LEAF_TPARAM , int LEAF_ARG
#define INST_LEAF_VALUE LEAF_ARG
#include "instances_allhits.hip"
#undef INST_K
#undef INST_LEAF_TPARAM
#undef INST_LEAF_VALUE
#undef INSTANCES_ALLHITS_KERNEL_TEXT

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool MASKED, int LEAF>
static void instances_allhits_launch(bvhgpu_instances* s, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, bool sorted, bool count_only,
                                     bvhgpu_hits* h, const uint32_t* ray_mask_dev) {
    hipStream_t st = s->ctx->stream;
    const InstMasks mk = {MASKED ? s->masks.as<uint32_t>() : nullptr, MASKED ? ray_mask_dev : nullptr};
    const InstScene<T> sc = {s->top->trav.as<TravNode<T>>(), (uint32_t)s->top->n_trav, s->recs.as<InstRec<T>>(), s->table.as<InstTree<T>>()};
    const uint32_t n32 = (uint32_t)n;
    const dim3 rgrid((unsigned)((n + 255) / 256)), block(256);
    const RowsPlan plan = {sorted, count_only, INST_ALLHITS_LANE_ROW_MAX, INST_ALLHITS_LDS_ROW_MAX, LeafVals<LEAF>::W * sizeof(T), true, true};
    rows_run(h, n, plan,
             [&](uint32_t* counts) {
                 if constexpr (LEAF == LEAF_TRIANGLE)
                     hipLaunchKernelGGL((k_instances_allhits_count<T, MASKED>), rgrid, block, 0, st, sc, rays_dev, tmax_dev, n32, counts, mk);
                 else
                     hipLaunchKernelGGL((k_instances_allhits_count_leaf<T, MASKED, LEAF>), rgrid, block, 0, st, sc, rays_dev, tmax_dev, n32, counts, mk);
             },
             [&](const RowsOut& o, auto SORTED) {
                 if constexpr (LEAF == LEAF_TRIANGLE)
                     hipLaunchKernelGGL((k_instances_allhits_fill<T, decltype(SORTED)::value, MASKED>), rgrid, block, 0, st, sc, rays_dev, tmax_dev, n32,
                                        o.offsets, o.instance, o.shape, static_cast<T*>(o.vals), o.list_shape, o.pos, mk);
                 else
                     hipLaunchKernelGGL((k_instances_allhits_fill_leaf<T, decltype(SORTED)::value, MASKED, LEAF>), rgrid, block, 0, st, sc, rays_dev, tmax_dev,
                                        n32, o.offsets, o.instance, o.shape, static_cast<T*>(o.vals), o.list_shape, o.pos, mk);
             },
             [&](const RowsOut& o, uint32_t n_long) {
                 if constexpr (LEAF == LEAF_TRIANGLE)
                     hipLaunchKernelGGL((k_instances_allhits_sort_row<T>), dim3(n_long), dim3(ROWS_SORT_THREADS), 0, st, sc, o.work, rays_dev, o.offsets,
                                        o.instance, o.shape, static_cast<T*>(o.vals), o.list_shape, o.pos);
                 else
                     hipLaunchKernelGGL((k_instances_allhits_sort_row_leaf<T, LEAF>), dim3(n_long), dim3(ROWS_SORT_THREADS), 0, st, sc, o.work, rays_dev,
                                        o.offsets, o.instance, o.shape, static_cast<T*>(o.vals), o.list_shape, o.pos);
             });
}
template <typename T, int LEAF>
static void instances_allhits_launch_leaf(bvhgpu_instances* s, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, bool sorted, bool count_only,
                                          bvhgpu_hits* h, bool masked, const uint32_t* ray_mask_dev) {
    if (masked) instances_allhits_launch<T, true, LEAF>(s, rays_dev, tmax_dev, n, sorted, count_only, h, ray_mask_dev);
    else instances_allhits_launch<T, false, LEAF>(s, rays_dev, tmax_dev, n, sorted, count_only, h, nullptr);
}

// masked: bvhgpu_instances_allhits_masked_* — the set's masks against ray_mask_dev (NULL: all ones); otherwise ray_mask_dev is not looked at
template <typename T>
void instances_allhits_batch(bvhgpu_instances* s, const typename Traits<T>::Ray* rays_dev, const T* tmax_dev, size_t n, unsigned flags, bvhgpu_hits* h,
                             bool masked, const uint32_t* ray_mask_dev) {
    const bool sorted = (flags & BVHGPU_INSTANCES_ALLHITS_LIST_ORDER) == 0;
    const bool count_only = (flags & BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY) != 0;
    char name[112];
    const char* m = masked ? "true" : "false";
    if (s->leaf == BVHGPU_LEAF_TRIANGLE) {
        if (count_only) std::snprintf(name, sizeof name, "bvhgpu::k_instances_allhits_count<%s, %s>", walk_type_name<T>(), m);
        else std::snprintf(name, sizeof name, "bvhgpu::k_instances_allhits_fill<%s, %s, %s>", walk_type_name<T>(), sorted ? "true" : "false", m);
    } else {
        if (count_only) std::snprintf(name, sizeof name, "bvhgpu::k_instances_allhits_count_leaf<%s, %s, %d>", walk_type_name<T>(), m, s->leaf);
        else std::snprintf(name, sizeof name, "bvhgpu::k_instances_allhits_fill_leaf<%s, %s, %s, %d>", walk_type_name<T>(), sorted ? "true" : "false", m, s->leaf);
    }
    rows_batch(h, s->ctx, Traits<T>::dtype, TRAVERSE_INST_ALLHITS, s->leaf, count_only, n, s->n == 0, name,   // (empty: no instances)
               [&] {
                   if (s->leaf == BVHGPU_LEAF_TRIANGLE) instances_allhits_launch_leaf<T, LEAF_TRIANGLE>(s, rays_dev, tmax_dev, n, sorted, count_only, h, masked, ray_mask_dev);
                   else if (s->leaf == BVHGPU_LEAF_SPHERE) instances_allhits_launch_leaf<T, LEAF_SPHERE>(s, rays_dev, tmax_dev, n, sorted, count_only, h, masked, ray_mask_dev);
                   else instances_allhits_launch_leaf<T, LEAF_BOX>(s, rays_dev, tmax_dev, n, sorted, count_only, h, masked, ray_mask_dev);
               });
}
template void instances_allhits_batch<float>(bvhgpu_instances*, const bvhgpu_ray_f32*, const float*, size_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);
template void instances_allhits_batch<double>(bvhgpu_instances*, const bvhgpu_ray_f64*, const double*, size_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);

}  // namespace bvhgpu

#else   // INSTANCES_ALLHITS_KERNEL_TEXT: the kernel text, inside namespace bvhgpu (see the includes of this file above)

template <typename T, bool MASKED INST_LEAF_TPARAM>
__global__ __launch_bounds__(256) void INST_K(k_instances_allhits_count)(InstScene<T> sc, const typename Traits<T>::Ray* __restrict__ rays,
                                                                         const T* __restrict__ tmaxs, uint32_t n, uint32_t* __restrict__ counts,
                                                                         InstMasks mk) {
    constexpr int LEAF = INST_LEAF_VALUE;
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = q < n;
    const T tm = active && tmaxs ? tmaxs[q] : Traits<T>::inf();
    uint32_t rmask = 0xFFFFFFFFu;
    if constexpr (MASKED) { if (active && mk.ray) rmask = mk.ray[q]; }
    uint32_t cnt = 0;
    instances_walk<T, MASKED, LEAF>(sc, rays + (active ? q : 0u), active, tm, mk.inst, rmask, [&](uint32_t, uint32_t, const T*) { cnt++; });
    if (active) counts[q] = cnt;
}

// ---- the second walk ----------------------------------------------------------------------------------------------------------------
// list_shape: NULL, or total u32 — the shapes of the long rows in the double order (a sorted batch that has long rows)
// pos:        NULL, or total u32 — the positions of the rows beyond INST_ALLHITS_LDS_ROW_MAX (a sorted batch that has such rows)
template <typename T, bool SORTED, bool MASKED INST_LEAF_TPARAM>
__global__ __launch_bounds__(256) void INST_K(k_instances_allhits_fill)(InstScene<T> sc, const typename Traits<T>::Ray* __restrict__ rays,
                                                                        const T* __restrict__ tmaxs, uint32_t n, const uint32_t* __restrict__ offsets,
                                                                        uint32_t* __restrict__ instance, uint32_t* __restrict__ shape, T* __restrict__ vals,
                                                                        uint32_t* __restrict__ list_shape, uint32_t* __restrict__ pos, InstMasks mk) {
    constexpr int LEAF = INST_LEAF_VALUE;
    constexpr uint32_t W = LeafVals<LEAF>::W;
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t beg = q < n ? offsets[q] : 0u, len = q < n ? offsets[q + 1] - beg : 0u;
    // (the count pass walked an empty row's ray: nothing to write.  Leaving it out can change the wave's `fast` choice against the count
    // walk's — only ever towards slab_hit_finite, which is exact for every lane whose own ray is finite: the same candidates either way)
    const bool active = len != 0;
    const typename Traits<T>::Ray* rp = rays + (active ? q : 0u);
    const T tm = active && tmaxs ? tmaxs[q] : Traits<T>::inf();
    uint32_t* __restrict__ ri = instance + beg;
    uint32_t* __restrict__ rs = shape + beg;
    T* __restrict__ rv = vals + (size_t)beg * W;
    const bool insert = SORTED && len <= INST_ALLHITS_LANE_ROW_MAX;
    const bool with_list = SORTED && !insert && list_shape != nullptr;
    const bool with_pos = SORTED && pos != nullptr && len > INST_ALLHITS_LDS_ROW_MAX;
    uint32_t rmask = 0xFFFFFFFFu;
    if constexpr (MASKED) { if (active && mk.ray) rmask = mk.ray[q]; }   // (the count walk's decision: the same two arrays)
    uint32_t cnt = 0;
    instances_walk<T, MASKED, LEAF>(sc, rp, active, tm, mk.inst, rmask, [&](uint32_t inst, uint32_t s, const T* v) {
        if (cnt >= len) return;   // (never: this walk is the count pass's; a lane stays inside its own region whatever happens)
        if (insert) {
            // ascending list: the first element e with dist < e is where a scan from the back stops, so search and shift are one loop
            const T dist = v[0];
            uint32_t hole = cnt;
#pragma unroll 1
            while (hole > 0) {
                const T e = rv[(size_t)(hole - 1) * W];
                if (!(dist < e)) break;
                rv[(size_t)hole * W] = e;
                ri[hole] = ri[hole - 1];
                rs[hole] = rs[hole - 1];
                hole--;
            }
            rv[(size_t)hole * W] = dist;
            ri[hole] = inst;
            rs[hole] = s;
        } else if (SORTED) {   // a long row: (distance, instance) and the shape in the double order for k_instances_allhits_sort_row
            rv[(size_t)cnt * W] = v[0];
            ri[cnt] = inst;
            if (with_list) list_shape[beg + cnt] = s;
            if (with_pos) pos[beg + cnt] = cnt;
        } else {               // the double order: the record as the walk meets it
            ri[cnt] = inst;
            rs[cnt] = s;
#pragma unroll
            for (uint32_t c = 0; c < W; c++) rv[(size_t)cnt * W + c] = v[c];
        }
        cnt++;
    });
    if (insert && active) {
        // the whole record of every element, computed again from the world ray and (instance, shape)
        T o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; }
#pragma unroll 1
        for (uint32_t j = 0; j < cnt; j++) {
            T v[3];
            inst_record<T, LEAF>(sc, o, d, ri[j], rs[j], v);
#pragma unroll
            for (uint32_t c = 0; c < W; c++) rv[(size_t)j * W + c] = v[c];
        }
    }
}

// one workgroup per long row of a sorted batch
template <typename T INST_LEAF_TPARAM>
__global__ __launch_bounds__(ROWS_SORT_THREADS) void INST_K(k_instances_allhits_sort_row)(InstScene<T> sc, const uint32_t* __restrict__ work,
                                                                                         const typename Traits<T>::Ray* __restrict__ rays,
                                                                                         const uint32_t* __restrict__ offsets, uint32_t* instance,
                                                                                         uint32_t* shape, T* vals, const uint32_t* __restrict__ list_shape,
                                                                                         uint32_t* pos) {
    constexpr int LEAF = INST_LEAF_VALUE;
    constexpr uint32_t W = LeafVals<LEAF>::W;
    __shared__ T ld[INST_ALLHITS_LDS_ROW_MAX];
    __shared__ uint32_t lp[INST_ALLHITS_LDS_ROW_MAX];
    __shared__ uint32_t li[INST_ALLHITS_LDS_ROW_MAX];
    const uint32_t q = work[blockIdx.x];
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;   // uniform over the workgroup
    uint32_t P = 1;
    while (P < len) P <<= 1;
    uint32_t* ri = instance + beg;
    uint32_t* rs = shape + beg;
    T* rv = vals + (size_t)beg * W;
    const bool in_lds = len <= INST_ALLHITS_LDS_ROW_MAX;
    if (in_lds) {
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) { ld[e] = rv[(size_t)e * W]; lp[e] = e; li[e] = ri[e]; }
        __syncthreads();
        rows_bitonic<T, false>(ld, 1u, lp, li, len, P);
    } else {   // (the host passes the positions whenever a row is this long, and checks that it does)
        __threadfence_block();
        __syncthreads();
        rows_bitonic<T, true>(rv, W, pos + beg, ri, len, P);
    }
    // the records of the row, from the world ray and the sorted (instance, shape) (the network ended with a barrier)
    const typename Traits<T>::Ray* rp = rays + q;
    T o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; d[k] = rp->d[k]; }
    for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) {
        const uint32_t p = in_lds ? lp[e] : pos[beg + e];
        const uint32_t inst = in_lds ? li[e] : ri[e];
        if (p >= len) continue;   // (the positions are a permutation of 0 .. len - 1: no read beyond the row's scratch whatever happens)
        const uint32_t s = list_shape[beg + p];
        T v[3];
        inst_record<T, LEAF>(sc, o, d, inst, s, v);
        if (in_lds) ri[e] = inst;
        rs[e] = s;
#pragma unroll
        for (uint32_t c = 0; c < W; c++) rv[(size_t)e * W + c] = v[c];
    }
}

#endif   // INSTANCES_ALLHITS_KERNEL_TEXT
