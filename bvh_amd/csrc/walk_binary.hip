// walk_binary.hip — the two walks over the engine's folded pre-order array (common.hpp TravNode) for a BATCH of rays, in exactly the
// reference's visit order (<FlatBvh as BoundingHierarchy>::traverse, src/flat_bvh.rs:396-431; slab test src/ray/intersect_default.rs:16-37
// → hit: i+1, miss: exit): k_traverse (one ray per lane per launch; small or coherent batches) and k_traverse_lds (persistent workgroups,
// top of the tree resident in LDS, ray refill; large batches).  launch_binary picks the instantiation for traverse_enqueue (traverse.hip).
#include <cstdio>

#include "walk.hpp"

namespace bvhgpu {

// ------------------------------------------------------------------------------------------------
// one ray per lane per launch
// ------------------------------------------------------------------------------------------------
template <typename T, int MODE, bool STATS>
__global__ __launch_bounds__(256) void k_traverse(const TravNode<T>* __restrict__ nodes, uint32_t n_trav,
                                                  const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays,
                                                  WalkOut<T> w) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    const bool active = r < n_rays;
    LaneRay<T, MODE> ray;
    ray.clear();
    if (active) ray.load(rays, r, w.tmax);
    uint32_t i = active ? 0u : n_trav;
    PoolCursor pc;
    unsigned long long steps = 0, leaf_steps = 0, wsteps = 0;
    // wave-uniform: every ray of this wave is finite → the NaN-free slab test (common.hpp) is exact (it does not return the t-slice, which
    // T_SLICE and the box modes need of every leaf)
    const bool fast = MODE != MODE_T_SLICE && !mode_box(MODE) && !__any(active && !ray.fin);
    while (true) {
        const bool run = i < n_trav;
        if (!__any(run)) break;
        bool rec = false;
        uint32_t shape = NONE;
        T t0 = 0, t1 = 0;
        if (STATS) wsteps++;
        if (run) {
            const NodeRegs<T> nd = load_node(nodes + i);
            const bool hit = fast ? slab_hit_finite<T>(ray.o, ray.inv, nd.mn, nd.mx)
                                  : slab_hit<T>(ray.o, ray.inv, nd.mn, nd.mx, t0, t1);
            shape = nd.shape;
            const bool leaf = trav_is_leaf(shape);
            rec = hit && leaf;
            i = hit ? i + 1 : nd.exit;   // a leaf's exit IS i+1
            if (STATS) { steps++; leaf_steps += leaf ? 1 : 0; }
        }
        report<T, MODE>(rec, shape, t0, t1, ray, w, pc, lane, lt);
        if (mode_first(MODE) && ray.best_prim != NONE) i = n_trav;   // occluded: the ray is done
    }
    const unsigned long long cands = active ? ray.cnt : 0;
    if (active) ray.retire(w);
    walk_epilogue<T, MODE>(w, pc, lane, STATS, steps, leaf_steps, wsteps, cands);
}

// ------------------------------------------------------------------------------------------------
// LDS-resident top of the tree.  On the 120k-triangle scene 72 % of all box tests touch the first 11
// levels of the tree (2047 entries) and the vector L1 — one tag lookup per lane per 16-byte load for
// these scattered reads — is the unit that saturates (measured: ~1 lane-access per clock per CU).  A
// 1024-thread workgroup copies the entries whose heap number is below K into LDS (split into 16-byte
// planes so that a ds_read_b128 of 16 lanes spreads over all 16 bank quads; 2 workgroups of 64 KB per
// CU) and every lane tracks the slot of its current entry: descend → 2*slot, miss → the exit's slot
// carried in the entry's spare word.  A lane outside the resident set (deep in the tree, or after a
// leaf) reads L2 as before and re-enters the resident set through the same word.
// The workgroup's waves draw rays from ONE cursor in LDS (a wave-aggregated ds_add per refill phase), so
// the tail of a launch is the tail of a workgroup's ray range, not of every wave's.  Retiring and
// refilling lanes is kept OUT of the walk loop: LDS_INNER lean steps (~38 VALU each), then one refill
// phase; a lane whose ray ends mid-way idles for at most LDS_INNER-1 steps.
// ------------------------------------------------------------------------------------------------
template <typename T> struct TopLds;
template <> struct TopLds<float> {
    static constexpr uint32_t BYTES_PER_SLOT = 32;
    float4 *lo, *hi;
    __device__ __forceinline__ TopLds(unsigned char* base, uint32_t K) {
        lo = reinterpret_cast<float4*>(base); hi = lo + K;
    }
    __device__ __forceinline__ void store(uint32_t q, const TravNode<float>* g) {
        const float4* p = reinterpret_cast<const float4*>(g);
        lo[q] = p[0]; hi[q] = p[1];
    }
    __device__ __forceinline__ NodeRegs<float> load(uint32_t q) const {
        const float4 a = lo[q], b = hi[q];
        NodeRegs<float> r;
        r.mn[0] = a.x; r.mn[1] = a.y; r.mn[2] = a.z; r.exit = __float_as_uint(a.w);
        r.mx[0] = b.x; r.mx[1] = b.y; r.mx[2] = b.z; r.shape = __float_as_uint(b.w);
        return r;
    }
};
template <> struct TopLds<double> {
    static constexpr uint32_t BYTES_PER_SLOT = 56;
    double2 *a, *b, *c;
    uint2* d;
    __device__ __forceinline__ TopLds(unsigned char* base, uint32_t K) {
        a = reinterpret_cast<double2*>(base); b = a + K; c = b + K; d = reinterpret_cast<uint2*>(c + K);
    }
    __device__ __forceinline__ void store(uint32_t q, const TravNode<double>* g) {
        const double2* p = reinterpret_cast<const double2*>(g);
        a[q] = p[0]; b[q] = p[1]; c[q] = p[2];
        const unsigned long long es = (unsigned long long)__double_as_longlong(p[3].x);
        d[q] = make_uint2((uint32_t)(es & 0xFFFFFFFFull), (uint32_t)(es >> 32));
    }
    __device__ __forceinline__ NodeRegs<double> load(uint32_t q) const {
        const double2 x = a[q], y = b[q], z = c[q];
        const uint2 w = d[q];
        NodeRegs<double> r;
        r.mn[0] = x.x; r.mn[1] = x.y; r.mn[2] = y.x;
        r.mx[0] = y.y; r.mx[1] = z.x; r.mx[2] = z.y;
        r.exit = w.x; r.shape = w.y;
        return r;
    }
};

constexpr int LDS_THREADS = 1024;
#ifndef BVH_LDS_INNER
#define BVH_LDS_INNER 8
#endif
constexpr int LDS_INNER = BVH_LDS_INNER;   // walk steps between two refill phases (4 / 6 / 8 / 10 / 12 / 16 measured: 8)

template <typename T, int MODE, bool STATS>
__global__ __launch_bounds__(LDS_THREADS) void k_traverse_lds(const TravNode<T>* __restrict__ nodes, uint32_t n_trav,
                                                               const uint32_t* __restrict__ slot_entry, uint32_t K,
                                                               uint32_t first_slot, uint32_t split,
                                                               const typename Traits<T>::Ray* __restrict__ rays,
                                                               uint32_t n_rays, uint32_t rays_per_wg, WalkOut<T> w) {
    // split != 0: every ray is walked as TWO independent items, item 2r over the entries of the root's left
    // subtree [0, split_at) and item 2r+1 over the right one [split_at, n_trav).  The per-ray list is the
    // concatenation of the two (pre-order!), so the CSR machinery simply runs over 2R items.  At 1 M rays a lane
    // only gets ~2 rays; halving the longest walks and doubling the items per lane shortens the tail of the launch.
    // (n_rays and rays_per_wg count items here.)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t& s_next = *reinterpret_cast<uint32_t*>(smem);
    TopLds<T> top(smem + 16, K);
    const uint32_t split_at = split ? load_node(nodes).exit : 0u;   // wave-uniform
    const unsigned long long g0 = (unsigned long long)blockIdx.x * rays_per_wg;
    const unsigned long long g1 = g0 + rays_per_wg;
    const uint32_t wg_begin = (uint32_t)(g0 < n_rays ? g0 : n_rays);
    const uint32_t wg_end = (uint32_t)(g1 < n_rays ? g1 : n_rays);
    if (threadIdx.x == 0) s_next = wg_begin;
    for (uint32_t q = threadIdx.x; q < K; q += blockDim.x) {
        const uint32_t e = slot_entry[q];
        if (e != NONE) top.store(q, nodes + e);
    }
    __syncthreads();

    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    LaneRay<T, MODE> ray;
    ray.clear();
    uint32_t i = 0, limit = 0, slot = SLOT_NONE;   // the walk runs while i < limit
    bool exhausted = wg_begin >= wg_end;   // wave-uniform: the workgroup's range has been handed out
    PoolCursor pc;
    unsigned long long steps = 0, leaf_steps = 0, wsteps = 0, cands = 0;
    while (true) {
        // ---- refill phase
        bool run = i < limit;
        const unsigned long long idle = __ballot(!run);
        if (idle) {
            if (!run && ray.r != NONE) { cands += ray.cnt; ray.retire(w); }
            if (!exhausted) {
                const uint32_t nidle = (uint32_t)__popcll(idle);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_next, nidle);
                base = __builtin_amdgcn_readfirstlane(base);
                const uint32_t mine = base + (uint32_t)__popcll(idle & lt);
                if (!run && base < wg_end && mine < wg_end) {
                    if (split_at) {
                        const bool right = (mine & 1u) != 0u;
                        ray.load(rays, mine >> 1, w.tmax);
                        ray.r = mine;                       // counts / pool records are per item
                        i = right ? split_at : 0u; limit = right ? n_trav : split_at;
                        slot = right ? 3u : 2u;             // heap numbers of the root's children
                    } else {
                        ray.load(rays, mine, w.tmax);
                        i = 0; limit = n_trav; slot = first_slot;
                    }
                    run = true;
                }
                exhausted = base >= wg_end || (wg_end - base) <= nidle;
            }
            if (!__any(run)) break;
        }
        const bool fast = MODE != MODE_T_SLICE && !mode_box(MODE) && !__any(run && !ray.fin);   // wave-uniform
        // ---- LDS_INNER walk steps
        for (int s = 0; s < LDS_INNER; s++) {
            bool rec = false;
            uint32_t shape = NONE;
            T t0 = 0, t1 = 0;
            if (STATS) wsteps++;
            if (i < limit) {
                NodeRegs<T> nd;
                if (slot < K) nd = top.load(slot);
                else nd = load_node(nodes + i);
                const bool hit = fast ? slab_hit_finite<T>(ray.o, ray.inv, nd.mn, nd.mx)
                                      : slab_hit<T>(ray.o, ray.inv, nd.mn, nd.mx, t0, t1);
                shape = nd.shape;
                const bool leaf = trav_is_leaf(shape);
                rec = hit && leaf;
                const bool descend = hit && !leaf;
                i = descend ? i + 1 : nd.exit;   // a leaf's exit IS i+1
                const uint32_t child = min(slot << 1, SLOT_NONE);
                slot = descend ? child : (leaf ? SLOT_NONE : (shape & 0xFFFFu));
                if (STATS) { steps++; leaf_steps += leaf ? 1 : 0; }
            }
            report<T, MODE>(rec, shape, t0, t1, ray, w, pc, lane, lt);
            if (mode_first(MODE) && ray.best_prim != NONE) i = limit;   // occluded: retired at the next refill
        }
    }
    walk_epilogue<T, MODE>(w, pc, lane, STATS, steps, leaf_steps, wsteps, cands);
}

// ------------------------------------------------------------------------------------------------
template <typename T, int MODE, bool STATS>
static void launch_walk(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, bool use_lds,
                        uint32_t split_at) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    ensure_flat_arrays(t);   // (a lazy flatten wrote the wide walk's arrays only: the binary array and its LDS slot table follow now)
    const uint32_t n_trav = (uint32_t)t->n_trav;
    const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
    char name[128];
    std::snprintf(name, sizeof name, "bvhgpu::%s<%s, %d, %s>", use_lds ? "k_traverse_lds" : "k_traverse", walk_type_name<T>(), MODE,
                  STATS ? "true" : "false");
    if (!use_lds) {   // one ray per lane per launch
        hipLaunchKernelGGL((k_traverse<T, MODE, STATS>), dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, nodes,
                           n_trav, rays_dev, (uint32_t)n_rays, w);
        h->walk_kernel = name;
        return;
    }
    // workgroups of lds_threads that each keep K top-of-tree slots in LDS; as many per CU as 160 KB of LDS
    // and 32 waves allow
    // 0 = per-type default: as many slots as let TWO workgroups share a CU's 160 KB (f32: 2559 x 32 B, f64: 1462 x 56 B) — one
    // slot more halves the occupancy (0.206 → 0.296 ms on configs[1]); 1024 threads for f32, 512 for f64 (tools/f64_sweep.py)
    const bool wide = sizeof(T) == 8;
    const int two_per_cu = (int)(((160 * 1024) / 2 - 16) / TopLds<T>::BYTES_PER_SLOT);
    const int want_threads = ctx->tune[BVHGPU_TUNE_TRAVERSE_LDS_THREADS] > 0 ? ctx->tune[BVHGPU_TUNE_TRAVERSE_LDS_THREADS] : (wide ? 512 : 1024);
    const int want_slots = ctx->tune[BVHGPU_TUNE_TRAVERSE_LDS_SLOTS] > 0 ? ctx->tune[BVHGPU_TUNE_TRAVERSE_LDS_SLOTS] : two_per_cu;
    const uint32_t lds_threads = (uint32_t)std::min(LDS_THREADS, std::max(64, want_threads & ~63));
    const uint32_t K = (uint32_t)std::min<int>((int)TopCfg<T>::SLOTS, std::max(4, want_slots));
    const size_t lds_bytes = 16 + (size_t)K * TopLds<T>::BYTES_PER_SLOT;
    const uint32_t wg_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds_bytes, 2048 / lds_threads));
    const size_t n_items = split_at ? 2 * n_rays : n_rays;
    const size_t full = (n_items + WAVE - 1) / WAVE;
    const uint32_t n_waves = (uint32_t)std::min<size_t>(full, (size_t)ctx->n_cu * wg_per_cu * (lds_threads / WAVE));
    const dim3 lgrid((n_waves + lds_threads / WAVE - 1) / (lds_threads / WAVE));
    const uint32_t rpg = (uint32_t)((n_items + lgrid.x - 1) / lgrid.x);   // items per workgroup
    const uint32_t first_slot = t->n >= 2 ? 2u : SLOT_NONE;               // entry 0 is the root's left child (heap number 2)
    static thread_local size_t lds_attr[16] = {};   // per device: dynamic-LDS limit already set for this instantiation
    size_t& have = lds_attr[ctx->device & 15];
    if (have < lds_bytes) {
        BVH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_traverse_lds<T, MODE, STATS>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        have = lds_bytes;
    }
    hipLaunchKernelGGL((k_traverse_lds<T, MODE, STATS>), lgrid, dim3(lds_threads), lds_bytes, st, nodes, n_trav,
                       t->slot_entry.as<uint32_t>(), K, first_slot, split_at, rays_dev, (uint32_t)n_items, rpg, w);
    h->walk_kernel = name;
}

template <typename T>
void launch_binary(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, bool stats,
                   bool use_lds, uint32_t split_at) {
#define WALK(M, S) launch_walk<T, M, S>(t, rays_dev, n_rays, w, h, use_lds, split_at)
    switch (mode) {
        case MODE_INDICES: if (stats) WALK(MODE_INDICES, true); else WALK(MODE_INDICES, false); break;
        case MODE_T_SLICE: if (stats) WALK(MODE_T_SLICE, true); else WALK(MODE_T_SLICE, false); break;
        case MODE_TRIANGLES: if (stats) WALK(MODE_TRIANGLES, true); else WALK(MODE_TRIANGLES, false); break;
        case MODE_ANY: WALK(MODE_ANY, false); break;
        case MODE_BOX_CLOSEST: WALK(MODE_BOX_CLOSEST, false); break;
        case MODE_BOX_FIRST: WALK(MODE_BOX_FIRST, false); break;
        case MODE_SPHERE_CLOSEST: WALK(MODE_SPHERE_CLOSEST, false); break;
        case MODE_SPHERE_FIRST: WALK(MODE_SPHERE_FIRST, false); break;
        default: if (stats) WALK(MODE_CLOSEST, true); else WALK(MODE_CLOSEST, false); break;
    }
#undef WALK
}
template void launch_binary<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, size_t, const WalkOut<float>&, bvhgpu_hits*, int, bool, bool, uint32_t);
template void launch_binary<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, size_t, const WalkOut<double>&, bvhgpu_hits*, int, bool, bool, uint32_t);

}  // namespace bvhgpu
