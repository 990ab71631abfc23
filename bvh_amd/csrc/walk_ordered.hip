// walk_ordered.hip — the reference's ordered iterators over the BvhNode array, collected per ray: k_traverse_ordered (child-ordered
// depth-first iterator, LDS stack) and k_traverse_heap (best-first iterator, BinaryHeap).  launch_ordered picks the instantiation for
// traverse_enqueue (traverse.hip).
#include <cstdio>

#include "walk.hpp"

namespace bvhgpu {

// ------------------------------------------------------------------------------------------------
// Ordered traversal: Bvh::nearest_child_traverse_iterator / farthest_child_traverse_iterator
// (bvh_impl.rs:184-212, bvh/child_distance_traverse.rs) collected per ray.  The iterator is a depth-first walk
// over the BvhNode array that tests both child boxes of an inner node with intersection_slice_for_aabb and
// visits the higher-priority hit child first ((left_dist > right_dist) ^ !ASCENDING → right first, :126), the
// other afterwards; a leaf yields its shape.  One ray per lane; the iterator's 32-entry stack (:36) lives in LDS
// (entry-major, so a wave's push/pop is conflict-free).  An entry holds what the iterator would do on pop:
// nothing, "go to node X" (the rest child) or "yield shape S".  A tree deeper than 32 levels makes the reference
// index out of bounds (panic); here it raises the overflow flag.
// The same set of shapes as FlatBvh::traverse comes out (slice is Some exactly when intersects_aabb is true),
// in the iterator's order; the output modes of the other walks apply.
// ------------------------------------------------------------------------------------------------
constexpr int ORD_STACK = 32;
constexpr uint32_t ORD_NOTHING = 0xFFFFFFFFu;   // RestChild::None
constexpr uint32_t ORD_YIELD = 0x80000000u;     // | shape index: a leaf was pushed (:143-147)

template <typename T, int MODE, bool ASCENDING>
__global__ __launch_bounds__(256) void k_traverse_ordered(const typename Traits<T>::Node* __restrict__ nodes, uint32_t n_nodes,
                                                          const T* __restrict__ shape_aabbs,
                                                          const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays,
                                                          WalkOut<T> w, uint32_t* __restrict__ overflow) {
    __shared__ uint32_t s_stack[ORD_STACK][256];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    const bool active = r < n_rays;
    LaneRay<T, MODE> ray;
    ray.clear();
    if (active) ray.load(rays, r);
    uint32_t node_index = 0;
    int sp = 0;
    bool has_node = false;
    if (active && n_nodes) {   // iter_initially_has_node (iter.rs:164-182): a root leaf is pre-tested with the shape's AABB
        const uint32_t rs = nodes[0].shape;
        if (rs != NONE) {
            const T* sb = shape_aabbs + 6 * (size_t)rs;
            const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
            T t0, t1;
            has_node = slab_hit<T>(ray.o, ray.inv, mn, mx, t0, t1);
        } else {
            has_node = true;
        }
    }
    PoolCursor pc;
    bool ovf = false;
    while (true) {
        const bool run = has_node || sp > 0;
        if (!__any(run)) break;
        bool rec = false;
        uint32_t shape = NONE;
        if (run) {
            if (has_node) {   // move_first_priority (:88-148) + stack_push (:211-213)
                const typename Traits<T>::Node* nd = nodes + node_index;
                const uint32_t ns = nd->shape;
                uint32_t entry = ORD_NOTHING;
                if (ns != NONE) {
                    has_node = false;
                    entry = ORD_YIELD | ns;
                } else {
                    T lmn[3], lmx[3], rmn[3], rmx[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) { lmn[k] = nd->l_min[k]; lmx[k] = nd->l_max[k]; rmn[k] = nd->r_min[k]; rmx[k] = nd->r_max[k]; }
                    const uint32_t li = nd->l, ri = nd->r;
                    T ld, rd, t1;
                    const bool lh = slab_hit<T>(ray.o, ray.inv, lmn, lmx, ld, t1);   // slice is Some ⇔ hit; entry = max(tmin, 0)
                    const bool rh = slab_hit<T>(ray.o, ray.inv, rmn, rmx, rd, t1);
                    if (!lh && !rh) has_node = false;
                    else if (lh && !rh) node_index = li;
                    else if (!lh && rh) node_index = ri;
                    else if ((ld > rd) != !ASCENDING) { node_index = ri; entry = li; }   // right first, left rests (:126-131)
                    else { node_index = li; entry = ri; }
                }
                if (sp >= ORD_STACK) { ovf = true; has_node = false; sp = 0; }
                else { s_stack[sp][threadIdx.x] = entry; sp++; }
            } else {          // stack_pop (:215-229)
                sp--;
                const uint32_t entry = s_stack[sp][threadIdx.x];
                if (entry == ORD_NOTHING) {
                    has_node = false;
                } else if (entry & ORD_YIELD) {
                    shape = entry & ~ORD_YIELD;
                    rec = true;
                } else {
                    node_index = entry;   // move_rest (:152-176)
                    has_node = true;
                }
            }
        }
        report<T, MODE>(rec, shape, (T)0, (T)0, ray, w, pc, lane, lt);
    }
    if (ovf) atomicOr(overflow, 1u);
    if (active) ray.retire(w);
    walk_epilogue<T, MODE>(w, pc, lane, false, 0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// Best-first traversal: Bvh::nearest_traverse_iterator / farthest_traverse_iterator (bvh_impl.rs:145-176) =
// DistanceTraverseIterator<ASCENDING> (bvh/distance_traverse.rs:40-158) collected per ray.  A max-heap of
// (dist, node) drives the walk: pop the leader; a leaf yields its shape (:151-155); an inner node tests its left,
// then its right child box with intersection_slice_for_aabb and pushes every hit child with dist = -entry
// (ascending) or exit (descending) (:99-131).  The heap is Rust's std BinaryHeap and equal distances come out
// in whatever order ITS sifts leave, so the same sifts run here: push = append + sift_up, pop = move the last
// element to the root, walk the hole down along the greater child (the right one when left <= right) to the
// bottom, then sift_up (alloc::collections::binary_heap, sift_down_to_bottom).
// One ray per lane at a time, workgroups stride over the batch.  A lane's heap: entries [0, HEAP_LDS) in LDS
// (entry-major: conflict-free), the rest in a global workspace (entry-major over all resident lanes: coalesced
// when lanes touch the same entry).  The frontier of a best-first walk is small (peak 10 on the 120k-triangle
// scene, 15 on the atrium stand-in), so the global part is touched only by unusual rays; if even that
// overflows the host doubles it and replays.
// ------------------------------------------------------------------------------------------------
constexpr int HEAP_LDS = 16;

template <typename T> struct LaneHeap {
    T (*sd)[256];
    uint32_t (*sn)[256];
    T* gd;
    uint32_t* gn;
    size_t G, g;
    uint32_t tid;
    __device__ __forceinline__ T dist(uint32_t e) const { return e < HEAP_LDS ? sd[e][tid] : gd[(size_t)(e - HEAP_LDS) * G + g]; }
    __device__ __forceinline__ uint32_t node(uint32_t e) const { return e < HEAP_LDS ? sn[e][tid] : gn[(size_t)(e - HEAP_LDS) * G + g]; }
    __device__ __forceinline__ void put(uint32_t e, T d, uint32_t n) {
        if (e < HEAP_LDS) { sd[e][tid] = d; sn[e][tid] = n; }
        else { gd[(size_t)(e - HEAP_LDS) * G + g] = d; gn[(size_t)(e - HEAP_LDS) * G + g] = n; }
    }
    // BinaryHeap::sift_up(0, pos) with the element held in registers (the std's Hole)
    __device__ __forceinline__ void sift_up(uint32_t pos, T d, uint32_t n) {
        while (pos > 0) {
            const uint32_t parent = (pos - 1) >> 1;
            const T pd = dist(parent);
            if (d <= pd) break;
            put(pos, pd, node(parent));
            pos = parent;
        }
        put(pos, d, n);
    }
};

template <typename T, int MODE, bool ASCENDING>
__global__ __launch_bounds__(256) void k_traverse_heap(const typename Traits<T>::Node* __restrict__ nodes, uint32_t n_nodes,
                                                       const T* __restrict__ shape_aabbs,
                                                       const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays,
                                                       WalkOut<T> w, T* __restrict__ heap_dist, uint32_t* __restrict__ heap_node,
                                                       uint32_t heap_cap, uint32_t* __restrict__ overflow) {
    __shared__ T s_dist[HEAP_LDS][256];
    __shared__ uint32_t s_node[HEAP_LDS][256];
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    LaneHeap<T> hp;
    hp.sd = s_dist; hp.sn = s_node; hp.gd = heap_dist; hp.gn = heap_node;
    hp.G = (size_t)gridDim.x * 256; hp.g = (size_t)blockIdx.x * 256 + threadIdx.x; hp.tid = threadIdx.x;
    const uint32_t cap = HEAP_LDS + heap_cap;
    PoolCursor pc;
    bool ovf = false;
    LaneRay<T, MODE> ray;
    for (size_t base = (size_t)blockIdx.x * 256; base < n_rays; base += hp.G) {   // workgroup-uniform
        const size_t r = base + threadIdx.x;
        const bool active = r < n_rays;
        ray.clear();
        if (active) ray.load(rays, (uint32_t)r);
        uint32_t len = 0;
        if (active && n_nodes) {   // iter_initially_has_node (iter.rs:164-182), then add_to_heap(T::zero(), 0) (:75-78)
            bool has_node = true;
            const uint32_t rs = nodes[0].shape;
            if (rs != NONE) {
                const T* sb = shape_aabbs + 6 * (size_t)rs;
                const T mn[3] = {sb[0], sb[1], sb[2]}, mx[3] = {sb[3], sb[4], sb[5]};
                T t0, t1;
                has_node = slab_hit<T>(ray.o, ray.inv, mn, mx, t0, t1);
            }
            if (has_node) { hp.put(0, ASCENDING ? -(T)0 : (T)0, 0u); len = 1; }
        }
        while (true) {
            const bool run = len > 0;
            if (!__any(run)) break;
            bool rec = false;
            uint32_t shape = NONE;
            if (run) {
                // BinaryHeap::pop
                len--;
                const T last_d = hp.dist(len);
                uint32_t node_index = hp.node(len);
                if (len > 0) {
                    const uint32_t last_n = node_index;
                    node_index = hp.node(0);
                    uint32_t pos = 0, child = 1;
                    while (child + 1 < len) {            // child <= end.saturating_sub(2)
                        T cd = hp.dist(child);
                        const T cr = hp.dist(child + 1);
                        if (cd <= cr) { child++; cd = cr; }
                        hp.put(pos, cd, hp.node(child));
                        pos = child;
                        child = 2 * pos + 1;
                    }
                    if (child == len - 1) { hp.put(pos, hp.dist(child), hp.node(child)); pos = child; }
                    hp.sift_up(pos, last_d, last_n);
                }
                // unpack_node (:82-97)
                const typename Traits<T>::Node* nd = nodes + node_index;
                const uint32_t ns = nd->shape;
                if (ns != NONE) {
                    rec = true; shape = ns;
                } else {
                    T lmn[3], lmx[3], rmn[3], rmx[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) { lmn[k] = nd->l_min[k]; lmx[k] = nd->l_max[k]; rmn[k] = nd->r_min[k]; rmx[k] = nd->r_max[k]; }
                    const uint32_t li = nd->l, ri = nd->r;
                    T l0, l1, r0, r1;
                    const bool lh = slab_hit<T>(ray.o, ray.inv, lmn, lmx, l0, l1);   // slice is Some ⇔ hit: (max(tmin,0), tmax)
                    const bool rh = slab_hit<T>(ray.o, ray.inv, rmn, rmx, r0, r1);
                    if (len + (lh ? 1u : 0u) + (rh ? 1u : 0u) > cap) {
                        ovf = true; len = 0;             // the host grows the workspace and replays the batch
                    } else {
                        if (lh) { hp.sift_up(len, ASCENDING ? -l0 : l1, li); len++; }   // BinaryHeap::push
                        if (rh) { hp.sift_up(len, ASCENDING ? -r0 : r1, ri); len++; }
                    }
                }
            }
            report<T, MODE>(rec, shape, (T)0, (T)0, ray, w, pc, lane, lt);
        }
        if (active) ray.retire(w);
    }
    if (ovf) atomicOr(overflow, HEAP_OVERFLOW_BIT);
    walk_epilogue<T, MODE>(w, pc, lane, false, 0, 0, 0, 0);
}

template <typename T, int MODE, bool ASCENDING>
static void launch_ordered_as(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, bool best_first,
                              uint32_t* ovf_flag) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    char name[128];
    std::snprintf(name, sizeof name, "bvhgpu::%s<%s, %d, %s>", best_first ? "k_traverse_heap" : "k_traverse_ordered", walk_type_name<T>(), MODE,
                  ASCENDING ? "true" : "false");
    if (best_first) {   // DistanceTraverseIterator
        const unsigned heap_grid = (unsigned)std::min<size_t>((n_rays + 255) / 256, (size_t)ctx->n_cu * 4);
        const size_t lanes = (size_t)heap_grid * 256;
        if (lanes * h->heap_cap * (sizeof(T) + 4) > ((size_t)16 << 30))
            throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::OrderedDepth};
        h->heap_dist.reserve(lanes * h->heap_cap * sizeof(T));
        h->heap_node.reserve(lanes * h->heap_cap * 4);
        hipLaunchKernelGGL((k_traverse_heap<T, MODE, ASCENDING>), dim3(heap_grid), dim3(256), 0, st,
                           t->nodes.as<typename Traits<T>::Node>(), (uint32_t)t->n_nodes, t->aabbs.as<T>(), rays_dev,
                           (uint32_t)n_rays, w, h->heap_dist.as<T>(), h->heap_node.as<uint32_t>(), h->heap_cap, ovf_flag);
    } else {
        hipLaunchKernelGGL((k_traverse_ordered<T, MODE, ASCENDING>), dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st,
                           t->nodes.as<typename Traits<T>::Node>(), (uint32_t)t->n_nodes, t->aabbs.as<T>(), rays_dev,
                           (uint32_t)n_rays, w, ovf_flag);
    }
    h->walk_kernel = name;
}

template <typename T>
void launch_ordered(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, bool ascending,
                    bool best_first, uint32_t* ovf_flag) {
#define ORDERED(M) do { if (ascending) launch_ordered_as<T, M, true>(t, rays_dev, n_rays, w, h, best_first, ovf_flag); \
                        else launch_ordered_as<T, M, false>(t, rays_dev, n_rays, w, h, best_first, ovf_flag); } while (0)
    switch (mode) {
        case MODE_INDICES: ORDERED(MODE_INDICES); break;
        case MODE_TRIANGLES: ORDERED(MODE_TRIANGLES); break;
        default: ORDERED(MODE_CLOSEST); break;
    }
#undef ORDERED
}
template void launch_ordered<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, size_t, const WalkOut<float>&, bvhgpu_hits*, int, bool, bool, uint32_t*);
template void launch_ordered<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, size_t, const WalkOut<double>&, bvhgpu_hits*, int, bool, bool, uint32_t*);

}  // namespace bvhgpu
