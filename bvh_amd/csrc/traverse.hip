// traverse.hip — one batch of rays (or queries) against a tree: <FlatBvh as BoundingHierarchy>::traverse (src/flat_bvh.rs:396-431) and the
// triangle stage that follows it in the reference's harness (Ray::intersects_triangle, src/ray/ray_impl.rs:154-213; loop
// src/testbase.rs:826-836).  traverse_enqueue decides the walk and hands the batch to the file that owns it — walk_wide.hip (the default
// for large incoherent batches), walk_binary.hip, walk_ordered.hip, query.hip — then turns what the walk left into the batch's output:
// Variable-length output (Vec<&Shape> per ray) becomes CSR in three steps:
//   1. walk: every reported shape is appended to a pool as (ray, k, shape) with k = the ray's running
//      hit count (per-wave chunks of the pool, 64 records doubling to 8192: one global atomic per chunk);
//      counts[ray] = k_end;
//   2. exclusive scan of counts → offsets;
//   3. indices[offsets[ray] + k] = shape  (+ per-hit values: t-slice or triangle Intersection)     (2. and 3.: csr.hip)
// If the pool was too small the totals are still exact; the host grows it and replays (traverse_check).
// Closest-hit and any-hit batches have no CSR: one Intersection + shape per ray, resolved by the kernels below where rays were cut into items.
#include "walk.hpp"

namespace bvhgpu {

// Closest hit of rays that were walked as items (WalkOut::closest_key): the winner's shape comes out of the key, its Intersection is computed
// again from the ray and the triangle — the same function on the same operands as in the walk, hence the same bits (ray_impl.rs:154-213) —
// and the key goes back to all-ones for the next batch.  Rays no item of which met a triangle get {+inf, 0, 0} / NONE (testbase.rs:826-836:
// nothing intersected).
template <typename T>
__global__ __launch_bounds__(256) void k_closest_resolve(unsigned long long* __restrict__ key, const typename Traits<T>::Ray* __restrict__ rays,
                                                         const T* __restrict__ tris, uint32_t n_rays, T* __restrict__ closest, uint32_t* __restrict__ closest_prim) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const unsigned long long k = key[r];
    T out[3] = {Traits<T>::inf(), 0, 0};
    uint32_t prim = NONE;
    if (k != ~0ull) {
        prim = (uint32_t)(k & 0x0FFFFFFFull);
        const typename Traits<T>::Ray* rp = rays + r;
        const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
        ray_triangle<T>(o, d, tris + 9 * (size_t)prim, out);
        key[r] = ~0ull;
    }
    closest[3 * (size_t)r] = out[0]; closest[3 * (size_t)r + 1] = out[1]; closest[3 * (size_t)r + 2] = out[2];
    closest_prim[r] = prim;
}

// closest hit of a ray whose items filed their candidates under (ray, item) (f64): the minimum over the ray's items in item order — items are
// the tree-level-4 subtrees in pre-order, so a later item replaces an earlier one only on a strictly smaller distance, as the reference's
// loop does over its candidate list (testbase.rs:831-833 behind flat_bvh.rs:408).  Leaves the item set all-zero for the next batch.
template <typename T>
__global__ __launch_bounds__(256) void k_closest_resolve_slots(uint32_t* __restrict__ ray_items, const uint32_t* __restrict__ item_prim,
                                                               const typename Traits<T>::Ray* __restrict__ rays, const T* __restrict__ tris, uint32_t n_rays,
                                                               T* __restrict__ closest, uint32_t* __restrict__ closest_prim) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    uint32_t m = ray_items[r];
    T best[3] = {Traits<T>::inf(), 0, 0};
    uint32_t prim = NONE;
    if (m) {
        ray_items[r] = 0u;
        const typename Traits<T>::Ray* rp = rays + r;
        const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
        while (m) {
            const int j = __ffs((int)m) - 1;
            m &= m - 1u;
            const uint32_t p = item_prim[((size_t)r << 4) + (uint32_t)j];
            T out[3];
            ray_triangle<T>(o, d, tris + 9 * (size_t)p, out);
            if (out[0] < best[0]) { best[0] = out[0]; best[1] = out[1]; best[2] = out[2]; prim = p; }
        }
    }
    closest[3 * (size_t)r] = best[0]; closest[3 * (size_t)r + 1] = best[1]; closest[3 * (size_t)r + 2] = best[2];
    closest_prim[r] = prim;
}

// closest-hit batch of the guide walk, whole rays: the walk left the nearest shape per ray; its Intersection, recomputed in f64
template <typename T>
__global__ __launch_bounds__(256) void k_closest_from_prim(const uint32_t* __restrict__ closest_prim, const typename Traits<T>::Ray* __restrict__ rays,
                                                           const T* __restrict__ tris, uint32_t n_rays, T* __restrict__ closest) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const uint32_t p = closest_prim[r];
    T out[3] = {Traits<T>::inf(), 0, 0};
    if (p != NONE) {
        const typename Traits<T>::Ray* rp = rays + r;
        const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
        ray_triangle<T>(o, d, tris + 9 * (size_t)p, out);
    }
    closest[3 * (size_t)r] = out[0]; closest[3 * (size_t)r + 1] = out[1]; closest[3 * (size_t)r + 2] = out[2];
}

// Any-hit batch, after its walk: KEYED (rays walked as items, WalkOut::any_key) — the winner's shape comes out of the key and its Intersection
// is computed again, the same function on the same operands as in the walk (the same bits); the key goes back to all-ones for the next batch.
// Every form: the occluded rays of each workgroup are counted into part[workgroup], and k_any_publish adds them up into the counter that
// becomes bvhgpu_hits_info's total.  (No atomics on one address: it takes only ~88 per µs on this chip — one per wave of a 1 M-ray batch made
// this kernel take 0.19 ms, one per workgroup of a 512-workgroup grid still 15 µs against k_closest_resolve's 9.)
template <typename T, bool KEYED>
__global__ __launch_bounds__(256) void k_any_resolve(uint32_t* __restrict__ key, const typename Traits<T>::Ray* __restrict__ rays,
                                                     const T* __restrict__ tris, uint32_t n_rays, T* __restrict__ isect, uint32_t* __restrict__ prim,
                                                     uint32_t* __restrict__ part) {
    __shared__ uint32_t s_cnt[256 / WAVE];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t p = NONE;
    if (r < n_rays) {
        if (KEYED) {
            const uint32_t k = key[r];
            T out[3] = {Traits<T>::inf(), 0, 0};
            if (k != NONE) {
                p = k & 0x0FFFFFFFu;
                const typename Traits<T>::Ray* rp = rays + r;
                const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
                ray_triangle<T>(o, d, tris + 9 * (size_t)p, out);
                key[r] = NONE;
            }
            isect[3 * (size_t)r] = out[0]; isect[3 * (size_t)r + 1] = out[1]; isect[3 * (size_t)r + 2] = out[2];
            prim[r] = p;
        } else {
            p = prim[r];
        }
    }
    const uint32_t m = (uint32_t)__popcll(__ballot(p != NONE));
    if (lane_id() == 0) s_cnt[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < blockDim.x / WAVE; w++) sum += s_cnt[w];
        part[blockIdx.x] = sum;
    }
}
// Box batch (MODE_BOX_CLOSEST / MODE_BOX_FIRST), after its walk: per ray {enter, exit} of the winning shape's own AABB and the shape, and the
// rays that have one counted like k_any_resolve's occluded rays (part[workgroup] → k_any_publish → bvhgpu_hits_info's total).  SRC = where
// the walk left the winner: BOX_SRC_RAY — whole rays, slice and shape are in place already; BOX_SRC_KEY32 — rays walked as items, first mode:
// the lowest item's candidate, {item << 28 | shape} (WalkOut::any_key); BOX_SRC_KEY64 — items, closest, f32: {key(enter) << 32 | item << 28 |
// shape} (WalkOut::closest_key; enter >= +0, so the key orders like the value); BOX_SRC_SLOTS — items, closest, f64: the candidates by
// (ray, item), reduced in item order with the reference's strict < (k_closest_resolve_slots).  The winner's slice is computed again from the
// ray and the box — slab_hit on the operands the walk used, hence the same bits — and keys / item sets go back to their idle values.
enum : int { BOX_SRC_RAY = 0, BOX_SRC_KEY32 = 1, BOX_SRC_KEY64 = 2, BOX_SRC_SLOTS = 3 };
template <typename T, int SRC>
__global__ __launch_bounds__(256) void k_box_resolve(uint32_t* __restrict__ key32, unsigned long long* __restrict__ key64, uint32_t* __restrict__ ray_items,
                                                     const uint32_t* __restrict__ item_prim, const typename Traits<T>::Ray* __restrict__ rays,
                                                     const T* __restrict__ aabbs, uint32_t n_rays, T* __restrict__ slice, uint32_t* __restrict__ prim,
                                                     uint32_t* __restrict__ part) {
    __shared__ uint32_t s_cnt[256 / WAVE];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t p = NONE;
    if (r < n_rays) {
        if (SRC == BOX_SRC_RAY) {
            p = prim[r];
        } else {
            T best[2] = {Traits<T>::inf(), 0};
            const typename Traits<T>::Ray* rp = rays + r;
            const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, inv[3] = {rp->inv[0], rp->inv[1], rp->inv[2]};
            auto slice_of = [&](uint32_t shape, T& t0, T& t1) {
                const T* b = aabbs + 6 * (size_t)shape;
                const T mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
                slab_hit<T>(o, inv, mn, mx, t0, t1);
            };
            if (SRC == BOX_SRC_KEY32) {
                const uint32_t k = key32[r];
                if (k != NONE) { p = k & 0x0FFFFFFFu; slice_of(p, best[0], best[1]); key32[r] = NONE; }
            } else if (SRC == BOX_SRC_KEY64) {
                const unsigned long long k = key64[r];
                if (k != ~0ull) { p = (uint32_t)(k & 0x0FFFFFFFull); slice_of(p, best[0], best[1]); key64[r] = ~0ull; }
            } else {
                uint32_t m = ray_items[r];
                if (m) ray_items[r] = 0u;
                while (m) {
                    const int j = __ffs((int)m) - 1;
                    m &= m - 1u;
                    const uint32_t q = item_prim[((size_t)r << 4) + (uint32_t)j];
                    T t0, t1;
                    slice_of(q, t0, t1);
                    if (t0 < best[0]) { best[0] = t0; best[1] = t1; p = q; }
                }
            }
            slice[2 * (size_t)r] = best[0]; slice[2 * (size_t)r + 1] = best[1];
            prim[r] = p;
        }
    }
    const uint32_t m = (uint32_t)__popcll(__ballot(p != NONE));
    if (lane_id() == 0) s_cnt[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < blockDim.x / WAVE; w++) sum += s_cnt[w];
        part[blockIdx.x] = sum;
    }
}
// Sphere batch (MODE_SPHERE_CLOSEST / MODE_SPHERE_FIRST), after its walk: k_box_resolve's sibling with ray_sphere as the leaf stage (a sibling,
// not a template parameter of k_box_resolve, whose instantiations keep their names and text).  Per ray {distance, exit} of the winning
// shape's sphere and the shape; the rays that have one are counted into part[workgroup].  SRC as above (BOX_SRC_*): distance > eps > 0, so
// its bits order as unsigned integers and the walk's keys and slots are the box batches'.  Every candidate the walk filed had distance <
// tmax already; the winner's hit is computed again — ray_sphere on the operands the walk used, hence the same bits.
template <typename T, int SRC>
__global__ __launch_bounds__(256) void k_sphere_resolve(uint32_t* __restrict__ key32, unsigned long long* __restrict__ key64, uint32_t* __restrict__ ray_items,
                                                        const uint32_t* __restrict__ item_prim, const typename Traits<T>::Ray* __restrict__ rays,
                                                        const T* __restrict__ spheres, uint32_t n_rays, T* __restrict__ hit, uint32_t* __restrict__ prim,
                                                        uint32_t* __restrict__ part) {
    __shared__ uint32_t s_cnt[256 / WAVE];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t p = NONE;
    if (r < n_rays) {
        if (SRC == BOX_SRC_RAY) {
            p = prim[r];
        } else {
            T best[2] = {Traits<T>::inf(), 0};
            const typename Traits<T>::Ray* rp = rays + r;
            const T o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
            if (SRC == BOX_SRC_KEY32) {
                const uint32_t k = key32[r];
                if (k != NONE) { p = k & 0x0FFFFFFFu; ray_sphere<T>(o, d, spheres + 4 * (size_t)p, best); key32[r] = NONE; }
            } else if (SRC == BOX_SRC_KEY64) {
                const unsigned long long k = key64[r];
                if (k != ~0ull) { p = (uint32_t)(k & 0x0FFFFFFFull); ray_sphere<T>(o, d, spheres + 4 * (size_t)p, best); key64[r] = ~0ull; }
            } else {
                uint32_t m = ray_items[r];
                if (m) ray_items[r] = 0u;
                while (m) {
                    const int j = __ffs((int)m) - 1;
                    m &= m - 1u;
                    const uint32_t q = item_prim[((size_t)r << 4) + (uint32_t)j];
                    T t[2];
                    ray_sphere<T>(o, d, spheres + 4 * (size_t)q, t);
                    if (t[0] < best[0]) { best[0] = t[0]; best[1] = t[1]; p = q; }
                }
            }
            hit[2 * (size_t)r] = best[0]; hit[2 * (size_t)r + 1] = best[1];
            prim[r] = p;
        }
    }
    const uint32_t m = (uint32_t)__popcll(__ballot(p != NONE));
    if (lane_id() == 0) s_cnt[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < blockDim.x / WAVE; w++) sum += s_cnt[w];
        part[blockIdx.x] = sum;
    }
}
// k_publish_counters for an any-hit, box or sphere batch: ctr[3] = the sum of k_any_resolve's per-workgroup counts, then the 8 counters go to the pinned
// host page and are zeroed for the next call
__global__ __launch_bounds__(256) void k_any_publish(unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ host_page,
                                                     const uint32_t* __restrict__ part, uint32_t n_part) {
    __shared__ unsigned long long s_sum[256 / WAVE];
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < n_part; i += blockDim.x) sum += part[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
    if (lane_id() == 0) s_sum[threadIdx.x / WAVE] = sum;
    __syncthreads();
    if (threadIdx.x < 8) {
        unsigned long long v = ctr[threadIdx.x];
        if (threadIdx.x == 3) {
            v = 0;
            for (uint32_t w = 0; w < blockDim.x / WAVE; w++) v += s_sum[w];
        }
        host_page[threadIdx.x] = v;
        ctr[threadIdx.x] = 0;
    }
    __threadfence_system();
}

// ---- one batch = enqueue (no host round trip) + check (after the stream has been synchronised) --------------------
// What the enqueue decided is kept in the result object, so that the check — and an asynchronous caller's
// bvhgpu_hits_wait — can replay the batch when the hit pool, a lane's heap or a lane's stack was too small.
template <typename T>
void traverse_enqueue(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, unsigned flags, bvhgpu_hits* h) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const bool stats = (flags & BVHGPU_TRAVERSE_STATS) != 0;
    const bool coherent = (flags & BVHGPU_TRAVERSE_COHERENT) != 0;
    const int ordered = (flags & BVHGPU_TRAVERSE_NEAREST_FIRST) ? 1 : ((flags & BVHGPU_TRAVERSE_FARTHEST_FIRST) ? 2 : 0);
    const int mode = (flags & TRAVERSE_SPHERE_HIT) ? ((flags & BVHGPU_TRAVERSE_FIRST) ? MODE_SPHERE_FIRST : MODE_SPHERE_CLOSEST)
                   : (flags & TRAVERSE_BOX_HIT) ? ((flags & BVHGPU_TRAVERSE_FIRST) ? MODE_BOX_FIRST : MODE_BOX_CLOSEST)
                   : (flags & TRAVERSE_ANY_HIT) ? MODE_ANY
                   : (flags & BVHGPU_TRAVERSE_CLOSEST) ? MODE_CLOSEST
                   : (flags & BVHGPU_TRAVERSE_TRIANGLES) ? MODE_TRIANGLES
                   : (flags & BVHGPU_TRAVERSE_T_SLICE) ? MODE_T_SLICE : MODE_INDICES;
    const int nv = mode == MODE_T_SLICE ? 2 : (mode == MODE_TRIANGLES ? 3 : 0);
    const int variant = ctx->tune[BVHGPU_TUNE_TRAVERSE_VARIANT];
    // (the COHERENT hint does not choose the walk kernel — on 10 M primary rays the wide walk takes 1.5 ms, the persistent binary walk 2.2 ms
    //  and one ray per lane per launch 5.4 ms — it chooses how the wide walk hands over its hits: see `staged` below)
    const bool big_batch = !ordered && n_rays >= (size_t)ctx->tune[BVHGPU_TUNE_TRAVERSE_LDS_MIN_RAYS];
    // walk kernel: wide walk (see k_traverse_wide for what it needs), else persistent workgroups over the binary array with
    // its top in LDS, else one ray per lane per launch
    // (a query batch — h->pend_kind, query.hip — goes through the plain CSR path of the binary walks whichever walk launch_query picks)
    const bool query = h->pend_kind != 0;
    const bool use_wide = variant >= 3 && big_batch && t->has_wide && !t->exact_only && !t->unfolded && !stats &&
                          mode != MODE_T_SLICE && !h->force_binary && t->n >= 2 && !query;
    const bool use_lds = !use_wide && variant != 0 && t->slot_entry.p != nullptr && big_batch && !query;
    // several items per ray while a resident lane gets fewer than ~4 rays: the tail of the launch dominates there
    const bool few_rays = n_rays < (size_t)ctx->n_cu * 2048 * 4;
    uint32_t split_at = 0;
    if (use_lds && mode < MODE_CLOSEST && ctx->tune[BVHGPU_TUNE_TRAVERSE_SPLIT] != 0 && t->n >= 2 && !t->unfolded && few_rays)
        split_at = 1;   // the kernel reads the boundary itself: exit index of entry 0 (the root's left child)
    // CSR batches: 1, 4 or 16 items per ray.  Closest hit: whole rays, or the same cut into 16 items below ~2 M rays — the per-ray minimum over
    // the items goes through WalkOut::closest_key (f32: one 64-bit atomicMin per item with a candidate) or through the (ray, item) slots (f64:
    // k_closest_resolve_slots).  Any hit: the same choice, the lowest item with a candidate through WalkOut::any_key (one 32-bit atomicMin per
    // item with a candidate, f32 and f64).  Box and sphere batches: closest like closest hit, first like any hit (k_box_resolve / k_sphere_resolve)
    int items_log4 = 0;
    if (use_wide && n_rays < WIDE_ITEM_MAX_RAYS) {
        const int want = ctx->tune[BVHGPU_TUNE_WIDE_ITEMS_LOG4];
        if (mode < MODE_CLOSEST) items_log4 = want >= 0 ? std::min(want, 2) : (few_rays ? 2 : 0);
        else items_log4 = (want >= 0 ? want >= 2 : few_rays) ? 2 : 0;
    }
    // the item filter beside the build (walk_wide.hip launch_wide): the tree is being rebuilt on this stream, the build has recorded the event
    // behind the pass that splits level 3, and the caller says that the rays do not depend on anything enqueued since
    const bool early_items = use_wide && items_log4 == 2 && (flags & BVHGPU_TRAVERSE_RAYS_READY) != 0 && t->pending_build && t->ev_top != nullptr &&
                             t->ev_top_gen == t->gen && ctx->tune[BVHGPU_TUNE_WIDE_EARLY_ITEMS] != 0;
    // f64 index batches: the f32 walk over the tree's guide boxes, leaf candidates confirmed in f64 (guide_ray_load; a result object that met
    // a ray outside the guide walk's range stays with the f64 walk)
    // A result object that met a ray outside the guide walk's range backs off: the next `guide_skip` f64 index batches take the f64 walk
    // straight away (1, 2, 4 … 64 batches on consecutive failures — a workload of axis-parallel rays pays one wasted guide walk in 65),
    // then the guide is tried again; a batch that stays in range resets the back-off (the fall-back used to be for ever).
    const bool guide_ok = sizeof(T) == 8 && use_wide && (mode == MODE_INDICES || mode == MODE_CLOSEST) && t->has_guide && !early_items && ctx->tune[BVHGPU_TUNE_WIDE_F64_GUIDE] != 0;
    const bool replaying_out_of_range = h->no_guide;      // traverse_check sent this very batch back
    // (one back-off slot per BATCH: a replay of the same batch — pool / index growth, a stack overflow's switch to the binary walk — takes none)
    const bool first_enqueue = h->pend_attempts == 0 && !h->force_binary && !replaying_out_of_range;
    if (guide_ok && first_enqueue && h->guide_skip > 0) h->guide_skip--;
    const bool use_guide = guide_ok && !replaying_out_of_range && h->guide_skip == 0;
    if (replaying_out_of_range) {
        h->no_guide = false;
        h->guide_backoff = h->guide_backoff ? std::min(2 * h->guide_backoff, 64u) : 1u;
        h->guide_skip = h->guide_backoff + 1u;             // (+1: the decrement of the next batch's enqueue)
    }
    h->pend_guide = use_guide;
    const size_t n_items = split_at ? 2 * n_rays : n_rays;
    h->ctx = ctx; h->dtype = Traits<T>::dtype; h->n_rays = n_rays; h->flags = flags; h->total = 0;
    h->stats = bvhgpu_traverse_stats{0, 0, 0, 0, 0};
    h->pend_tree = t; h->pend_rays = rays_dev; h->pend_wide = use_wide; h->pend_unfolded = t->unfolded || t->n == 1;
    // two counter sets: a batch uses one and (k_scan_final) zeroes the other for the batch after it
    if (h->ctr.reserve(16 * sizeof(unsigned long long))) h->ctr_clean = false;
    if (!h->pin) BVH_HIP(hipHostMalloc(&h->pin, 64, hipHostMallocDefault));
    unsigned long long* pin = reinterpret_cast<unsigned long long*>(h->pin);
    unsigned long long* ctr = h->ctr.as<unsigned long long>() + 8 * (h->ctr_set & 1);
    unsigned long long* ctr_other = h->ctr.as<unsigned long long>() + 8 * ((h->ctr_set & 1) ^ 1);

    WalkOut<T> w{};
    const bool box = mode_box(mode), sphere = mode_sphere(mode);
    w.ctr = ctr;
    if (box) w.set_boxes(t->aabbs.as<T>());   // (box batches read no triangles: their leaf primitive is the shape's own AABB)
    else if (sphere) w.set_spheres(t->spheres.as<T>());   // (nor do sphere batches: bvhgpu_tree_set_spheres_*'s array)
    else w.tris = t->tris.as<T>();

    uint32_t* ovf_flag = reinterpret_cast<uint32_t*>(ctr + 7);   // bit 0 ordered-iterator stack, bit 1 heap workspace, bit 2 wide-walk stack
    const bool best_first = ordered && (flags & BVHGPU_TRAVERSE_BEST_FIRST) != 0;
    // the batch's walk, by the file that owns it (each writes h->walk_kernel), between the walk's two timing events
    auto walk = [&] {
        if (ctx->timing) BVH_HIP(hipEventRecord(ctx->ev[4], st));
        if (query) launch_query<T>(t, n_rays, w, h, ovf_flag);
        else if (ordered) launch_ordered<T>(t, rays_dev, n_rays, w, h, mode, ordered == 1, best_first, ovf_flag);
        else if (use_wide) launch_wide_walk<T>(t, rays_dev, n_rays, w, h, mode, items_log4, use_guide, early_items, ovf_flag);
        else launch_binary<T>(t, rays_dev, n_rays, w, h, mode, stats, use_lds, split_at);
        if (ctx->timing) BVH_HIP(hipEventRecord(ctx->ev[5], st));
    };

    if (!h->ctr_clean) BVH_HIP(hipMemsetAsync(ctr, 0, 8 * sizeof(unsigned long long), st));   // (only this batch's set has to be clean)
    h->ctr_clean = false;
    if (mode >= MODE_CLOSEST) {   // no CSR: one Intersection (box: one t-slice) + shape per ray (closest / closest_prim); any hit and box: the rays with an answer counted in ctr[3]
        const bool any = mode_first(mode);   // (the first candidate ends the ray: the keys of any hit)
        h->closest.reserve(std::max<size_t>(n_rays, 1) * 3 * sizeof(T));
        h->closest_prim.reserve(std::max<size_t>(n_rays, 1) * 4);
        if (n_rays == 0) { h->pend_tree = nullptr; return; }
        w.closest = h->closest.as<T>(); w.closest_prim = h->closest_prim.as<uint32_t>();
        if (mode_tmax(mode)) w.tmax = static_cast<const T*>(h->pend_tmax);
        const bool by_items = use_wide && items_log4 == 2;
        const bool keyed = by_items && (any || sizeof(T) == 4);
        if (keyed) {   // the per-ray keys (u32 any hit, u64 closest hit): all-ones between batches (the resolve kernel puts them back)
            DevBuf& key = any ? h->any_key : h->closest_key;
            bool& clean = any ? h->akey_clean : h->ckey_clean;
            if (key.reserve(n_rays * (any ? sizeof(uint32_t) : sizeof(unsigned long long)))) clean = false;
            if (!clean) BVH_HIP(hipMemsetAsync(key.p, 0xFF, key.cap, st));
            clean = true;
            if (any) w.any_key = key.as<uint32_t>(); else w.closest_key = key.as<unsigned long long>();
        } else if (by_items) {   // f64 closest hit: candidates by (ray, item), the rays' item sets all-zero between batches (k_closest_resolve_slots puts the zeros back)
            h->item_cnt.reserve(((n_rays << 4) + 1) * 4);
            if (h->ray_items.reserve((n_rays + 1) * 4)) BVH_HIP(hipMemsetAsync(h->ray_items.p, 0, h->ray_items.cap, st));
            w.item_cnt = h->item_cnt.as<uint32_t>();
            w.ray_items = h->ray_items.as<uint32_t>();
        }
        walk();
        const dim3 rgrid((unsigned)((n_rays + 255) / 256)), rblock(256);
        const T* tris = t->tris.as<T>();
        const uint32_t nr = (uint32_t)n_rays;
        if (box) {
            h->any_part.reserve((size_t)rgrid.x * 4);
            uint32_t* part = h->any_part.as<uint32_t>();
            const T* boxes = t->aabbs.as<T>();
#define BOX_RESOLVE(SRC) hipLaunchKernelGGL((k_box_resolve<T, SRC>), rgrid, rblock, 0, st, w.any_key, w.closest_key, w.ray_items, (const uint32_t*)w.item_cnt, \
                                            rays_dev, boxes, nr, w.closest, w.closest_prim, part)
            if (!by_items) BOX_RESOLVE(BOX_SRC_RAY);
            else if (any) BOX_RESOLVE(BOX_SRC_KEY32);
            else if (keyed) BOX_RESOLVE(BOX_SRC_KEY64);
            else BOX_RESOLVE(BOX_SRC_SLOTS);
#undef BOX_RESOLVE
        } else if (sphere) {
            h->any_part.reserve((size_t)rgrid.x * 4);
            uint32_t* part = h->any_part.as<uint32_t>();
            const T* spheres = t->spheres.as<T>();
#define SPHERE_RESOLVE(SRC) hipLaunchKernelGGL((k_sphere_resolve<T, SRC>), rgrid, rblock, 0, st, w.any_key, w.closest_key, w.ray_items, (const uint32_t*)w.item_cnt, \
                                               rays_dev, spheres, nr, w.closest, w.closest_prim, part)
            if (!by_items) SPHERE_RESOLVE(BOX_SRC_RAY);
            else if (any) SPHERE_RESOLVE(BOX_SRC_KEY32);
            else if (keyed) SPHERE_RESOLVE(BOX_SRC_KEY64);
            else SPHERE_RESOLVE(BOX_SRC_SLOTS);
#undef SPHERE_RESOLVE
        } else if (any) {
            h->any_part.reserve((size_t)rgrid.x * 4);
            if (by_items) hipLaunchKernelGGL((k_any_resolve<T, true>), rgrid, rblock, 0, st, w.any_key, rays_dev, tris, nr, w.closest, w.closest_prim, h->any_part.as<uint32_t>());
            else hipLaunchKernelGGL((k_any_resolve<T, false>), rgrid, rblock, 0, st, nullptr, rays_dev, tris, nr, w.closest, w.closest_prim, h->any_part.as<uint32_t>());
        } else if (keyed) {
            hipLaunchKernelGGL(k_closest_resolve<T>, rgrid, rblock, 0, st, w.closest_key, rays_dev, tris, nr, w.closest, w.closest_prim);
        } else if (by_items) {
            hipLaunchKernelGGL(k_closest_resolve_slots<T>, rgrid, rblock, 0, st, w.ray_items, (const uint32_t*)w.item_cnt, rays_dev, tris, nr, w.closest, w.closest_prim);
        } else if (use_guide) {   // whole rays of the guide walk: the shapes are in closest_prim, their Intersections follow
            hipLaunchKernelGGL(k_closest_from_prim<T>, rgrid, rblock, 0, st, (const uint32_t*)w.closest_prim, rays_dev, tris, nr, w.closest);
        }
        if (ctx->timing) BVH_HIP(hipEventRecord(ctx->ev[6], st));
        // readback + reset for the next call
        if (any || box || sphere) hipLaunchKernelGGL(k_any_publish, dim3(1), dim3(256), 0, st, ctr, pin, (const uint32_t*)h->any_part.as<uint32_t>(), rgrid.x);
        else publish_counters(st, ctr, pin);
        h->ctr_clean = true;
        join_flat(t);
        return;
    }

    h->offsets.reserve((n_rays + 1) * 4);
    const uint32_t nb = (uint32_t)((n_rays + SCAN_BLOCK - 1) / SCAN_BLOCK);
    if (h->blocksums.reserve((nb + 1) * sizeof(unsigned long long))) h->bs_clean = false;
    if (h->pool_cap == 0) {
        h->pool_cap = std::max<size_t>(n_rays, (size_t)1 << 16);
        // pair records take 16 bytes whether they hold one hit or two: a first pool sized in 12-byte slots would hold 0.75 records per ray and
        // a batch of single-hit rays would overflow it where the 12-byte records fitted — size it so that every ray has a record
        if (use_wide && items_log4 == 0 && mode == MODE_INDICES && ctx->tune[BVHGPU_TUNE_WIDE_REC8] != 0) h->pool_cap = (h->pool_cap * 16 + sizeof(HitRec) - 1) / sizeof(HitRec);
    }
    if (n_rays == 0) {
        BVH_HIP(hipMemsetAsync(h->offsets.p, 0, 4, st));
        h->pend_tree = nullptr;
        return;
    }
    // staged output (WalkOut::raybuf): whole rays, indices only — the hit-heavy large batches; stage_shift 3 = eight shapes per ray
    // Default: for batches the caller calls COHERENT (primary rays).  Measured on the stand-in scene: 10 M coherent rays 2.60 → 2.17 ms per
    // step (the walk itself 1.79 → 1.54: no chunk atomics, a third of the bytes; neighbouring rays' slots are written close in time and
    // merge in L2); 12.5 M incoherent rays 3.30 → 3.23; 100 M incoherent rays 21.1 → 22.0 (the walk 16.3 → 18.4: every hit of a
    // wave lands on a line of its own) — so incoherent batches keep the pool, whose records a wave writes contiguously.
    const int stage_knob = ctx->tune[BVHGPU_TUNE_WIDE_STAGE_SHIFT];
    const int stage_shift = stage_knob < 0 ? (coherent ? 3 : 0) : std::min(stage_knob, 5);
    const bool staged = use_wide && items_log4 == 0 && mode == MODE_INDICES && stage_shift >= 2;
    h->pend_staged = staged;
    if (h->idx_cap < h->pool_cap) h->idx_cap = h->pool_cap;
    h->pool.reserve(h->pool_cap * sizeof(HitRec));
    h->indices.reserve(h->idx_cap * 4);
    if (staged) { h->raybuf.reserve(((size_t)n_rays << stage_shift) * 4 + 64); w.raybuf = h->raybuf.as<uint32_t>(); w.stage_shift = (uint32_t)stage_shift; }
    // pair records (8 bytes per hit) for whole-ray index batches
    const bool rec8 = use_wide && items_log4 == 0 && mode == MODE_INDICES && ctx->tune[BVHGPU_TUNE_WIDE_REC8] != 0;
    h->pend_rec8 = rec8;
    if (nv) {
        h->pool_t.reserve(h->pool_cap * nv * sizeof(T));
        (mode == MODE_T_SLICE ? h->tslice : h->isect).reserve(h->pool_cap * nv * sizeof(T));
    }
    // (the pool's bytes then hold 16-byte pair records: three for every four HitRec slots)
    const unsigned long long cap = rec8 ? (unsigned long long)h->pool_cap * sizeof(HitRec) / 16u : h->pool_cap;
    uint32_t* counts;
    uint32_t* bsum_other = nullptr;
    if (use_wide) {   // per-ray words kept all-zero between batches (k_scan_final puts the zeros back)
        if (h->wcounts.reserve((n_rays + 1) * 4)) h->wcounts_clean = false;
        if (!h->wcounts_clean) BVH_HIP(hipMemsetAsync(h->wcounts.p, 0, h->wcounts.cap, st));
        h->wcounts_clean = false;
        if (items_log4) {
            h->ray_mask.reserve((n_rays + 1) * 2);
            h->item_cnt.reserve(((n_rays << (2 * items_log4)) + 1) * 4);
            if (h->ray_items.reserve((n_rays + 1) * 4)) BVH_HIP(hipMemsetAsync(h->ray_items.p, 0, h->ray_items.cap, st));   // then kept zero like wcounts
            w.item_cnt = h->item_cnt.as<uint32_t>();
            w.ray_items = h->ray_items.as<uint32_t>();
        }
        counts = h->wcounts.as<uint32_t>();
        // the walk's workgroups leave the hits per 64-ray block (their own blocks: LDS sums): no reduce pass for the scan
        const size_t grid = wide_walk_grid<T>(ctx, n_rays, items_log4, coherent, use_guide);
        const size_t n_blocks = (n_rays + 63) / 64;
        if (nb <= SCAN_FUSED_MAX_BLOCKS && (n_blocks + grid - 1) / grid <= WIDE_BSUM_MAX) {
            // two sets of SCAN_FUSED_MAX_BLOCKS sums, used alternately like the counter sets (k_scan_final zeroes the other one)
            if (h->scan_sums.reserve(2 * SCAN_FUSED_MAX_BLOCKS * 4)) BVH_HIP(hipMemsetAsync(h->scan_sums.p, 0, h->scan_sums.cap, st));
            w.scan_sums = h->scan_sums.as<uint32_t>() + (size_t)SCAN_FUSED_MAX_BLOCKS * (h->bsum_set & 1);
            bsum_other = h->scan_sums.as<uint32_t>() + (size_t)SCAN_FUSED_MAX_BLOCKS * ((h->bsum_set & 1) ^ 1);
            h->bsum_set ^= 1;   // (this batch's k_scan_final zeroes the other set: the next batch's)
        }
    } else {
        h->counts.reserve((n_items + 1) * 4);
        counts = h->counts.as<uint32_t>();
    }
    w.counts = counts; w.pool = h->pool.as<HitRec>(); w.pool_v = h->pool_t.as<T>(); w.pool_cap = cap;
    w.pool_pair = rec8 ? h->pool.as<uint4>() : nullptr;
    walk();
    CsrArgs csr;
    csr.count_kind = use_wide ? COUNT_MASKED : (split_at ? COUNT_PAIR : COUNT_PLAIN);
    csr.nv = nv; csr.items_log4 = items_log4; csr.stage_shift = staged ? stage_shift : 0; csr.rec8 = rec8;
    csr.nb = nb; csr.cap = cap; csr.ctr_other = ctr_other; csr.pin = pin; csr.bsum_other = bsum_other;
    csr_enqueue<T>(h, n_rays, w, csr);
    if (use_wide) h->wcounts_clean = true;   // (stays true only if the check finds that the batch ran to completion)
    if (ctx->timing) { BVH_HIP(hipEventRecord(ctx->ev[6], st)); }
    if (nb > SCAN_FUSED_MAX_BLOCKS) {   // readback + reset for the next call (smaller batches: k_scan_final's last block did both)
        publish_counters(st, ctr, pin);
    } else {
        h->ctr_set ^= 1;   // the set that was just zeroed
    }
    h->ctr_clean = true;
    join_flat(t);   // (BVHGPU_TUNE_FLATTEN_LAZY = 2: the flatten part that ran beside this walk — the batch's wait covers it)
}

// After the stream has been synchronised: true = the batch is complete; false = something was too small and has been
// grown (or the walk switched) — enqueue again.  Throws on the conditions the reference would panic on.
bool traverse_check(bvhgpu_hits* h) {
    if (!h->pend_tree) return true;   // nothing was launched (empty batch)
    bvhgpu_ctx* ctx = h->ctx;
    const unsigned flags = h->flags;
    const bool stats = (flags & BVHGPU_TRAVERSE_STATS) != 0;
    const bool ordered = (flags & (BVHGPU_TRAVERSE_NEAREST_FIRST | BVHGPU_TRAVERSE_FARTHEST_FIRST)) != 0;
    const bool best_first = ordered && (flags & BVHGPU_TRAVERSE_BEST_FIRST) != 0;
    const unsigned long long* pin = reinterpret_cast<const unsigned long long*>(h->pin);
    BVH_HIP(hipGetLastError());
    if (best_first && (pin[7] & HEAP_OVERFLOW_BIT)) {   // a lane's heap outgrew the workspace
        if (++h->pend_attempts > 24) throw HipFail{hipErrorUnknown, "best-first heap did not converge", __LINE__};
        h->heap_cap *= 2; return false;
    }
    if (ordered && (pin[7] & 1ull)) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::OrderedDepth};
    if (h->pend_guide && (pin[7] & WALK_FLAG_GUIDE_RANGE)) {   // a ray outside the guide walk's range: this result object goes back to the f64 walk
        h->no_guide = true; h->wcounts_clean = false; return false;   // (the replay of this batch walks in f64; traverse_enqueue sets the back-off)
    }
    if (h->pend_qwide && (pin[7] & 4ull)) {   // a lane of the wide query walk outgrew its LDS stack: replay with the binary walk
        h->force_binary = true; return false;
    }
    if (h->pend_wide && (pin[7] & 4ull)) {   // a lane's stack outgrew LDS + workspace: the binary walks need no stack
        h->force_binary = true; h->wcounts_clean = false; h->bs_clean = false; h->ckey_clean = false; h->akey_clean = false; h->ray_items.release(); return false;
    }
    if (flags & (TRAVERSE_ANY_HIT | TRAVERSE_BOX_HIT | TRAVERSE_SPHERE_HIT)) {   // the occluded rays (box, sphere: the rays with a candidate), counted by k_any_resolve / k_box_resolve / k_sphere_resolve and k_any_publish
        h->total = pin[3];
        if (ctx->timing) ctx->ev_set |= 4u;
        h->pend_tree = nullptr;
        return true;
    }
    if (flags & BVHGPU_TRAVERSE_CLOSEST) {
        if (stats) {
            h->stats.hits = pin[5];
            h->stats.device_steps = pin[1];
            h->stats.wave_steps = pin[4];
            h->stats.visited = h->pend_unfolded ? pin[1] : pin[1] + pin[5];
            h->stats.leaf_visits = h->pend_unfolded ? pin[2] : pin[5];
        }
        if (ctx->timing) ctx->ev_set |= 4u;
        h->pend_tree = nullptr;
        return true;
    }
    const unsigned long long used = pin[0];   // pool slots taken (whole chunks)
    const unsigned long long total = pin[3];  // sum of the per-ray counts = number of hits
    const bool pair_recs = h->pend_rec8;   // `used` counts 16-byte records of two hits, pool_cap 12-byte slots
    if ((pair_recs ? 2 * used : used) < total && !h->pend_staged) throw HipFail{hipErrorUnknown, "hit pool / count scan mismatch", __LINE__};
    if (total > 0xFFFFFFFFull) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::Overflow};
    // Pool or index array too small: grow to the need and replay — both in ONE replay (the count scan is complete even when records were
    // dropped, and pair records need fewer pool slots than there are hits, so the pool no longer sizes the index array).
    const bool pool_small = used > (pair_recs ? (unsigned long long)h->pool_cap * sizeof(HitRec) / 16u : (unsigned long long)h->pool_cap);
    const bool idx_small = total > h->idx_cap;
    if (pool_small || idx_small) {
        if (++h->pend_attempts > 3) throw HipFail{hipErrorUnknown, pool_small ? "hit pool did not converge" : "index array did not converge", __LINE__};
        if (pool_small) {
            const size_t need = pair_recs ? ((size_t)used * 16u + sizeof(HitRec) - 1) / sizeof(HitRec) : (size_t)used;
            h->pool_cap = need + need / 8 + 1024;
        }
        if (idx_small) h->idx_cap = (size_t)total + (size_t)total / 8 + 1024;
        return false;
    }
    if (h->pend_guide) h->guide_backoff = 0;   // an f64 batch that stayed inside the guide walk's range
    h->total = total;
    h->stats.hits = total;
    if (stats) {
        h->stats.device_steps = pin[1];
        h->stats.wave_steps = pin[4];
        // reference-equivalent loop iterations (flat_bvh.rs:408): in the folded layout every
        // reported leaf stands for a navigator visit plus a leaf-entry visit
        h->stats.visited = h->pend_unfolded ? pin[1] : pin[1] + total;
        h->stats.leaf_visits = h->pend_unfolded ? pin[2] : total;
    }
    if (ctx->timing) ctx->ev_set |= 4u;
    h->pend_tree = nullptr;
    return true;
}

template <typename T>
void traverse_batch(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, unsigned flags,
                    bvhgpu_hits* h) {
    h->force_binary = false; h->pend_attempts = 0;
    for (;;) {
        traverse_enqueue<T>(t, rays_dev, n_rays, flags, h);
        BVH_HIP(hipStreamSynchronize(t->ctx->stream));
        if (traverse_check(h)) return;
    }
}

template void traverse_enqueue<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, size_t, unsigned, bvhgpu_hits*);
template void traverse_enqueue<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, size_t, unsigned, bvhgpu_hits*);
template void traverse_batch<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, size_t, unsigned, bvhgpu_hits*);
template void traverse_batch<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, size_t, unsigned, bvhgpu_hits*);

}  // namespace bvhgpu
