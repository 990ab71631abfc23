// walk_wide.hip — the 4-wide walk (k_traverse_wide: four grandchild boxes per step, rays cut into items, the f32 guide walk of f64
// batches) with its item filter (k_wide_items) and workgroup geometry.  launch_wide_walk picks the instantiation for traverse_enqueue
// (traverse.hip); wide_walk_grid tells it how many workgroups that launch will have.
#include <cstdio>

#include "walk.hpp"

namespace bvhgpu {

// ------------------------------------------------------------------------------------------------
// Wide walk (large incoherent batches, the default): four grandchild boxes per step instead of one child box.
//
// Why it returns the reference's list.  FlatBvh::traverse reports shape s iff the slab test passes for every
// ancestor box of s and for s's own AABB (flat_bvh.rs:408-427), in pre-order.  Every ancestor box is the exact join
// (component-wise min / max, no rounding) of the AABBs below it, so it contains s's AABB component by component.
// For a ray whose origin is finite and whose inverse direction is finite and nonzero (common.hpp ray_is_finite), against
// finite boxes, no product (b - o) * inv is NaN (b - o may round to ±inf; only inf * 0 would be NaN) and each is
// monotone in b (IEEE subtraction and multiplication by a constant are monotone under round-to-nearest):
// growing a box can only lower its entry parameter and raise its exit parameter, so
//        slab(ray, AABB(s)) passes  ⇒  slab(ray, every ancestor box of s) passes.
// The ancestor tests are therefore redundant for the RESULT, and a walk may skip tree levels as long as it keeps the
// pre-order: this kernel visits, for an inner node b, the four grandchildren directly (common.hpp WideNode).  On the
// 120k-triangle scene a ray needs 20 dependent steps instead of 79, for the same 79 box tests.  Rays with a non-finite
// component (axis-parallel: inv = ±inf) or a zero inv component (caller-built rays) can produce NaN products, which the
// reference turns into a miss
// (intersect_default.rs:22-28) and which break the implication above; waves holding such a ray take the exact
// sequence instead: the skipped child box is rebuilt as the join of its two grandchild boxes (bit-identical to
// the builder's box up to the sign of a zero, which no product distinguishes) and tested with the reference's
// NaN-aware slab test before its grandchildren are.  Trees where a child box is NOT the join of its grandchildren
// (empty bounds after a split with no SAH winner, bvh_node.rs:225-230; uploaded FlatBvh whose shapes moved) and the
// outputs that need the reference's own visit sequence (STATS, T_SLICE) use the binary walks (walk_binary.hip).
//
// Per lane: `cur` = what to do next (an inner node, a leaf to report, or nothing) and a stack of the other hit
// grandchildren (at most 3 pushes per step; the first `stack_lds` entries per lane in LDS, entry-major, the rest in
// a global workspace; overflowing that raises a flag and the host replays the batch with the binary walk).
// The nodes with the K lowest 4-ary heap numbers (root 0, children 4q+1..4q+4) are copied to LDS by every workgroup
// (one 16-byte plane per chunk, like walk_binary.hip's TopLds), a lane follows heap numbers while it is inside that set.
// A ray may be cut into 4 ITEMS, one per grandchild of the root (no ancestor test is owed, see above): item 4r+j walks
// the root with only slot j enabled; a ray's list is the concatenation of its items' lists.
// Waves are persistent and draw items from a workgroup cursor exactly like k_traverse_lds (walk_binary.hip).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t CUR_NONE = 0x7FFFFFFFu;   // neither a shape index (< 2^28) nor an inner reference (bit 31)
#ifndef BVH_WIDE_INNER_STEPS
#define BVH_WIDE_INNER_STEPS 4
#endif
#ifndef BVH_WIDE_INNER_STEPS_WHOLE
#define BVH_WIDE_INNER_STEPS_WHOLE 8
#endif
#ifndef BVH_WIDE_INNER_STEPS_COHERENT
#define BVH_WIDE_INNER_STEPS_COHERENT 12
#endif
// walk steps between two refill phases: items of a ray cut into 16 are short (2 / 3 / 4 / 6 steps: 0.1225 / 0.1220 / 0.1219 / 0.1252 ms on
// configs[1]: a compile-time 4), whole rays walk for hundreds of steps (a kernel argument: 4 / 6 / 8 / 12 / 16 → 1.50 / 1.45 / 1.42 / 1.38 / 1.41 ms for
// 10 M primary rays on the stand-in scene, 2.28 / 2.28 / 2.26 / 2.27 / 2.30 for a 12.5 M-ray incoherent shard: 12 for batches the caller
// calls COHERENT, 8 otherwise)
#ifndef BVH_WIDE_MIN_WAVES_F32
#define BVH_WIDE_MIN_WAVES_F32 8   // __launch_bounds__: waves per SIMD the f32 kernel must allow (8 = two 1024-thread workgroups per CU)
#endif
#ifndef BVH_WIDE_MIN_WAVES_F64
#define BVH_WIDE_MIN_WAVES_F64 4   // f64: two 512-thread workgroups per CU
#endif
// An ITEM is (ray, j): the part of a ray's walk below the j-th of the 4^L subtrees L wide levels under the root (L = 1: the
// root's grandchildren, L = 2: their grandchildren).  No ancestor test is owed for a finite ray (see above), so items
// are independent walks and a ray's list is the concatenation of its items' lists in j order.  A workgroup tests each of
// its rays against the 4^L subtree boxes first and keeps the items whose box is hit in a compact list (62 % / 86 % of
// the items of the BASELINE stream die there); the walk then only ever draws live items.  Why: at 1 M rays a resident
// lane gets two rays, and the launch lasts as long as its unluckiest lanes (up to 66 dependent steps per ray); items of
// a quarter / a sixteenth of that length pack the lanes better (simulated critical path per workgroup 80 → 63 → 54 steps).
// Rays with a non-finite component are not cut: they travel as one item (j = WIDE_ITEM_WHOLE) from the root.
constexpr uint32_t WIDE_ITEM_WHOLE = 16;               // j of an uncut ray (its hits are filed under j = 0)


// reference of the subtree in slot `c` of a node that sits in LDS slot `q`: grandchildren that are resident too are named by
// their LDS slot (4-ary heap number), so that the walk never has to translate
__device__ __forceinline__ uint32_t wide_resident_ref(uint32_t ref, uint32_t q, uint32_t c, uint32_t K) {
    const uint32_t cs = 4u * q + 1u + c;
    return (ref != NONE && (ref & WIDE_INNER) && cs < K) ? (WIDE_INNER | WIDE_RESIDENT | cs) : ref;
}

// the four slab tests of one wide node → hit bits.  EXACT: the reference's NaN-aware sequence with the skipped child
// boxes rebuilt and tested first (see the header above).
template <typename T, bool EXACT>
__device__ __forceinline__ uint32_t wide_hits(const T o[3], const T inv[3], const WideRegs<T>& nd) {
    uint32_t m = 0;
    if (!EXACT) {   // absent slots carry NaN boxes: v_min / v_max3 keep the NaN and both compares fail
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const T mn[3] = {nd.mn[0][c], nd.mn[1][c], nd.mn[2][c]}, mx[3] = {nd.mx[0][c], nd.mx[1][c], nd.mx[2][c]};
            m |= slab_hit_finite<T>(o, inv, mn, mx) ? (1u << c) : 0u;
        }
        return m;
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c0 = 2 * p, c1 = 2 * p + 1;
        const T mn0[3] = {nd.mn[0][c0], nd.mn[1][c0], nd.mn[2][c0]}, mx0[3] = {nd.mx[0][c0], nd.mx[1][c0], nd.mx[2][c0]};
        T t0, t1;
        if (nd.ref[c1] == NONE) {   // the child is a leaf (or absent): its own box is in slot c0
            if (nd.ref[c0] != NONE && slab_hit<T>(o, inv, mn0, mx0, t0, t1)) m |= 1u << c0;
        } else {
            const T mn1[3] = {nd.mn[0][c1], nd.mn[1][c1], nd.mn[2][c1]}, mx1[3] = {nd.mx[0][c1], nd.mx[1][c1], nd.mx[2][c1]};
            T jmn[3], jmx[3];
#pragma unroll
            for (int k = 0; k < 3; k++) { jmn[k] = tmin(mn0[k], mn1[k]); jmx[k] = tmax(mx0[k], mx1[k]); }
            if (slab_hit<T>(o, inv, jmn, jmx, t0, t1)) {
                if (slab_hit<T>(o, inv, mn0, mx0, t0, t1)) m |= 1u << c0;
                if (slab_hit<T>(o, inv, mn1, mx1, t0, t1)) m |= 1u << c1;
            }
        }
    }
    return m;
}

// The 4^L item subtrees of a tree: box + reference, in pre-order (j = 4 * slot at wide level 1 + slot at wide level 2).  Every
// workgroup that needs them derives them itself from the root's wide node (and its four children's): two dependent loads.
#ifndef BVH_WIDE_LONG_FRAC
#define BVH_WIDE_LONG_FRAC 0.2   // of the box diagonal; measured on configs[1]: none 127 / 0.1 125 / 0.2 121 / 0.3 123.5 / 0.5 126.5 us
#endif
template <typename T> struct ItemTable {
    T box[16][6];
    uint32_t ref[16];
    T half_diag[16];   // scheduling only: an item whose ray stays inside the box for more than this is walked early (long walk expected)
};
template <typename T, int ITEMS_LOG4>
__device__ __forceinline__ void item_table_build(const WideNode<T>* __restrict__ wide, ItemTable<T>* tb, uint32_t tid) {
    constexpr uint32_t ITEMS = 1u << (2 * ITEMS_LOG4);
    if (tid < ITEMS) {
        const uint32_t c = ITEMS_LOG4 == 2 ? tid >> 2 : tid, k = tid & 3u;
        const WideNode<T>* root = wide;   // tree node 0
        uint32_t ref = root->ref[c];
        T b[6];
#pragma unroll
        for (int a = 0; a < 3; a++) { b[a] = root->mn[a][c]; b[3 + a] = root->mx[a][c]; }
        if (ITEMS_LOG4 == 2) {
            if (ref != NONE && (ref & WIDE_INNER)) {   // an inner grandchild of the root: its own four grandchildren
                const WideNode<T>* g = wide + (ref & (WIDE_RESIDENT - 1u));
                ref = g->ref[k];
#pragma unroll
                for (int a = 0; a < 3; a++) { b[a] = g->mn[a][k]; b[3 + a] = g->mx[a][k]; }
            } else if (k != 0) {                       // a leaf (or nothing): the whole of it is item 4c
                ref = NONE;
            }
        }
        if (ref == NONE) {
            const T nan = __builtin_nan("");
#pragma unroll
            for (int a = 0; a < 6; a++) b[a] = nan;
        }
#pragma unroll
        for (int a = 0; a < 6; a++) tb->box[tid][a] = b[a];
        tb->ref[tid] = ref;
        const T dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
        tb->half_diag[tid] = (T)BVH_WIDE_LONG_FRAC * sqrt(dx * dx + dy * dy + dz * dz);
    }
}
// LDS slot (4-ary heap number) of item j's subtree root
template <int ITEMS_LOG4> __device__ __forceinline__ uint32_t item_slot(uint32_t j) {
    return ITEMS_LOG4 == 2 ? 5u + j : 1u + j;   // level 1: 1 + c; level 2: 4 * (1 + c) + 1 + k = 5 + 4c + k
}

// The rays of one workgroup of the wide walk (64-ray blocks b, b + G, b + 2G, ... of the batch) → its live items, written
// into its own region of the list: the 4^L subtree boxes are tested, the survivors compacted per wave (one LDS atomic per
// wave and list end).  Items whose ray stays long inside their subtree's box (long walks expected) fill the list from the
// front, the others from the back — the walk draws from the front, so that the longest chains start first instead of setting
// the end of the launch.  Called by the walk's prologue or, earlier and beside the build, by k_wide_items.
struct GuideArgs;
__device__ __forceinline__ void guide_ray_load(const bvhgpu_ray_f64* __restrict__ rays64, uint32_t r, double S, float o[3], float inv[3], bool& bad);
// rays64 != NULL (GUIDE, T = float): the batch is an f64 one — every ray is converted where it is loaded (guide_ray_load) and *any_bad
// collects whether one of them lies outside the guide walk's range
template <typename T, int L4, bool GUIDE = false>
__device__ __forceinline__ void filter_rays_into_list(const ItemTable<T>* tb, const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays,
                                                      uint32_t* __restrict__ list, uint32_t per_wg, uint32_t my_rays, uint32_t G, uint32_t b,
                                                      uint32_t tid, uint32_t bd, int lane, uint32_t* s_nlist, uint32_t* s_nback,
                                                      const bvhgpu_ray_f64* __restrict__ rays64 = nullptr, double guide_S = 0.0, bool* any_bad = nullptr) {
    constexpr uint32_t ITEMS = 1u << (2 * L4);
    for (uint32_t l0 = 0; l0 < my_rays; l0 += bd) {   // workgroup-uniform
        const uint32_t local = l0 + tid;
        const uint32_t r = local < my_rays ? ((((local >> 6) * G + b) << 6) | (local & 63u)) : n_rays;
        uint32_t mask = 0, longm = 0;
        if (r < n_rays) {
            T o[3], inv[3];
            if constexpr (GUIDE) {
                bool bad;
                guide_ray_load(rays64, r, guide_S, o, inv, bad);
                *any_bad = *any_bad || bad;
            } else {
                const typename Traits<T>::Ray* rp = rays + r;
#pragma unroll
                for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; inv[k] = rp->inv[k]; }
            }
            if (!ray_is_finite<T>(o, inv)) {
                mask = 1u << WIDE_ITEM_WHOLE; longm = mask;
            } else {
#pragma unroll 4
                for (uint32_t j = 0; j < ITEMS; j++) {   // the boxes are workgroup-uniform: LDS broadcast reads
                    const T mn[3] = {tb->box[j][0], tb->box[j][1], tb->box[j][2]}, mx[3] = {tb->box[j][3], tb->box[j][4], tb->box[j][5]};
                    T len;
                    const bool hit = slab_hit_finite_len<T>(o, inv, mn, mx, len);
                    mask |= hit ? (1u << j) : 0u;
                    longm |= (hit && len > tb->half_diag[j]) ? (1u << j) : 0u;
                }
            }
        }
        const uint32_t cap = per_wg * ITEMS;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const uint32_t mm0 = side ? (mask & ~longm) : (mask & longm);
            const uint32_t mine = (uint32_t)__popc(mm0);
            uint32_t incl = mine;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const uint32_t u = __shfl_up(incl, d);
                if (lane >= d) incl += u;
            }
            const uint32_t total = __shfl(incl, WAVE - 1);
            uint32_t base = 0;
            if (lane == 0 && total) base = atomicAdd(side ? s_nback : s_nlist, total);
            base = __shfl(base, 0) + incl - mine;
            uint32_t mm = mm0;
            while (mm) {
                const uint32_t bit = (uint32_t)__ffs(mm) - 1u;
                mm &= mm - 1u;
                list[side ? cap - 1u - base : base] = (r << WIDE_ITEM_BITS) | bit;
                base++;
            }
        }
    }
}

// The item filter of a batch, EARLY: launched on the ctx's side stream behind the level pass that splits tree level 3, it
// runs beside the rest of the build (nine tenths of which leave the chip idle) instead of in front of the walk — the walk's
// prologue shrinks from 17-28 µs to the LDS image load.  The 16 item boxes are those of tree level 4 (heap numbers 16..31),
// read out of the BvhNode records of levels 0..3, which are final by then IF the level tier wrote them all (counter
// CTR_TOPMASK) and every level-4 node is an inner node; otherwise the kernel says so (front = NONE) and every workgroup of the
// walk filters its rays itself, as it does for a tree that is not being rebuilt.  Same grid as the walk (workgroup b owns the
// same 64-ray blocks and the same list region), a quarter of its threads: it is a guest on the chip.
template <typename T>
__global__ __launch_bounds__(256) void k_wide_items(const typename Traits<T>::Node* __restrict__ nodes, uint32_t n_nodes,
                                                    const uint32_t* __restrict__ node_count, const uint32_t* __restrict__ build_ctr,
                                                    const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays,
                                                    uint32_t* __restrict__ list_all, uint32_t* __restrict__ wg_items) {
    constexpr int L4 = 2;
    constexpr uint32_t ITEMS = 16;
    __shared__ ItemTable<T> tb;
    __shared__ uint32_t s_nlist, s_nback, s_bad;
    const uint32_t tid = threadIdx.x, bd = blockDim.x;
    const int lane = lane_id();
    if (tid == 0) { s_nlist = 0u; s_nback = 0u; s_bad = (build_ctr[BUILD_CTR_TOPMASK] & 0xFFFEu) == 0xFFFEu ? 0u : 1u; }
    __syncthreads();
    if (s_bad) { if (tid == 0) wg_items[2u * blockIdx.x] = NONE; return; }
    if (tid < ITEMS) {   // item j = subtree of heap number 16 + j: four steps down from the root, its box is in its parent's record
        uint32_t node = 0;
        T bx[6];
        bool ok = n_nodes > 1u;
        uint32_t cnt = ok ? node_count[0] : 0u;
#pragma unroll
        for (int lv = 3; lv >= 0 && ok; lv--) {
            const typename Traits<T>::Node nd = nodes[node];
            const uint32_t right = ((16u + tid) >> lv) & 1u;
            ok = nd.shape == NONE && nd.l < n_nodes && nd.r < n_nodes && nd.r > nd.l;
            if (!ok) break;
            const uint32_t nl = (nd.r - nd.l + 1u) >> 1;   // the left subtree holds 2 nl - 1 nodes (bvh_node.rs:138-142)
            cnt = right ? cnt - nl : nl;
            node = right ? nd.r : nd.l;
#pragma unroll
            for (int k = 0; k < 3; k++) { bx[k] = right ? nd.r_min[k] : nd.l_min[k]; bx[3 + k] = right ? nd.r_max[k] : nd.l_max[k]; }
        }
        ok = ok && cnt > 1u;   // the item's root must be an inner node (the walk names it by its wide node)
        if (!ok) atomicOr(&s_bad, 1u);
#pragma unroll
        for (int k = 0; k < 6; k++) tb.box[tid][k] = bx[k];
        const T dx = bx[3] - bx[0], dy = bx[4] - bx[1], dz = bx[5] - bx[2];
        tb.half_diag[tid] = (T)BVH_WIDE_LONG_FRAC * sqrt(dx * dx + dy * dy + dz * dz);
    }
    __syncthreads();
    if (s_bad) { if (tid == 0) wg_items[2u * blockIdx.x] = NONE; return; }
    const uint32_t n_blocks = (n_rays + 63u) >> 6;
    const uint32_t my_blocks = n_blocks > blockIdx.x ? (n_blocks - blockIdx.x + gridDim.x - 1u) / gridDim.x : 0u;
    const uint32_t per_wg = ((n_blocks + gridDim.x - 1u) / gridDim.x) << 6;
    uint32_t* list = list_all + (size_t)blockIdx.x * per_wg * ITEMS;
    filter_rays_into_list<T, L4>(&tb, rays, n_rays, list, per_wg, my_blocks << 6, gridDim.x, blockIdx.x, tid, bd, lane, &s_nlist, &s_nback);
    __syncthreads();
    if (tid == 0) { wg_items[2u * blockIdx.x] = s_nlist; wg_items[2u * blockIdx.x + 1u] = s_nback; }
}

// ---- guide walk: an f64 index batch walked over the tree's f32 guide boxes (common.hpp "guide boxes") -----------------------------------
// The f64 wide walk costs 1.9 x the f32 one (half-rate VALU, 13 instead of 7 chunks per node).  Only leaf tests decide a ray's list
// (monotonicity), so every inner test may be conservative: the walk converts every f64 ray to f32 (round to nearest) where it loads it (guide_ray_load) and
// flags rays the containment argument does not cover; the f32 wide walk then runs over `wide_guide` unchanged, except that a leaf
// CANDIDATE is confirmed by the f64 slab test of the shape's own f64 box with the f64 ray before it is reported.  Same lists, same order.
struct GuideArgs { const bvhgpu_ray_f64* rays64; const double* aabbs64; const float* info; const double* tris64; };   // info[0] = S (tree->guide_info); tris64: closest-hit batches
// The guide walk's f32 view of an f64 ray, made where the ray is loaded (round 4: a kernel of its own wrote an f32 copy of the batch first
// — 72 B read + 36 B written per ray and a launch, 19-22 µs per 1 M rays): origin and 1/d rounded to nearest, and the range test of the
// containment argument (common.hpp "guide boxes"); `bad` = the argument does not cover this ray.
__device__ __forceinline__ void guide_ray_load(const bvhgpu_ray_f64* __restrict__ rays64, uint32_t r, double S, float o[3], float inv[3], bool& bad) {
    const bvhgpu_ray_f64* q = rays64 + r;
    bad = !(S >= GUIDE_SCENE_MIN) || !(S <= GUIDE_SCENE_MAX);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double ok = q->o[k], ik = q->inv[k];
        const double ao = fabs(ok), ainv = fabs(ik), ai = ainv * (4.0 * S);
        // (NaN fails every comparison; S = 0 — a scene that is one point — leaves no room for the growth)
        bad = bad || !(ao <= GUIDE_ORIGIN_MAX * S) || !(ao <= GUIDE_F32_MAX) || !(ai <= 0x1p100) || !(ai >= 0x1p-100) ||
              !(ainv <= GUIDE_F32_MAX) || !(ainv >= GUIDE_F32_MIN_NORMAL);
        o[k] = (float)ok; inv[k] = (float)ik;
    }
}
// the f64 test of a leaf candidate (finite ray: the NaN-free form is exact, common.hpp slab_hit_finite)
__device__ __forceinline__ bool guide_leaf_hit(const GuideArgs& ga, uint32_t ray, uint32_t shape) {
    const bvhgpu_ray_f64* rp = ga.rays64 + ray;
    const double* b = ga.aabbs64 + 6 * (size_t)shape;
    const double o[3] = {rp->o[0], rp->o[1], rp->o[2]}, inv[3] = {rp->inv[0], rp->inv[1], rp->inv[2]};
    const double mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
    return slab_hit_finite<double>(o, inv, mn, mx);
}

// a leaf candidate of the guide walk that passed its f64 box, in a closest-hit batch: Ray::intersects_triangle in f64 (ray_impl.rs:154-213) and the
// reference's strict < against the lane's nearest so far (testbase.rs:831-833).  Inlined, although candidates are rare and the f64
// Möller–Trumbore needs more registers than the f32 walk around it owns: as a real call (__noinline__) the walk took 0.208 ms instead of
// 0.141 — the calling convention's register split costs the hot loop more than the spills around the rare branch do.
#ifndef BVH_GUIDE_CANDIDATE_ATTR
#define BVH_GUIDE_CANDIDATE_ATTR __forceinline__
#endif
__device__ BVH_GUIDE_CANDIDATE_ATTR double guide_candidate_distance(const bvhgpu_ray_f64* __restrict__ rays64, const double* __restrict__ tris64, uint32_t ray, uint32_t shape) {
    const bvhgpu_ray_f64* rp = rays64 + ray;
    const double o[3] = {rp->o[0], rp->o[1], rp->o[2]}, d[3] = {rp->d[0], rp->d[1], rp->d[2]};
    double out[3];
    ray_triangle<double>(o, d, tris64 + 9 * (size_t)shape, out);
    return out[0];
}

#ifdef BVH_WIDE_PROFILE   // developer build: per-wave timestamps (100 MHz wall clock) of the wide walk's phases
__device__ unsigned long long g_wide_prof[4 * 16384];
// lane-utilisation counts per wave (16 per wave): [0] wave-steps, [1] lanes on an inner node, [2] steps with a resident fetch,
// [3] steps with a non-resident fetch, [4] steps with a lane on the slow push path, [5] lanes on it, [6] lanes reporting a leaf,
// [7] steps with a report, [8] lanes holding an item (x steps), [9] refill rounds, [10] rounds on the exact (non-finite) path,
// [11] steps with a pop from the HBM part of the stack, [12] boxes hit (sum of popc(m)), [13] lanes whose node had no hit
__device__ unsigned long long g_wide_util[16 * 16384];
#endif
// ITEMS_LOG4 = 0: one item per ray, drawn by ray number.  1 / 2: every workgroup first cuts ITS rays into live items (its
// region of `list`, filled through an LDS counter — no global atomic: one address only takes ~88 atomics per µs on this
// chip, which made a separate filter kernel with one atomic per wave cost more than the walk) and then walks them.
template <typename T, int MODE, int ITEMS_LOG4, int MAX_THREADS, int MIN_WAVES, int GUIDE = 0>
__global__ __launch_bounds__(MAX_THREADS, MIN_WAVES) void k_traverse_wide(
    const WideNode<T>* __restrict__ wide, const uint32_t* __restrict__ wslot_node, uint32_t K, uint32_t stack_lds,
    const typename Traits<T>::Ray* __restrict__ rays, uint32_t n_rays, uint32_t* __restrict__ list_all, const uint32_t* __restrict__ wg_items,
    WalkOut<T> w, uint32_t* __restrict__ gstack, uint32_t gstack_cap, uint32_t* __restrict__ overflow, GuideArgs ga, uint32_t whole_steps) {
    static_assert(GUIDE == 0 || ((MODE == MODE_INDICES || MODE == MODE_CLOSEST) && sizeof(T) == 4), "the guide walk is the f32 walk of an f64 index / closest-hit batch");
    constexpr bool GUIDE_CLOSEST = GUIDE != 0 && MODE == MODE_CLOSEST;   // candidates are decided in f64 (guide_closest_candidate); the lane keeps (distance, shape)
    double gbest = 0.0;
    static_assert(ITEMS_LOG4 >= 0 && ITEMS_LOG4 <= 2, "1, 4 or 16 items per ray");
    static_assert(MODE != MODE_T_SLICE, "the t-slice output walks the binary array");
    constexpr int CH = WideIo<T>::CHUNKS;
    constexpr int L4 = ITEMS_LOG4 > 0 ? ITEMS_LOG4 : 1;      // (so that the item code compiles when it is not used)
    constexpr uint32_t ITEMS = 1u << (2 * L4);
    extern __shared__ __attribute__((aligned(16))) uint4 wsmem[];
    uint32_t& s_next = *reinterpret_cast<uint32_t*>(wsmem);
    uint32_t& s_nlist = *(reinterpret_cast<uint32_t*>(wsmem) + 1);
    uint32_t& s_nback = *(reinterpret_cast<uint32_t*>(wsmem) + 2);
    uint32_t* s_item_ref = reinterpret_cast<uint32_t*>(wsmem + 1);           // 16 references (64 bytes)
    uint4* nodes = wsmem + 5;
    uint32_t* s_stack = reinterpret_cast<uint32_t*>(nodes + (size_t)CH * K);
    const uint32_t bd = blockDim.x, tid = threadIdx.x;
    const int WIDE_INNER_STEPS = ITEMS_LOG4 == 0 ? (int)whole_steps : BVH_WIDE_INNER_STEPS;
    constexpr uint32_t SB = MAX_THREADS;   // stride of the LDS stack's entry planes: a constant, so that the three stores of a push share one address register
    const size_t G = (size_t)gridDim.x * bd, gid = (size_t)blockIdx.x * bd + tid;
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    // GUIDE: `rays` is unused — the batch is ga.rays64, every ray converted to f32 where it is loaded; guide_bad = one of this lane's
    // rays was outside the range the containment argument covers (the wave raises WALK_FLAG_GUIDE_RANGE at the end: the host replays in f64)
    double guide_S = 0.0;
    bool guide_bad = false;
    if constexpr (GUIDE != 0) guide_S = (double)ga.info[0];
#ifdef BVH_WIDE_PROFILE
    const unsigned long long prof_t0 = wall_clock64();
    unsigned long long prof_steps = 0;
    unsigned long long pu[16];
    for (int i = 0; i < 16; i++) pu[i] = 0;
    uint32_t pl_boxes = 0, pl_nohit = 0;
#endif
    // This workgroup's rays: the 64-ray blocks b, b + grid, b + 2 grid, ... of the batch.  (Contiguous ranges per workgroup
    // put all of a stream's expensive stretch — the BASELINE stream's first 5 000 rays start inside a cube — on a few
    // workgroups: the slowest workgroup finished at 158 µs against a mean of 115 µs.)
    const uint32_t n_blocks = (n_rays + 63u) >> 6;
    const uint32_t my_blocks = n_blocks > blockIdx.x ? (n_blocks - blockIdx.x + gridDim.x - 1u) / gridDim.x : 0u;
    const uint32_t per_wg = ((n_blocks + gridDim.x - 1u) / gridDim.x) << 6;   // capacity of a workgroup's share (host: the same formula)
    const uint32_t my_rays = my_blocks << 6;                                   // local ray numbers [0, my_rays), some beyond n_rays in the last block
    auto ray_of = [&](uint32_t local) -> uint32_t { return (((local >> 6) * gridDim.x + blockIdx.x) << 6) | (local & 63u); };
    // hits per 64-ray block of this workgroup (local block numbers): retiring items add to them, the workgroup stores them at
    // the end — the CSR scan then needs no reduce pass over the counts.  (LDS atomics: adding straight into global sums put
    // the BASELINE stream's 10 000 hits on one cache line, 128 → 162 µs.)
    __shared__ uint32_t s_bsum[WIDE_BSUM_MAX];
    if (w.scan_sums) for (uint32_t b = tid; b < WIDE_BSUM_MAX; b += bd) s_bsum[b] = 0u;
    if (tid == 0) { s_next = 0u; s_nlist = 0u; s_nback = 0u; }
    for (uint32_t q = tid; q < K; q += bd) {
        const uint32_t node = wslot_node[q];
        if (node != NONE) {
            const uint4* src = reinterpret_cast<const uint4*>(wide + node);
            uint4* dst = nodes + (size_t)q * CH;
#pragma unroll
            for (int c = 0; c < CH - 1; c++) dst[c] = src[c];
            uint4 rf = src[CH - 1];   // the four references: resident grandchildren by LDS slot
            rf.x = wide_resident_ref(rf.x, q, 0u, K); rf.y = wide_resident_ref(rf.y, q, 1u, K);
            rf.z = wide_resident_ref(rf.z, q, 2u, K); rf.w = wide_resident_ref(rf.w, q, 3u, K);
            dst[CH - 1] = rf;
        }
    }
    uint32_t* list = nullptr;
    if (ITEMS_LOG4 > 0) {
        __shared__ ItemTable<T> tb;
        item_table_build<T, L4>(wide, &tb, tid);
        __syncthreads();
        if (tid < ITEMS) {   // references of the item subtrees, resident ones by LDS slot
            const uint32_t ref = tb.ref[tid], slot = item_slot<L4>(tid);
            s_item_ref[tid] = (ref != NONE && (ref & WIDE_INNER) && slot < K) ? (WIDE_INNER | WIDE_RESIDENT | slot) : ref;
        }
        // rays → live items, into this workgroup's region of the list (at most ITEMS per ray) — unless the batch's early filter
        // (k_wide_items, enqueued beside the build of the tree) has done it already
        list = list_all + (size_t)blockIdx.x * per_wg * ITEMS;
        const uint32_t pre_front = wg_items ? wg_items[2u * blockIdx.x] : NONE;   // workgroup-uniform
        if (pre_front != NONE) {
            if (tid == 0) { s_nlist = pre_front; s_nback = wg_items[2u * blockIdx.x + 1u]; }
        } else {
            if constexpr (GUIDE != 0) filter_rays_into_list<T, L4, true>(&tb, rays, n_rays, list, per_wg, my_rays, gridDim.x, blockIdx.x, tid, bd, lane, &s_nlist, &s_nback,
                                                                            ga.rays64, guide_S, &guide_bad);
            else filter_rays_into_list<T, L4>(&tb, rays, n_rays, list, per_wg, my_rays, gridDim.x, blockIdx.x, tid, bd, lane, &s_nlist, &s_nback);
        }
        __threadfence_block();
    }
    __syncthreads();
    const uint32_t wg_begin = 0u;
    const uint32_t n_front = s_nlist;
    const uint32_t wg_end = ITEMS_LOG4 == 0 ? my_rays : n_front + s_nback;
#ifdef BVH_WIDE_PROFILE
    const unsigned long long prof_t1 = wall_clock64();
#endif

    LaneRay<T, MODE> ray;
    ray.clear();
    uint32_t cur = CUR_NONE, sp = 0, item = NONE;
    bool exhausted = wg_begin >= wg_end;   // wave-uniform: the workgroup's range has been handed out
    bool ovf = false;
    uint32_t pair_pend = NONE;   // pair records: the lane's hit that waits for its ray's next one
    PoolCursor pc;
    auto push_slow = [&](uint32_t v) {
        if (sp < stack_lds) s_stack[sp * SB + tid] = v;
        else if (sp - stack_lds < gstack_cap) gstack[(size_t)(sp - stack_lds) * G + gid] = v;
        else ovf = true;
        sp++;
    };
    auto pop_or_none = [&]() -> uint32_t {
        if (sp == 0) return CUR_NONE;
        sp--;
        if (sp < stack_lds) return s_stack[sp * SB + tid];
        return sp - stack_lds < gstack_cap ? gstack[(size_t)(sp - stack_lds) * G + gid] : CUR_NONE;
    };
    while (true) {
        // ---- refill phase
        bool run = cur != CUR_NONE;
        const unsigned long long idle = __ballot(!run);
        if (idle) {
            if (MODE == MODE_INDICES && ITEMS_LOG4 == 0 && w.pool_pair)   // (wave-uniform) a retiring ray's unpaired last hit
                report_pair(false, !run && item != NONE, 0u, ray, pair_pend, w.pool_pair, w.pool_cap, w.ctr, pc, lane, lt);
            if (!run && item != NONE) {   // the item has left the tree: its part of the ray's list is complete
                if (mode_first(MODE)) {
                    if constexpr (ITEMS_LOG4 == 0) {
                        const size_t r = item;
                        if constexpr (mode_pair(MODE)) { w.closest[2 * r] = ray.best[0]; w.closest[2 * r + 1] = ray.best[1]; }
                        else { w.closest[3 * r] = ray.best[0]; w.closest[3 * r + 1] = ray.best[1]; w.closest[3 * r + 2] = ray.best[2]; }
                        w.closest_prim[r] = ray.best_prim;
                    } else if (ray.best_prim != NONE) {
                        // The ray's list is the concatenation of its items' lists in item order, and this lane stopped at its item's first
                        // candidate inside the segment: the ray's answer is the candidate of the LOWEST item that found one.  Item (< 16) and
                        // shape (< 2^28: WIDE_MAX_SHAPES) fit one 32-bit key: one atomicMin; k_any_resolve recomputes the Intersection (k_box_resolve the t-slice,
                        // k_sphere_resolve the sphere hit).
                        const uint32_t j = item & ((1u << WIDE_ITEM_BITS) - 1u);
                        const uint32_t jj = j == WIDE_ITEM_WHOLE ? 0u : j;
                        atomicMin(&w.any_key[item >> WIDE_ITEM_BITS], (jj << 28) | ray.best_prim);
                    }
                } else if (MODE == MODE_CLOSEST || MODE == MODE_BOX_CLOSEST || MODE == MODE_SPHERE_CLOSEST) {   // (box: the distance is the entry parameter, non-negative; sphere: > eps — the same keys and slots)
                    if constexpr (ITEMS_LOG4 == 0) {
                        const size_t r = item;
                        if constexpr (mode_pair(MODE)) { w.closest[2 * r] = ray.best[0]; w.closest[2 * r + 1] = ray.best[1]; }
                        else if constexpr (!GUIDE_CLOSEST) { w.closest[3 * r] = ray.best[0]; w.closest[3 * r + 1] = ray.best[1]; w.closest[3 * r + 2] = ray.best[2]; }
                        w.closest_prim[r] = ray.best_prim;   // (guide: the shape only — k_closest_from_prim recomputes its Intersection in f64)
                    } else if (ray.best_prim != NONE) {
                        // The ray's other items sit in other lanes: the nearest candidate of the RAY is the minimum over its items of (distance, item
                        // number) — items are the tree-level-4 subtrees in pre-order, so on equal distances the lower item holds the candidate the
                        // reference's loop meets first (strict <, testbase.rs:831-833 behind flat_bvh.rs:408), and inside an item this lane kept the
                        // first one.  Distance (monotone key), item and shape (< 2^28: WIDE_MAX_SHAPES) fit one 64-bit word: one atomicMin.
                        const uint32_t j = item & ((1u << WIDE_ITEM_BITS) - 1u);
                        const uint32_t jj = j == WIDE_ITEM_WHOLE ? 0u : j;
                        if constexpr (sizeof(T) == 4 && !GUIDE_CLOSEST) {
                            const unsigned long long key = ((unsigned long long)Traits<T>::key(ray.best[0]) << 32) | ((unsigned long long)jj << 28) | (unsigned long long)ray.best_prim;
                            atomicMin(&w.closest_key[item >> WIDE_ITEM_BITS], key);
                        } else {
                            // f64: a 64-bit distance leaves no room for item and shape in one word.  Every item that found a candidate files its shape
                            // under (ray, item) — the slots the index walk uses for hit counts — and marks itself in the ray's item set;
                            // k_closest_resolve_slots walks the set in item order with the reference's strict <, recomputing each candidate's
                            // Intersection (the same instruction sequence: the same bits)
                            const size_t r = item >> WIDE_ITEM_BITS;
                            w.item_cnt[(r << (2 * ITEMS_LOG4)) + jj] = ray.best_prim;
                            atomicOr(&w.ray_items[r], 1u << jj);
                        }
                    }
                } else if (ray.cnt) {
                    uint32_t r = item;
                    if (ITEMS_LOG4 == 0) {
                        w.counts[item] = ray.cnt;
                    } else {
                        const uint32_t j = item & ((1u << WIDE_ITEM_BITS) - 1u);
                        const uint32_t jj = j == WIDE_ITEM_WHOLE ? 0u : j;
                        r = item >> WIDE_ITEM_BITS;
                        atomicAdd(&w.counts[r], ray.cnt);
                        atomicOr(&w.ray_items[r], 1u << jj);
                        w.item_cnt[((size_t)r << (2 * ITEMS_LOG4)) + jj] = ray.cnt;
                    }
                    if (w.scan_sums) atomicAdd(&s_bsum[((r >> 6) - blockIdx.x) / gridDim.x], ray.cnt);
                }
                item = NONE;
            }
            if (!exhausted) {
                const uint32_t nidle = (uint32_t)__popcll(idle);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_next, nidle);
                base = __builtin_amdgcn_readfirstlane(base);
                const uint32_t mine = base + (uint32_t)__popcll(idle & lt);
                if (!run && base < wg_end && mine < wg_end) {
                    if (ITEMS_LOG4 == 0) {
                        item = ray_of(mine);
                        if (item < n_rays) {
                            if constexpr (GUIDE != 0) { bool bad; guide_ray_load(ga.rays64, item, guide_S, ray.o, ray.inv, bad); guide_bad = guide_bad || bad; ray.loaded(item); gbest = __builtin_inf(); }
                            else ray.load(rays, item, w.tmax);
                            cur = WIDE_INNER | WIDE_RESIDENT | 0u;   // the root is heap slot 0 (K >= 1)
                        } else {
                            item = NONE;                         // padding of the batch's last 64-ray block
                        }
                    } else {
                        item = list[mine < n_front ? mine : per_wg * ITEMS - 1u - (mine - n_front)];
                        const uint32_t j = item & ((1u << WIDE_ITEM_BITS) - 1u);
                        if constexpr (GUIDE != 0) { bool bad; guide_ray_load(ga.rays64, item >> WIDE_ITEM_BITS, guide_S, ray.o, ray.inv, bad); ray.loaded(item >> WIDE_ITEM_BITS); gbest = __builtin_inf(); }   // (the filter has looked at its range)
                        else ray.load(rays, item >> WIDE_ITEM_BITS, w.tmax);
                        cur = j == WIDE_ITEM_WHOLE ? (WIDE_INNER | WIDE_RESIDENT | 0u) : s_item_ref[j];
                        if (j == WIDE_ITEM_WHOLE) item = item & ~((1u << WIDE_ITEM_BITS) - 1u);   // filed under j = 0
                    }
                    ray.r = item;                                // pool records are per item
                    sp = 0;
                    run = cur != CUR_NONE;
                }
                exhausted = base >= wg_end || (wg_end - base) <= nidle;
            }
            if (!__any(run)) break;
        }
        const bool fast = !__any(run && !ray.fin);   // wave-uniform
#ifdef BVH_WIDE_PROFILE
        prof_steps += WIDE_INNER_STEPS;
        pu[9]++; pu[10] += fast ? 0 : 1;
        pu[8] += WIDE_INNER_STEPS * (unsigned long long)__popcll(__ballot(run));
#endif
        for (int s = 0; s < WIDE_INNER_STEPS; s++) {
#ifdef BVH_WIDE_PROFILE
            {
                const bool in = (cur & WIDE_INNER) != 0u;
                pu[0]++; pu[1] += __popcll(__ballot(in));
                pu[2] += __any(in && (cur & WIDE_RESIDENT)) ? 1 : 0;
                pu[3] += __any(in && !(cur & WIDE_RESIDENT)) ? 1 : 0;
                const bool slow = in && sp + 3u > stack_lds;
                pu[4] += __any(slow) ? 1 : 0; pu[5] += __popcll(__ballot(slow));
                const bool lf = !in && cur < CUR_NONE;
                pu[6] += __popcll(__ballot(lf)); pu[7] += __any(lf) ? 1 : 0;
                pu[11] += __any((in || lf) && sp > stack_lds) ? 1 : 0;
            }
#endif
            if (cur & WIDE_INNER) {   // (CUR_NONE and shape indices have bit 31 clear)
                const uint32_t id = cur & (WIDE_RESIDENT - 1u);
                WideRegs<T> nd;
                if (cur & WIDE_RESIDENT) nd = WideIo<T>::from_lds(nodes, id);
                else nd = WideIo<T>::from_global(wide + id);
                const uint32_t m = fast ? wide_hits<T, false>(ray.o, ray.inv, nd) : wide_hits<T, true>(ray.o, ray.inv, nd);
                // the lowest hit slot is visited now, the others wait on the stack, highest slot first
                const uint32_t first = m & (0u - m);
                const uint32_t rest = m ^ first;
#ifdef BVH_WIDE_PROFILE
                pl_boxes += (uint32_t)__popc(m); pl_nohit += m == 0u ? 1u : 0u;
#endif
                const uint32_t s0 = (rest & 8u) ? nd.ref[3] : ((rest & 4u) ? nd.ref[2] : nd.ref[1]);
                const uint32_t s1 = ((rest & 12u) == 12u) ? nd.ref[2] : nd.ref[1];
                if (sp + 3u <= stack_lds) {   // room for three: store them all, count what is real
                    uint32_t* at = s_stack + sp * SB + tid;
                    at[0] = s0; at[SB] = s1; at[2 * SB] = nd.ref[1];
                    sp += (uint32_t)__popc(rest);
                } else {
                    if (rest & 8u) push_slow(nd.ref[3]);
                    if (rest & 4u) push_slow(nd.ref[2]);
                    if (rest & 2u) push_slow(nd.ref[1]);
                }
                cur = first == 0u ? pop_or_none() : (first == 1u ? nd.ref[0] : (first == 2u ? nd.ref[1] : (first == 4u ? nd.ref[2] : nd.ref[3])));
            }
            bool rec = cur < CUR_NONE;   // a leaf: report it, take the next pending grandchild
            const uint32_t shape = cur;
            if (rec) cur = pop_or_none();
            if (GUIDE) {   // a leaf candidate of the guide walk: the shape's own f64 box and the f64 ray decide (wave-uniform skip: candidates are rare)
                if (__any(rec)) {
                    if (rec) rec = guide_leaf_hit(ga, ITEMS_LOG4 == 0 ? ray.r : (ray.r >> WIDE_ITEM_BITS), shape);
                }
            }
            if (MODE == MODE_INDICES && ITEMS_LOG4 == 0 && w.raybuf) {   // (wave-uniform) the ray's first hits need no record: see WalkOut::raybuf
                if (rec && (ray.cnt >> w.stage_shift) == 0u) {
                    w.raybuf[((size_t)ray.r << w.stage_shift) | ray.cnt] = shape;
                    ray.cnt++;
                    rec = false;
                }
            }
            T t0 = 0, t1 = 0;
            if constexpr (mode_box(MODE)) {   // the leaf stage of the box modes: the literal t-slice of the shape's own AABB (the wide node that held it is gone,
                if (rec) {                    // and the NaN-free test that found it does not return the slice) — the same boolean, so rec stands
                    const T* b = w.box(shape);
                    const T mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
                    slab_hit<T>(ray.o, ray.inv, mn, mx, t0, t1);
                }
            }
            if constexpr (GUIDE_CLOSEST) {   // (wave-uniform skip, like the f64 box test above: candidates are rare)
                if (__any(rec)) {
                    if (rec) {
                        const double dist = guide_candidate_distance(ga.rays64, ga.tris64, ITEMS_LOG4 == 0 ? ray.r : (ray.r >> WIDE_ITEM_BITS), shape);
                        if (dist < gbest) { gbest = dist; ray.best_prim = shape; }
                        ray.cnt++;
                    }
                }
            } else if (MODE == MODE_INDICES && ITEMS_LOG4 == 0 && w.pool_pair) report_pair(rec, false, shape, ray, pair_pend, w.pool_pair, w.pool_cap, w.ctr, pc, lane, lt);   // (wave-uniform)
            else report<T, MODE>(rec, shape, t0, t1, ray, w, pc, lane, lt);
            if (mode_first(MODE) && ray.best_prim != NONE) { cur = CUR_NONE; sp = 0; }   // occluded: the item retires at the next refill
        }
        if (ovf) { cur = CUR_NONE; sp = 0; }
    }
    if (__any(ovf) && lane == 0) atomicOr(overflow, 4u);
    if constexpr (GUIDE != 0) { if (__any(guide_bad) && lane == 0) atomicOr(overflow, (uint32_t)WALK_FLAG_GUIDE_RANGE); }
    if (MODE == MODE_INDICES && ITEMS_LOG4 == 0 && w.pool_pair) {
        pool_invalidate_tail16(w.pool_pair, w.pool_cap, pc, lane);
        pc.left = 0;                                                // (nothing left for the epilogue's HitRec form to invalidate)
    }
    walk_epilogue<T, MODE>(w, pc, lane, false, 0, 0, 0, 0);
    if (MODE < MODE_CLOSEST && w.scan_sums) {   // every wave of the workgroup gets here: all items of its rays have retired
        __syncthreads();
        // one atomic per 64-ray block that has hits, on the sum of its scan block (workgroups finish at different times and a
        // scan block's 16 sums come from 16 workgroups: nothing like the per-item atomics that were tried first)
        for (uint32_t b = tid; b < my_blocks; b += bd)
            if (s_bsum[b]) atomicAdd(&w.scan_sums[(b * gridDim.x + blockIdx.x) / (uint32_t)(SCAN_BLOCK / 64)], s_bsum[b]);
    }
#ifdef BVH_WIDE_PROFILE
    if (lane == 0) {
        const size_t wv = gid >> 6;
        if (wv < 16384) {
            g_wide_prof[4 * wv] = prof_t0; g_wide_prof[4 * wv + 1] = prof_t1; g_wide_prof[4 * wv + 2] = wall_clock64(); g_wide_prof[4 * wv + 3] = prof_steps;
            for (int i = 0; i < 12; i++) g_wide_util[16 * wv + i] = pu[i];
            g_wide_util[16 * wv + 12] = 0; g_wide_util[16 * wv + 13] = 0;
        }
    }
    __syncthreads();
    if ((gid >> 6) < 16384) { atomicAdd(&g_wide_util[16 * (gid >> 6) + 12], (unsigned long long)pl_boxes); atomicAdd(&g_wide_util[16 * (gid >> 6) + 13], (unsigned long long)pl_nohit); }
#endif
}

// ---- wide walk launch ------------------------------------------------------------------------
// Workgroup geometry: `wg_per_cu` workgroups of `threads` share a CU's 160 KB of LDS; each keeps the per-lane stack
// (stack_lds entries x threads x 4 B) and as many top-of-tree wide nodes as fit in the rest.
template <typename T> struct WideGeom {
    uint32_t threads, wg_per_cu, stack_lds, K;
    size_t lds_bytes;
    WideGeom(const bvhgpu_ctx* ctx, bool whole_rays, bool coherent = false) {
        const bool f64 = sizeof(T) == 8;
        const int want_threads = ctx->tune[BVHGPU_TUNE_WIDE_THREADS] > 0 ? ctx->tune[BVHGPU_TUNE_WIDE_THREADS] : (f64 ? 512 : 1024);
        threads = (uint32_t)std::min(f64 ? 512 : 1024, std::max(64, want_threads & ~63));
        wg_per_cu = (uint32_t)std::max(1, std::min(ctx->tune[BVHGPU_TUNE_WIDE_WG_PER_CU] > 0 ? ctx->tune[BVHGPU_TUNE_WIDE_WG_PER_CU] : 2,
                                                   (int)(2048 / threads)));
        // 16 items per ray (short walks below tree level 4): 4 / 6 / 8 / 10 / 12 entries measured, 6; whole rays on the stand-in scene (a lane on the
        // slow push path in 68-93 % of the steps with 6): 4 / 6 / 8 / 10 / 12 / 16 → 1.71 / 1.58 / 1.50 / 1.48 / 1.47 / 1.50 ms for 10 M primary rays,
        // 2.79 / 2.46 / 2.28 / 2.31 / 2.39 / 2.60 ms for a 12.5 M-ray incoherent shard: 8, and 10 for batches the caller calls COHERENT (with 12 steps
        // between refills: 8 / 10 / 12 entries → 1.39 / 1.36 / 1.37 ms)
        stack_lds = (uint32_t)std::max(0, std::min(ctx->tune[BVHGPU_TUNE_WIDE_STACK_LDS] >= 0 ? ctx->tune[BVHGPU_TUNE_WIDE_STACK_LDS] : (whole_rays ? (coherent ? 10 : 8) : 6), 32));
        // static LDS of the kernel: item table (448 / 832 bytes) + block sums (512 bytes)
        const size_t budget = (size_t)(160 * 1024) / wg_per_cu - (f64 ? 1536 : 1024);
        const size_t stack_stride = f64 ? 512 : 1024;   // (the kernel's MAX_THREADS: its stack planes have a fixed stride)
        const size_t fixed = 80 + (size_t)stack_lds * stack_stride * 4;
        const size_t per_slot = (size_t)WideIo<T>::CHUNKS * 16;
        size_t k = budget > fixed + per_slot ? (budget - fixed) / per_slot : 1;
        if (ctx->tune[BVHGPU_TUNE_WIDE_SLOTS] > 0) k = std::min<size_t>(k, (size_t)ctx->tune[BVHGPU_TUNE_WIDE_SLOTS]);
        K = (uint32_t)std::max<size_t>(1, std::min<size_t>(k, WIDE_SLOTS));
        lds_bytes = 80 + (size_t)K * per_slot + (size_t)stack_lds * stack_stride * 4;
    }
};
// Workgroups of the wide walk for a batch: one ray per lane — unless the rays are cut into items (16 per ray: a workgroup's lanes stay busy
// with a quarter of the rays) and the batch is too small to fill the chip's workgroup slots that way: then the rays are spread over all
// slots, down to BVHGPU_TUNE_WIDE_MIN_RAYS_PER_WG rays per workgroup.  (One ray per lane, a small batch takes the time of ONE workgroup's
// 1024 rays whatever its size; bvhgpu_traverse_host_* walks its batches in such chunks.  profiles/r6_walk_size_sweep.log)
inline size_t wide_grid(const bvhgpu_ctx* ctx, uint32_t threads, uint32_t wg_per_cu, size_t n_rays, int items_log4) {
    const size_t slots = (size_t)ctx->n_cu * wg_per_cu;
    size_t per_wg = threads;
    const int min_rays = ctx->tune[BVHGPU_TUNE_WIDE_MIN_RAYS_PER_WG];
    if (items_log4 == 2 && min_rays > 0 && n_rays * 4 <= slots * threads) {   // (measured: 33 K / 66 K / 125 K rays 48 -> 37 / 38 / 41 µs; 250 K rays 49 -> 53)
        const size_t spread = ((n_rays + slots - 1) / slots + 63) & ~(size_t)63;
        per_wg = std::min<size_t>(threads, std::max<size_t>(spread, (size_t)std::max(64, min_rays & ~63)));
    }
    const size_t full = (n_rays + per_wg - 1) / per_wg;
    return std::min<size_t>(std::max<size_t>(full, 1), slots);
}
constexpr uint32_t WIDE_GSTACK = 24;   // stack entries per lane beyond the LDS part, in HBM (a walk pushes at most 3 per wide level)
// (tests/test_gpu_refit.py WIDE_STACK restates this and WideGeom's smallest default LDS part, 6, to know on which trees no lane can overflow)

// GUIDE: T = float on an f64 tree — the nodes are the tree's guide boxes, rays_dev unused (NULL), ga the f64 batch: every ray is converted where the walk loads it (guide_ray_load)
template <typename T, int MODE, int ITEMS_LOG4, int GUIDE = 0>
static void launch_wide(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h,
                        uint32_t* ovf_flag, bool early_items, GuideArgs ga = GuideArgs{nullptr, nullptr, nullptr, nullptr}) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const WideGeom<T> g(ctx, ITEMS_LOG4 == 0, (h->flags & BVHGPU_TRAVERSE_COHERENT) != 0);
    const dim3 grid((unsigned)wide_grid(ctx, g.threads, g.wg_per_cu, n_rays, ITEMS_LOG4));
    uint32_t* list = nullptr;
    if (ITEMS_LOG4 > 0) {   // every workgroup's region of the live-item list: its rays x 4^L entries
        const size_t n_blocks = (n_rays + 63) / 64;
        const size_t per_wg = ((n_blocks + grid.x - 1) / grid.x) * 64;   // k_traverse_wide: capacity of a workgroup's share
        h->witems.reserve(((size_t)grid.x * per_wg << (2 * ITEMS_LOG4)) * 4 + 16);
        list = h->witems.as<uint32_t>();
    }
    const uint32_t* wg_items = nullptr;
    if (ITEMS_LOG4 == 2 && early_items) {
        // The item filter runs on the ctx's side stream as soon as the build on the main stream has split tree level 3 (t->ev_top) —
        // beside the remaining level passes and the workgroup / wave tiers, which leave most of the chip idle — and the walk waits
        // for it (h->ev_items) instead of filtering in its own prologue.  k_wide_items checks on the device that the top of the tree
        // is what this needs; if not, every workgroup of the walk filters its rays itself.
        if (!ctx->side) BVH_HIP(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        if (!h->ev_items) BVH_HIP(hipEventCreateWithFlags(&h->ev_items, hipEventDisableTiming));
        h->wg_items.reserve((size_t)grid.x * 2 * 4 + 16);
        BVH_HIP(hipStreamWaitEvent(ctx->side, t->ev_top, 0));
        hipLaunchKernelGGL(k_wide_items<T>, grid, dim3(256), 0, ctx->side, t->nodes.as<typename Traits<T>::Node>(), (uint32_t)t->n_nodes,
                           t->node_count.as<uint32_t>(), t->ctr.as<uint32_t>(), rays_dev, (uint32_t)n_rays, list, h->wg_items.as<uint32_t>());
        BVH_HIP(hipEventRecord(h->ev_items, ctx->side));
        BVH_HIP(hipStreamWaitEvent(st, h->ev_items, 0));
        wg_items = h->wg_items.as<uint32_t>();
    }
    const size_t lanes = (size_t)grid.x * g.threads;
    h->wstack.reserve(lanes * WIDE_GSTACK * 4);
    constexpr int MAXT = sizeof(T) == 8 ? 512 : 1024;
    constexpr int MINW = sizeof(T) == 8 ? BVH_WIDE_MIN_WAVES_F64 : BVH_WIDE_MIN_WAVES_F32;
    auto kern = &k_traverse_wide<T, MODE, ITEMS_LOG4, MAXT, MINW, GUIDE>;
    char name[128];
    std::snprintf(name, sizeof name, "bvhgpu::k_traverse_wide<%s, %d, %d, %d, %d, %d>", walk_type_name<T>(), MODE, ITEMS_LOG4, MAXT, MINW, GUIDE);
    static thread_local size_t lds_attr[16] = {};   // per device: dynamic-LDS limit already set for this instantiation
    size_t& have = lds_attr[ctx->device & 15];
    if (have < g.lds_bytes) {
        BVH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
        have = g.lds_bytes;
    }
    hipLaunchKernelGGL(kern, grid, dim3(g.threads), g.lds_bytes, st, GUIDE ? t->wide_guide.as<WideNode<T>>() : t->wide.as<WideNode<T>>(),
                       t->wslot_node.as<uint32_t>(), g.K, g.stack_lds, rays_dev, (uint32_t)n_rays, list, wg_items, w, h->wstack.as<uint32_t>(),
                       WIDE_GSTACK, ovf_flag, ga,
                       (uint32_t)((h->flags & BVHGPU_TRAVERSE_COHERENT) ? BVH_WIDE_INNER_STEPS_COHERENT : BVH_WIDE_INNER_STEPS_WHOLE));
    h->walk_kernel = name;
}

// the cuts that exist: whole rays or 16 items per ray for every mode, 4 items for the CSR modes only
template <typename T, int MODE, int GUIDE = 0>
static void launch_wide_items(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int items_log4,
                              uint32_t* ovf_flag, bool early_items, GuideArgs ga = GuideArgs{nullptr, nullptr, nullptr, nullptr}) {
    if (items_log4 == 2) { launch_wide<T, MODE, 2, GUIDE>(t, rays_dev, n_rays, w, h, ovf_flag, early_items, ga); return; }
    if constexpr (MODE < MODE_CLOSEST) {
        if (items_log4 == 1) { launch_wide<T, MODE, 1, GUIDE>(t, rays_dev, n_rays, w, h, ovf_flag, false, ga); return; }
    }
    launch_wide<T, MODE, 0, GUIDE>(t, rays_dev, n_rays, w, h, ovf_flag, false, ga);
}

// use_guide (f64 index and closest-hit batches only): the f32 walk over the tree's guide boxes, leaf candidates decided in f64
// early_items: the item filter beside the build (launch_wide), for CSR batches cut into 16 items
template <typename T>
void launch_wide_walk(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, int items_log4,
                      bool use_guide, bool early_items, uint32_t* ovf_flag) {
    if constexpr (sizeof(T) == 8) {
        if (use_guide) {
            // the same outputs: the guide walk touches none of the T-typed ones (an index batch has no values; a closest-hit batch leaves the
            // shapes in closest_prim — or the (ray, item) slots — and k_closest_from_prim / k_closest_resolve_slots compute the Intersections)
            WalkOut<float> wg{};
            wg.counts = w.counts; wg.pool = w.pool; wg.pool_cap = w.pool_cap; wg.ctr = w.ctr; wg.closest_prim = w.closest_prim;
            wg.item_cnt = w.item_cnt; wg.ray_items = w.ray_items; wg.scan_sums = w.scan_sums;
            wg.pool_pair = w.pool_pair; wg.raybuf = w.raybuf; wg.stage_shift = w.stage_shift;
            // (the guide walk converts every f64 ray where it loads it: no f32 copy of the batch; a closest-hit batch decides every leaf
            //  candidate's box AND triangle in f64)
            const GuideArgs ga{reinterpret_cast<const bvhgpu_ray_f64*>(rays_dev), t->aabbs.as<double>(), t->guide_info.as<float>(),
                               mode == MODE_CLOSEST ? t->tris.as<double>() : nullptr};
            if (mode == MODE_CLOSEST) launch_wide_items<float, MODE_CLOSEST, 1>(t, nullptr, n_rays, wg, h, items_log4, ovf_flag, false, ga);
            else launch_wide_items<float, MODE_INDICES, 1>(t, nullptr, n_rays, wg, h, items_log4, ovf_flag, false, ga);
            return;
        }
    }
    switch (mode) {
        case MODE_INDICES: launch_wide_items<T, MODE_INDICES>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, early_items); break;
        case MODE_TRIANGLES: launch_wide_items<T, MODE_TRIANGLES>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, early_items); break;
        case MODE_ANY: launch_wide_items<T, MODE_ANY>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
        case MODE_BOX_CLOSEST: launch_wide_items<T, MODE_BOX_CLOSEST>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
        case MODE_BOX_FIRST: launch_wide_items<T, MODE_BOX_FIRST>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
        case MODE_SPHERE_CLOSEST: launch_wide_items<T, MODE_SPHERE_CLOSEST>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
        case MODE_SPHERE_FIRST: launch_wide_items<T, MODE_SPHERE_FIRST>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
        default: launch_wide_items<T, MODE_CLOSEST>(t, rays_dev, n_rays, w, h, items_log4, ovf_flag, false); break;
    }
}
template void launch_wide_walk<float>(bvhgpu_tree*, const bvhgpu_ray_f32*, size_t, const WalkOut<float>&, bvhgpu_hits*, int, int, bool, bool, uint32_t*);
template void launch_wide_walk<double>(bvhgpu_tree*, const bvhgpu_ray_f64*, size_t, const WalkOut<double>&, bvhgpu_hits*, int, int, bool, bool, uint32_t*);

// workgroups of the launch that launch_wide_walk makes for such a batch (the guide walk of an f64 batch launches the f32 geometry)
template <typename T>
size_t wide_walk_grid(const bvhgpu_ctx* ctx, size_t n_rays, int items_log4, bool coherent, bool use_guide) {
    if (sizeof(T) == 8 && use_guide) return wide_walk_grid<float>(ctx, n_rays, items_log4, coherent, false);
    const WideGeom<T> g(ctx, items_log4 == 0, coherent);
    return wide_grid(ctx, g.threads, g.wg_per_cu, n_rays, items_log4);
}
template size_t wide_walk_grid<float>(const bvhgpu_ctx*, size_t, int, bool, bool);
template size_t wide_walk_grid<double>(const bvhgpu_ctx*, size_t, int, bool, bool);

#ifdef BVH_WIDE_PROFILE
void debug_wide_prof(unsigned long long* out, size_t n) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide_prof), sizeof(unsigned long long) * n);
}
void debug_wide_util(unsigned long long* out, size_t n) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide_util), sizeof(unsigned long long) * n);
}
#endif

}  // namespace bvhgpu
