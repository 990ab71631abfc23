// query.hip — <FlatBvh as BoundingHierarchy>::traverse (src/flat_bvh.rs:396-431) for a BATCH of the crate's other three
// IntersectsAabb queries (src/aabb/intersection.rs:35-45, src/ball.rs:102-106): axis-aligned boxes, points and balls.
//
// A query's list is the reference's: the shapes of the leaf entries the flat-array walk reaches and whose own AABB passes, in
// pre-order (left first).  The per-kind predicates are restated operation by operation (-ffp-contract=off, no fast-math):
//   AABB   Aabb::intersects_aabb (aabb_impl.rs:240-248): miss iff on some axis q.max < lo || hi < q.min
//   POINT  Aabb::contains (aabb_impl.rs:175-177): p >= lo && p <= hi component by component (nalgebra's partial order)
//   BALL   Ball::intersects_aabb (ball.rs:85-99): s = ((0 + d0*d0) + d1*d1) + d2*d2, d = clamp(c, lo, hi) - c with num_traits'
//          clamp (c < lo ? lo : (c > hi ? hi : c)), hit iff s <= r*r (powi(2) = x*x)
// Two walks, both writing the hit pool / counts that traverse_enqueue's CSR path (count scan, scatter, pool growth with replay)
// turns into offsets + indices exactly as for a ray batch:
//   k_query       one query per lane, stackless over the folded binary array (common.hpp TravNode: hit → i+1, miss → exit) — or,
//                 for a tree with a split that had no SAH winner, over the reference-layout FlatNode array (see launch_query);
//   k_query_wide  one query per lane over the wide nodes (common.hpp WideNode), four grandchild boxes per step, a per-lane stack
//                 of (node, slots still to visit) in LDS; a lane whose stack is full raises the overflow flag and the batch is
//                 replayed with k_query.
#include <cstdio>

#include "walk.hpp"

namespace bvhgpu {

// ---- the three predicates -------------------------------------------------------------------------------------------------
template <typename T, int KIND> struct QueryLane {
    T a[KIND == BVHGPU_QUERY_AABB ? 6 : 3];
    T rr;   // BALL: radius * radius
    __device__ __forceinline__ void load(const T* __restrict__ q, uint32_t i) {
        if (KIND == BVHGPU_QUERY_AABB) {
#pragma unroll
            for (int k = 0; k < 6; k++) a[k] = q[6 * (size_t)i + k];
        } else if (KIND == BVHGPU_QUERY_POINT) {
#pragma unroll
            for (int k = 0; k < 3; k++) a[k] = q[3 * (size_t)i + k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) a[k] = q[4 * (size_t)i + k];
            const T r = q[4 * (size_t)i + 3];
            rr = r * r;
        }
    }
    __device__ __forceinline__ bool hits(const T lo[3], const T hi[3]) const {
        if (KIND == BVHGPU_QUERY_AABB) {
            bool miss = false;
#pragma unroll
            for (int k = 0; k < 3; k++) miss = miss | (a[3 + k] < lo[k]) | (hi[k] < a[k]);
            return !miss;
        } else if (KIND == BVHGPU_QUERY_POINT) {
            bool in = true;
#pragma unroll
            for (int k = 0; k < 3; k++) in = in & (a[k] >= lo[k]) & (a[k] <= hi[k]);
            return in;
        } else {
            T s = (T)0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const T c = a[k];
                const T cl = c < lo[k] ? lo[k] : (c > hi[k] ? hi[k] : c);
                const T d = cl - c;
                const T dd = d * d;
                s = s + dd;
            }
            return s <= rr;
        }
    }
};

// ------------------------------------------------------------------------------------------------
// binary walk: one query per lane.  LAYOUT 0 = the folded TravNode array (a leaf entry tests the shape's own AABB, which for a tree
// built here is bit-identical to its navigator box; an uploaded FlatBvh is mirrored 1:1 there), LAYOUT 1 = the FlatNode array exactly
// as flat_bvh.rs:408-427 walks it (navigator box, then the leaf entry's shape AABB) — for trees whose build had a split without SAH
// winner: both child boxes of such a split are Aabb::empty(), which a finite box query or a point misses but a NaN box query (and a
// ball whose r*r is +inf) hits, so a leaf's navigator box there is NOT its shape's box and folding it away would change the list.
// ------------------------------------------------------------------------------------------------
template <typename T, int KIND, int LAYOUT>
__global__ __launch_bounds__(256) void k_query(const void* __restrict__ entries, uint32_t n_entries, const T* __restrict__ aabbs,
                                               const T* __restrict__ queries, uint32_t n, WalkOut<T> w) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    const bool active = qi < n;
    QueryLane<T, KIND> q;
    if (active) q.load(queries, qi);
    LaneRay<T, MODE_INDICES> lr;   // (only r and cnt: the pool bookkeeping of report())
    lr.clear();
    if (active) { lr.r = qi; lr.cnt = 0; }
    uint32_t i = active ? 0u : n_entries;
    PoolCursor pc;
    while (true) {
        const bool run = i < n_entries;
        if (!__any(run)) break;
        bool rec = false;
        uint32_t shape = NONE;
        if (run) {
            if (LAYOUT == 0) {
                const NodeRegs<T> nd = load_node(reinterpret_cast<const TravNode<T>*>(entries) + i);
                const bool hit = q.hits(nd.mn, nd.mx);
                shape = nd.shape;
                rec = hit && trav_is_leaf(shape);
                i = hit ? i + 1 : nd.exit;   // a leaf's exit IS i+1
            } else {
                const typename Traits<T>::Flat* f = reinterpret_cast<const typename Traits<T>::Flat*>(entries) + i;
                const uint32_t entry = f->entry, exit_ = f->exit;
                T mn[3], mx[3];
                if (entry == NONE) {   // leaf entry: the shape's own AABB (flat_bvh.rs:411-418)
                    shape = f->shape;
                    const T* sb = aabbs + 6 * (size_t)shape;
#pragma unroll
                    for (int k = 0; k < 3; k++) { mn[k] = sb[k]; mx[k] = sb[3 + k]; }
                    rec = q.hits(mn, mx);
                    i = exit_;
                } else {
#pragma unroll
                    for (int k = 0; k < 3; k++) { mn[k] = f->min[k]; mx[k] = f->max[k]; }
                    i = q.hits(mn, mx) ? entry : exit_;
                }
            }
        }
        report<T, MODE_INDICES>(rec, shape, (T)0, (T)0, lr, w, pc, lane, lt);
    }
    if (active) lr.retire(w);
    walk_epilogue<T, MODE_INDICES>(w, pc, lane, false, 0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// Wide walk.  Why skipping the odd tree levels returns the reference's list: FlatBvh::traverse reports shape s iff the predicate holds
// for every ancestor box of s and for s's own AABB.  In a tree built here (or refitted, or imported from such a build) every ancestor
// box is the exact join of the boxes below it: lo_A <= lo_s and hi_A >= hi_s component by component.
//   AABB   a miss on A (q.max < lo_A or hi_A < q.min on some axis) implies the same strict comparison against lo_s <= ... / hi_s >= ...
//          on s: a miss on A implies a miss on s, for EVERY query — a NaN component makes both comparisons false on every box (all hit),
//          an inverted or infinite query box is compared literally on both sides of the implication.
//   POINT  lo_s <= p <= hi_s implies lo_A <= p <= hi_A; a NaN point fails every comparison (no hit anywhere).
// So for these two kinds the ancestor tests are pure pruning and the walk may skip the boxes of the odd levels, as long as it keeps
// the pre-order.  BALL is monotone only for non-inverted boxes: |clamp(c, lo, hi) - c| shrinks as the box grows when lo <= hi, but a
// shape AABB with min > max on an axis (the builder accepts any finite box) breaks it (lo = 5, hi = 3, c = 4.9: d = 0.1; grown to
// lo = 0, hi = 4: d = -0.9).  Ball walks therefore rebuild each skipped child box as the join of its two grandchild boxes (exact, up
// to the sign of a zero, which neither the clamp nor the square sees) and test it before the grandchildren: every box the reference
// tests is tested, in its order — exact whatever the boxes.
// An absent slot carries a NaN box, which PASSES the AABB and BALL predicates (every comparison is false): absent slots are rejected by
// their reference (NONE), never by their box.  Trees with empty child bounds (a split without SAH winner), uploaded FlatBvhs and
// trees of fewer than two shapes never reach this kernel.
// Per lane: the current node, the set of its hit slots still to visit and their references in registers; a stack of (node | set << 28)
// for the ancestors that still have slots to visit (one entry per wide level at most: a tree of up to 2 * QW_STACK levels below the
// root never overflows it), entry-major in LDS.
// ------------------------------------------------------------------------------------------------
constexpr int QW_THREADS = 256;
constexpr int QW_STACK = 16;
constexpr uint32_t QW_NODE_MASK = 0x0FFFFFFFu;   // node index bits of a stack entry (launch_query: 2n - 1 tree nodes fit 28 bits)

template <typename T, int KIND>
__device__ __forceinline__ uint32_t query_wide_hits(const QueryLane<T, KIND>& q, const WideRegs<T>& nd) {
    uint32_t m = 0;
    if (KIND != BVHGPU_QUERY_BALL) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const T mn[3] = {nd.mn[0][c], nd.mn[1][c], nd.mn[2][c]}, mx[3] = {nd.mx[0][c], nd.mx[1][c], nd.mx[2][c]};
            m |= (nd.ref[c] != NONE && q.hits(mn, mx)) ? (1u << c) : 0u;
        }
        return m;
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c0 = 2 * p, c1 = 2 * p + 1;
        const T mn0[3] = {nd.mn[0][c0], nd.mn[1][c0], nd.mn[2][c0]}, mx0[3] = {nd.mx[0][c0], nd.mx[1][c0], nd.mx[2][c0]};
        if (nd.ref[c1] == NONE) {   // the child is a leaf (its box in slot c0) or absent
            if (nd.ref[c0] != NONE && q.hits(mn0, mx0)) m |= 1u << c0;
        } else {
            const T mn1[3] = {nd.mn[0][c1], nd.mn[1][c1], nd.mn[2][c1]}, mx1[3] = {nd.mx[0][c1], nd.mx[1][c1], nd.mx[2][c1]};
            T jmn[3], jmx[3];
#pragma unroll
            for (int k = 0; k < 3; k++) { jmn[k] = tmin(mn0[k], mn1[k]); jmx[k] = tmax(mx0[k], mx1[k]); }
            if (q.hits(jmn, jmx)) {
                if (q.hits(mn0, mx0)) m |= 1u << c0;
                if (q.hits(mn1, mx1)) m |= 1u << c1;
            }
        }
    }
    return m;
}

template <typename T, int KIND>
__global__ __launch_bounds__(QW_THREADS) void k_query_wide(const WideNode<T>* __restrict__ wide, const T* __restrict__ queries, uint32_t n,
                                                           WalkOut<T> w, uint32_t* __restrict__ ovf_flag) {
    __shared__ uint32_t s_stack[QW_STACK * QW_THREADS];
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = lane_id();
    const unsigned long long lt = lanemask_lt();
    const bool active = qi < n;
    QueryLane<T, KIND> q;
    LaneRay<T, MODE_INDICES> lr;
    lr.clear();
    uint32_t node = 0, mask = 0, sp = 0;
    uint32_t ref[4] = {NONE, NONE, NONE, NONE};
    if (active) {
        q.load(queries, qi);
        lr.r = qi; lr.cnt = 0;
        const WideRegs<T> nd = WideIo<T>::from_global(wide);   // the root
        mask = query_wide_hits<T, KIND>(q, nd);
#pragma unroll
        for (int c = 0; c < 4; c++) ref[c] = nd.ref[c];
    }
    bool overflow = false;
    PoolCursor pc;
    while (true) {
        const bool run = !overflow && (mask != 0 || sp != 0);
        if (!__any(run)) break;
        bool rec = false;
        uint32_t shape = NONE;
        if (run) {
            if (mask == 0) {   // back to the nearest ancestor with slots left: its references again (16 bytes of its node)
                sp--;
                const uint32_t e = s_stack[sp * QW_THREADS + threadIdx.x];
                node = e & QW_NODE_MASK;
                mask = e >> 28;
                const uint4 r4 = *reinterpret_cast<const uint4*>(wide[node].ref);
                ref[0] = r4.x; ref[1] = r4.y; ref[2] = r4.z; ref[3] = r4.w;
            }
            const int c = __builtin_ctz(mask);
            mask &= mask - 1u;
            const uint32_t r = c == 0 ? ref[0] : (c == 1 ? ref[1] : (c == 2 ? ref[2] : ref[3]));
            if (!(r & WIDE_INNER)) {   // a leaf: its box (= the shape's AABB) passed
                rec = true;
                shape = r;
            } else {
                if (mask != 0) {
                    if (sp == (uint32_t)QW_STACK) {
                        overflow = true;
                    } else {
                        s_stack[sp * QW_THREADS + threadIdx.x] = node | (mask << 28);
                        sp++;
                    }
                }
                if (!overflow) {
                    node = r & ~WIDE_INNER;
                    const WideRegs<T> nd = WideIo<T>::from_global(wide + node);
                    mask = query_wide_hits<T, KIND>(q, nd);
#pragma unroll
                    for (int k = 0; k < 4; k++) ref[k] = nd.ref[k];
                }
            }
        }
        report<T, MODE_INDICES>(rec, shape, (T)0, (T)0, lr, w, pc, lane, lt);
    }
    if (__any(overflow) && lane == 0) atomicOr(ovf_flag, 4u);   // (bit 2, like the ray walk's stack: traverse_check replays with k_query)
    if (active) lr.retire(w);
    walk_epilogue<T, MODE_INDICES>(w, pc, lane, false, 0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// BVHGPU_TUNE_QUERY_VARIANT = -1, measured on configs[1]'s scene with both walks forced (tools/query_bench.py, profiles/r7_query_bench.json:
// batches of 256 .. 1 M queries, about 6 hits per box / ball query; wall clock of the whole call, binary / wide): the wide walk wins for
// points (f32 1.24 - 1.34x up to 64 K queries, 1.07 at 250 K, 0.94 at 1 M; f64 1.08 - 1.33 at every size), is level for boxes (f32
// 0.95 - 1.03, f64 0.99 - 1.09) and loses for f32 balls (0.86 - 0.99: a ball also tests the rebuilt child box of every pair, six tests
// per node instead of four) and f64 balls below 250 K (0.89 - 0.98; 1.01 - 1.05 from 250 K).  The default takes the wide walk where it
// was ahead or level at every measured size.
#ifndef BVH_QUERY_POINT_WIDE_MAX_F32
#define BVH_QUERY_POINT_WIDE_MAX_F32 262144   // f32 points: the wide walk below this many queries
#endif
#ifndef BVH_QUERY_BALL_WIDE_MIN_F64
#define BVH_QUERY_BALL_WIDE_MIN_F64 262144    // f64 balls: the wide walk from this many queries on
#endif
static bool query_wide_by_default(int kind, bool f64, size_t n) {
    if (kind == BVHGPU_QUERY_POINT) return f64 || n < (size_t)BVH_QUERY_POINT_WIDE_MAX_F32;
    if (kind == BVHGPU_QUERY_AABB) return f64;
    return f64 && n >= (size_t)BVH_QUERY_BALL_WIDE_MIN_F64;
}

template <typename T> static const char* qtype_name() { return sizeof(T) == 4 ? "float" : "double"; }

template <typename T>
void launch_query(bvhgpu_tree* t, size_t n, const WalkOut<T>& w, bvhgpu_hits* h, uint32_t* ovf_flag) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const int kind = h->pend_kind;
    const T* q = static_cast<const T*>(h->pend_queries);
    const int knob = ctx->tune[BVHGPU_TUNE_QUERY_VARIANT];
    const bool wide_ok = t->has_wide && !t->exact_only && !t->unfolded && t->n >= 2 && 2 * t->n <= (size_t)QW_NODE_MASK && !h->force_binary;
    const bool use_wide = wide_ok && (knob == 1 || (knob < 0 && query_wide_by_default(kind, sizeof(T) == 8, n)));
    h->pend_qwide = use_wide;
    char name[96];
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (use_wide) {
        std::snprintf(name, sizeof name, "bvhgpu::k_query_wide<%s, %d>", qtype_name<T>(), kind);
        const WideNode<T>* wn = t->wide.as<WideNode<T>>();
        switch (kind) {
            case BVHGPU_QUERY_AABB: hipLaunchKernelGGL((k_query_wide<T, BVHGPU_QUERY_AABB>), dim3(grid), dim3(QW_THREADS), 0, st, wn, q, (uint32_t)n, w, ovf_flag); break;
            case BVHGPU_QUERY_POINT: hipLaunchKernelGGL((k_query_wide<T, BVHGPU_QUERY_POINT>), dim3(grid), dim3(QW_THREADS), 0, st, wn, q, (uint32_t)n, w, ovf_flag); break;
            default: hipLaunchKernelGGL((k_query_wide<T, BVHGPU_QUERY_BALL>), dim3(grid), dim3(QW_THREADS), 0, st, wn, q, (uint32_t)n, w, ovf_flag); break;
        }
        h->walk_kernel = name;
        return;
    }
    ensure_flat_arrays(t);   // (a lazy flatten wrote the wide walk's arrays only: the binary arrays follow now)
    // a tree with a split that had no SAH winner and was built here: the FlatNode array (the folded array lost the leaves' navigator
    // boxes); do_query refuses such a tree when it was imported and has no FlatNode array
    const int layout = (t->exact_only && !t->unfolded) ? 1 : 0;
    const void* entries = layout ? t->flat.p : t->trav.p;
    const uint32_t n_entries = (uint32_t)(layout ? t->n_flat : t->n_trav);
    std::snprintf(name, sizeof name, "bvhgpu::k_query<%s, %d, %d>", qtype_name<T>(), kind, layout);
    const T* aabbs = t->aabbs.as<T>();
#define QUERY_LAUNCH(K, L) hipLaunchKernelGGL((k_query<T, K, L>), dim3(grid), dim3(256), 0, st, entries, n_entries, aabbs, q, (uint32_t)n, w)
    switch (kind) {
        case BVHGPU_QUERY_AABB: if (layout) QUERY_LAUNCH(BVHGPU_QUERY_AABB, 1); else QUERY_LAUNCH(BVHGPU_QUERY_AABB, 0); break;
        case BVHGPU_QUERY_POINT: if (layout) QUERY_LAUNCH(BVHGPU_QUERY_POINT, 1); else QUERY_LAUNCH(BVHGPU_QUERY_POINT, 0); break;
        default: if (layout) QUERY_LAUNCH(BVHGPU_QUERY_BALL, 1); else QUERY_LAUNCH(BVHGPU_QUERY_BALL, 0); break;
    }
#undef QUERY_LAUNCH
    h->walk_kernel = name;
}

// the batch to completion: traverse_enqueue (walk + count scan + scatter), then the check that grows the pool / switches to the binary
// walk and replays (traverse_check), as for a synchronous ray batch
template <typename T>
void query_batch(bvhgpu_tree* t, int kind, const T* queries_dev, size_t n, bvhgpu_hits* h) {
    h->force_binary = false; h->pend_attempts = 0;
    h->pend_kind = kind; h->pend_queries = queries_dev; h->pend_qwide = false;
    for (;;) {
        traverse_enqueue<T>(t, nullptr, n, 0u, h);
        BVH_HIP(hipStreamSynchronize(t->ctx->stream));
        if (traverse_check(h)) return;
    }
}

template void launch_query<float>(bvhgpu_tree*, size_t, const WalkOut<float>&, bvhgpu_hits*, uint32_t*);
template void launch_query<double>(bvhgpu_tree*, size_t, const WalkOut<double>&, bvhgpu_hits*, uint32_t*);
template void query_batch<float>(bvhgpu_tree*, int, const float*, size_t, bvhgpu_hits*);
template void query_batch<double>(bvhgpu_tree*, int, const double*, size_t, bvhgpu_hits*);

}  // namespace bvhgpu
