// instances_within.hip — every (instance, shape) within max_dist of every query point over an instance set, in order, as a CSR
// (bvhgpu_instances_within_*; include/bvh_mi355x.h).
//
// The definition is within.hip's loop twice.  Point p_j comes with m = max_dist[j]; r2 = m * m is ONE multiplication in T; a negative or
// NaN m gives an empty row without a walk.  The top-level array is walked with the world point and r2: a non-leaf entry is entered iff
// min_distance_squared(box, p) <= r2, a leaf entry (instance i) sends the lane into member tree_of[i] with
//   q[k] = row4(Y_i[k], p)                                       the point in the object's frame
//   F    = (row3(Y_i[0], Y_i[0]) + row3(Y_i[1], Y_i[1])) + row3(Y_i[2], Y_i[2])      the squared Frobenius norm of Y_i's 3x3 part
//   r2o  = r2 * F                                                the limit in the object's frame
// and the member's array is walked with q and r2o; a leaf entry (shape s) there is decided in WORLD space:
//   w[v][k] = row4(X_i[k], tri_s[v]);   d = triangle_dist2(w, p);   (i, s) is a candidate with key d iff d <= r2.
// |p - X v| >= |q - v| / ||Y||_F, so every point of a world triangle within m of p lies within m * ||Y||_F of q: the object-frame prune is
// conservative (in exact arithmetic; a pair whose d lies within rounding of r2 may be decided by a box test, as §4i found for one tree),
// and the threshold never moves, so the candidate set does not depend on the order of the walk.  A NaN r2o (0 * inf) passes no box test.
//   Row j, default: ALL candidates in a stable ascending sort by d; equal d stay in the double order (instances in the top level's list
//   order, within each the shapes in the member's).  No key is NaN (a NaN d fails <=).  The output distance is sqrt(d).
//   BVHGPU_INSTANCES_WITHIN_LIST_ORDER: the double order, no sort pass.  BVHGPU_INSTANCES_WITHIN_COUNT_ONLY: `offsets` alone.
//
// The batch is rows.hip's schedule (count walk, scan, ONE host read, offsets, fill walk, a workgroup per long row) with a point per lane.
// Every walk is instances_within_walk: ONE loop, a lane is either in the top-level array (point p, limit r2) or in a member's (point q,
// limit r2o) — instances_allhits.hip's state machine with within.hip's step — and no walk has a cross-lane operation.
//   k_instances_within_count     counts[j] = the candidates of point j (lanes with a negative or NaN limit do not walk)
//   k_instances_within_fill      A row of a sorted batch up to INST_WITHIN_LANE_ROW_MAX is built by the lane's stable insertion (search from the
//                                back with the strict <) on its own region — the key of element e lives in dist[e] — and a final per-lane
//                                pass turns the keys into sqrt.  A LIST_ORDER row gets (instance, shape, sqrt(d)) appended as the walk meets
//                                them.  A longer row of a sorted batch gets (d, instance) appended in the double order, its shapes into a
//                                scratch row in the same order (and its positions, beyond INST_WITHIN_LDS_ROW_MAX) and is left to
//   k_instances_within_sort_row  rows_bitonic on the keys (d, position) with the instance as payload, in LDS up to INST_WITHIN_LDS_ROW_MAX
//                                elements, in place in global memory beyond; the shape of an element is gathered from the scratch row by
//                                its position; then sqrt.
// The row length is uniform per workgroup of k_instances_within_sort_row: every loop bound and every barrier there depends on it alone.
//
// Which arrays are walked: region.hip's rule (RegionMember), array by array, in a table made by every batch (instances_arrays.hpp InstWithinArr; the last
// row is the top level's).  The folded `trav` array for a built tree (a leaf entry carries the shape's — the instance's — own box and
// tests it), the UNFOLDED rule for an uploaded FlatBvh and a one-shape tree (a leaf entry is entered untested), and an unfolded mirror of
// the FlatNode array (unfold.hpp) for a built tree with empty child bounds — the top level included, whose build over the world boxes
// can meet a split without SAH winner like any other.
//
// MASKED (bvhgpu_instances_within_masked_*): point j carries a mask P[j] and the walk passes over an instance whose mask shares
// no bit with it, at its top-level leaf: one 4-byte load, no record, no X_i, no member table.  The candidate set does not depend on the
// walk's order, so the row is the unmasked row without the hidden instances' pairs.  The count walk and the fill walk read the same two
// arrays and so take the same decision for every (point, instance): the offsets are what the fill writes.  A point whose mask is 0 does not
// walk.  k_instances_within_sort_row only ever sees pairs that are already in a row: no mask.
#include <cstdio>
#include <vector>

#include "instances_arrays.hpp"
#include "point_dist.hpp"
#include "rows.hpp"

namespace bvhgpu {

// Thresholds: within.hip's, taken over unmeasured for this family.  An element sorted in LDS is an f64 key, a position
// and an instance — rows_lds_row_max_ok's 16 bytes: 32 KB a row in f64, 24 KB in f32; the shapes stay in global memory.
constexpr uint32_t INST_WITHIN_LANE_ROW_MAX = 32;
constexpr uint32_t INST_WITHIN_LDS_ROW_MAX = 2048;
static_assert(rows_lds_row_max_ok(INST_WITHIN_LDS_ROW_MAX), "a row sorted in LDS must fit a workgroup's LDS, padded to a power of two");

// what the walks read of the set
template <typename T> struct InstWithinScene {
    const InstWithinArr<T>* arrs;   // n_trees + 1 rows
    const InstRec<T>* recs;
    const T* xforms;                // n x 12: X_i as committed
    uint32_t top;                   // the top level's row of `arrs`
};

template <typename T> struct InstWithinPoint {
    T p[3], r2;
    bool walk;   // the limit is neither negative nor NaN
    __device__ __forceinline__ void load(const T* __restrict__ points, const T* __restrict__ max_dist, uint32_t q) {
        for (int c = 0; c < 3; c++) p[c] = points[3 * (size_t)q + c];
        const T m = max_dist[q];
        r2 = m * m;
        walk = m >= (T)0;
    }
};

// One point per lane, ONE loop.  on_candidate(instance, shape, d) for every pair the definition keeps, in the double order.  X_i is read
// once on entry to an instance and carried through the member's walk: 6 (f64: 16) registers more across the loop than reading it again
// at every accepted leaf, no scratch either way, and the faster of the two where it was timed (DESIGN.md §4n has both forms' figures).
// MASKED: pmask is the point's mask; an instance with (inst_mask[i] & pmask) == 0 is passed over at its leaf and the lane goes on in the top level.
template <typename T, typename F, bool MASKED = false>
__device__ __forceinline__ void instances_within_walk(const InstWithinScene<T>& sc, const InstWithinPoint<T>& pt, F&& on_candidate,
                                                      const uint32_t* __restrict__ inst_mask = nullptr, uint32_t pmask = 0xFFFFFFFFu) {
    const InstWithinArr<T> top = sc.arrs[sc.top];
    const TravNode<T>* nodes = top.nodes;
    const T* tris = nullptr;
    T p[3] = {pt.p[0], pt.p[1], pt.p[2]};
    T lim = pt.r2;
    T xr[12] = {};   // X_i of the instance the lane is in
    uint32_t i = 0, end = top.n_trav, unfolded = top.unfolded, inst = NONE, top_next = 0;
    while (i < end) {
        const NodeRegs<T> nd = load_node(nodes + i);
        const bool leaf = trav_is_leaf(nd.shape);
        bool enter = true;
        if (!(unfolded != 0u && leaf)) {   // (a leaf entry of an unfolded array has no navigator test)
            const T md = aabb_min_dist2<T>(nd.mn, nd.mx, p);
            enter = md <= lim;
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
                    for (int k = 0; k < 3; k++) w[3 * v + k] = row4<T>(xr + 4 * k, tv);
                }
                const T d = triangle_dist2<T>(w, pt.p);
                if (d <= pt.r2) on_candidate(inst, nd.shape, d);
            } else {              // an instance: into its member with the point and the limit in the object's frame
                bool visible = true;
                if constexpr (MASKED) visible = (inst_mask[nd.shape] & pmask) != 0u;   // (hidden: the lane stays here and goes on at nd.exit)
                if (visible) {
                    top_next = i;
                    inst = nd.shape;
                    const InstRec<T> rec = load_rec<T>(sc.recs + inst);
                    const InstWithinArr<T> a = sc.arrs[rec.tree];
                    T f[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) { p[k] = row4<T>(rec.y + 4 * k, pt.p); f[k] = row3<T>(rec.y + 4 * k, rec.y + 4 * k); }
                    const T f01 = f[0] + f[1];
                    const T fn = f01 + f[2];
                    lim = pt.r2 * fn;
                    const T* x = sc.xforms + 12 * (size_t)inst;
#pragma unroll
                    for (int k = 0; k < 12; k++) xr[k] = x[k];
                    nodes = a.nodes; tris = a.tris; i = 0; end = a.n_trav; unfolded = a.unfolded;
                }
            }
        }
        if (inst != NONE && i >= end) {   // the member's array has ended: back to the top level, behind the leaf that sent the lane here
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = pt.p[k];
            lim = pt.r2;
            nodes = top.nodes; i = top_next; end = top.n_trav; unfolded = top.unfolded; inst = NONE;
        }
    }
}

template <typename T, bool MASKED = false>
__global__ __launch_bounds__(256) void k_instances_within_count(InstWithinScene<T> sc, const T* __restrict__ points, const T* __restrict__ max_dist, uint32_t n,
                                                                uint32_t* __restrict__ counts, InstMasks mk) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    InstWithinPoint<T> pt;
    pt.load(points, max_dist, q);
    uint32_t cnt = 0;
    auto count = [&](uint32_t, uint32_t, T) { cnt++; };
    if constexpr (MASKED) {
        const uint32_t pmask = mk.ray ? mk.ray[q] : 0xFFFFFFFFu;
        if (pt.walk && pmask != 0u) instances_within_walk<T, decltype(count)&, true>(sc, pt, count, mk.inst, pmask);
    } else {
        if (pt.walk) instances_within_walk<T>(sc, pt, count);
    }
    counts[q] = cnt;
}

// ---- the second walk ----------------------------------------------------------------------------------------------------------------
// list_shape: NULL, or total u32 — the shapes of the long rows in the double order (a sorted batch that has long rows)
// pos:        NULL, or total u32 — the positions of the rows beyond INST_WITHIN_LDS_ROW_MAX (a sorted batch that has such rows)
template <typename T, bool SORTED, bool MASKED = false>
__global__ __launch_bounds__(256) void k_instances_within_fill(InstWithinScene<T> sc, const T* __restrict__ points, const T* __restrict__ max_dist, uint32_t n,
                                                               const uint32_t* __restrict__ offsets, uint32_t* __restrict__ instance,
                                                               uint32_t* __restrict__ shape, T* __restrict__ dist, uint32_t* __restrict__ list_shape,
                                                               uint32_t* __restrict__ pos, InstMasks mk) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;
    if (len == 0) return;   // (the count pass walked this point, or refused its limit: nothing to write)
    InstWithinPoint<T> pt;
    pt.load(points, max_dist, q);
    uint32_t* __restrict__ ri = instance + beg;
    uint32_t* __restrict__ rs = shape + beg;
    T* __restrict__ rd = dist + beg;
    const bool insert = SORTED && len <= INST_WITHIN_LANE_ROW_MAX;
    const bool with_list = SORTED && !insert && list_shape != nullptr;
    const bool with_pos = SORTED && pos != nullptr && len > INST_WITHIN_LDS_ROW_MAX;
    uint32_t cnt = 0;
    auto put = [&](uint32_t inst, uint32_t s, T d) {
        if (cnt >= len) return;   // (never: this walk is the count pass's; a lane stays inside its own region whatever happens)
        if (insert) {
            // ascending list: the first element e with d < e is where a scan from the back stops, so search and shift are one loop
            uint32_t hole = cnt;
#pragma unroll 1
            while (hole > 0) {
                const T e = rd[hole - 1];
                if (!(d < e)) break;
                rd[hole] = e;
                ri[hole] = ri[hole - 1];
                rs[hole] = rs[hole - 1];
                hole--;
            }
            rd[hole] = d;
            ri[hole] = inst;
            rs[hole] = s;
        } else if (SORTED) {   // a long row: (d, instance) and the shape in the double order for k_instances_within_sort_row
            rd[cnt] = d;
            ri[cnt] = inst;
            if (with_list) list_shape[beg + cnt] = s;
            if (with_pos) pos[beg + cnt] = cnt;
        } else {               // the double order: the distance as the walk meets it
            rd[cnt] = sqrt(d);
            ri[cnt] = inst;
            rs[cnt] = s;
        }
        cnt++;
    };
    if constexpr (MASKED) {   // (the count walk's decision: the same two arrays; a row with len != 0 has a mask that is not 0)
        const uint32_t pmask = mk.ray ? mk.ray[q] : 0xFFFFFFFFu;
        instances_within_walk<T, decltype(put)&, true>(sc, pt, put, mk.inst, pmask);
    } else {
        instances_within_walk<T>(sc, pt, put);
    }
    if (insert) {
#pragma unroll 1
        for (uint32_t j = 0; j < cnt; j++) rd[j] = sqrt(rd[j]);
    }
}

// one workgroup per long row of a sorted batch
template <typename T>
__global__ __launch_bounds__(ROWS_SORT_THREADS) void k_instances_within_sort_row(const uint32_t* __restrict__ work, const uint32_t* __restrict__ offsets,
                                                                                uint32_t* instance, uint32_t* shape, T* dist,
                                                                                const uint32_t* __restrict__ list_shape, uint32_t* pos) {
    __shared__ T ld[INST_WITHIN_LDS_ROW_MAX];
    __shared__ uint32_t lp[INST_WITHIN_LDS_ROW_MAX];
    __shared__ uint32_t li[INST_WITHIN_LDS_ROW_MAX];
    const uint32_t q = work[blockIdx.x];
    const uint32_t beg = offsets[q], len = offsets[q + 1] - beg;   // uniform over the workgroup
    uint32_t P = 1;
    while (P < len) P <<= 1;
    uint32_t* ri = instance + beg;
    uint32_t* rs = shape + beg;
    T* rd = dist + beg;
    const bool in_lds = len <= INST_WITHIN_LDS_ROW_MAX;
    if (in_lds) {
        for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) { ld[e] = rd[e]; lp[e] = e; li[e] = ri[e]; }
        __syncthreads();
        rows_bitonic<T, false>(ld, 1u, lp, li, len, P);
    } else {   // (the host passes the positions whenever a row is this long, and checks that it does)
        __threadfence_block();
        __syncthreads();
        rows_bitonic<T, true>(rd, 1u, pos + beg, ri, len, P);
    }
    // the shape of every element by its position in the double order, and the distance (the network ended with a barrier)
    for (uint32_t e = threadIdx.x; e < len; e += ROWS_SORT_THREADS) {
        const uint32_t p = in_lds ? lp[e] : pos[beg + e];
        if (p >= len) continue;   // (the positions are a permutation of 0 .. len - 1: no read beyond the row's scratch whatever happens)
        rs[e] = list_shape[beg + p];
        if (in_lds) { ri[e] = li[e]; rd[e] = sqrt(ld[e]); }
        else rd[e] = sqrt(rd[e]);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool MASKED>
static void instances_within_launch(bvhgpu_instances* s, const InstWithinScene<T>& sc, const T* points_dev, const T* max_dist_dev, size_t n, bool sorted,
                                    bool count_only, bvhgpu_hits* h, const uint32_t* point_mask_dev) {
    hipStream_t st = s->ctx->stream;
    const InstMasks mk = {MASKED ? s->masks.as<uint32_t>() : nullptr, MASKED ? point_mask_dev : nullptr};
    const uint32_t n32 = (uint32_t)n;
    const dim3 pgrid((unsigned)((n + 255) / 256)), block(256);
    const RowsPlan plan = {sorted, count_only, INST_WITHIN_LANE_ROW_MAX, INST_WITHIN_LDS_ROW_MAX, sizeof(T), true, true};
    rows_run(h, n, plan,
             [&](uint32_t* counts) { hipLaunchKernelGGL((k_instances_within_count<T, MASKED>), pgrid, block, 0, st, sc, points_dev, max_dist_dev, n32, counts, mk); },
             [&](const RowsOut& o, auto SORTED) {
                 hipLaunchKernelGGL((k_instances_within_fill<T, decltype(SORTED)::value, MASKED>), pgrid, block, 0, st, sc, points_dev, max_dist_dev, n32, o.offsets,
                                    o.instance, o.shape, static_cast<T*>(o.vals), o.list_shape, o.pos, mk);
             },
             [&](const RowsOut& o, uint32_t n_long) {
                 hipLaunchKernelGGL((k_instances_within_sort_row<T>), dim3(n_long), dim3(ROWS_SORT_THREADS), 0, st, o.work, o.offsets, o.instance, o.shape,
                                    static_cast<T*>(o.vals), o.list_shape, o.pos);
             });
}

// the points of a batch over a committed instance set (the caller has checked commit, staleness and the members' kinds)
// masked: bvhgpu_instances_within_masked_* — the set's masks against point_mask_dev (NULL: all ones); otherwise point_mask_dev is not looked at
template <typename T>
void instances_within_batch(bvhgpu_instances* s, const T* points_dev, const T* max_dist_dev, size_t n, unsigned flags, bvhgpu_hits* h, bool masked,
                            const uint32_t* point_mask_dev) {
    const bool sorted = (flags & BVHGPU_INSTANCES_WITHIN_LIST_ORDER) == 0;
    const bool count_only = (flags & BVHGPU_INSTANCES_WITHIN_COUNT_ONLY) != 0;
    char name[96];
    const char* m = masked ? ", true" : "";   // (the unmasked names are what they were)
    if (count_only) std::snprintf(name, sizeof name, "bvhgpu::k_instances_within_count<%s%s>", walk_type_name<T>(), m);
    else std::snprintf(name, sizeof name, "bvhgpu::k_instances_within_fill<%s, %s%s>", walk_type_name<T>(), sorted ? "true" : "false", m);
    rows_batch(h, s->ctx, Traits<T>::dtype, TRAVERSE_INST_WITHIN, 0, count_only, n, s->n == 0, name, [&] {   // (empty: no instances)
        // the table of the batch: which array of every member and of the top level (instances_arrays.hpp), in the result object
        const InstWithinArr<T>* arrs = instances_array_table<T>(s, h->unfold, h->rg_members, h->rg_members_host);
        const InstWithinScene<T> sc = {arrs, s->recs.as<InstRec<T>>(), s->xforms.as<T>(), (uint32_t)s->trees.size()};
        if (masked) instances_within_launch<T, true>(s, sc, points_dev, max_dist_dev, n, sorted, count_only, h, point_mask_dev);
        else instances_within_launch<T, false>(s, sc, points_dev, max_dist_dev, n, sorted, count_only, h, nullptr);
    });
}
template void instances_within_batch<float>(bvhgpu_instances*, const float*, const float*, size_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);
template void instances_within_batch<double>(bvhgpu_instances*, const double*, const double*, size_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);

}  // namespace bvhgpu
