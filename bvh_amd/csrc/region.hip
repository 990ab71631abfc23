// region.hip — every shape whose box passes a convex region (a set of planes) for every region of a batch, in list order, as a CSR
// (bvhgpu_region_*; include/bvh_mi355x.h): frustum culling, shadow-cascade slabs, froxels, portals, selection prisms.
//
// The definition is FlatBvh::traverse (flat_bvh.rs:396-431) with the plane-set test below in place of intersects_aabb.  Region q is m
// planes (nx, ny, nz, d) in the tree's dtype T; a box [lo, hi] passes when for every plane, in order,
//   p[k] = (n[k] >= 0) ? hi[k] : lo[k];   s = dot3(n, p) + d;   s >= 0          (walk.hpp dot3; every operation rounded once, no contraction)
// (-0 takes hi, a NaN component takes lo, a NaN s is a miss, m = 0 passes every box).  An inner entry tests its box and goes to i + 1 on
// a pass and to `exit` otherwise; a leaf entry tests the shape's own AABB and reports the shape on a pass.  BVHGPU_REGION_CLASSIFY adds a
// byte per reported shape: 1 iff the same sums with the opposite corner, p'[k] = (n[k] >= 0) ? lo[k] : hi[k], are all >= 0.
//
// Culling batches are 1 .. a few thousand regions of which one may return a third of the scene, so a lane per region (query.hip) is
// the wrong shape.  The unit of work here is (region, chunk): a chunk is a contiguous range of `chunk_entries` entries of the pre-order
// array, and ONE WAVEFRONT owns one unit.  The batch is rows.hip's schedule over the n x n_chunks units (count launch, scan, ONE host read,
// offsets, fill launch; no sort, no worklist); the caller's offsets[q] is the scanned word at q * n_chunks (k_region_offsets).  Inside a
// unit the order is entry order and the units of a region concatenate in chunk order, so a row is in list order without a sort and
// without an atomic.
//
// Window scan (region_unit).  The wave reads 64 consecutive entries, lane l tests entry i + l (coalesced 2 KB / 4 KB through load_node).
//   skip   the largest `exit` of the failing inner entries seen so far: per lane the exclusive prefix maximum over the window, carried
//          in from earlier windows.  An entry is live iff its index >= skip: it is not inside a subtree the walk left.  A dead failing
//          entry may take part in the maximum: its subtree is nested in the one that skipped it.
//   report a live passing leaf goes to base + popcount(ballot & lanemask_lt)
//   next   i = max(i + 64, skip), clipped to the chunk end: a missed large subtree is jumped over, a small one costs at most 63 tests.
// Chunk start.  What matters of the entries in front of a chunk is the ancestors of its first entry s: the inner entries a < s with
// exit_a > s.  k_region_ancestors writes them once per batch (a lane per chunk descends from entry 0 following `exit`), up to
// REGION_ANC_MAX per chunk and their count; the unit's wave tests them in one gather step and starts with skip = the largest exit of the
// failing ones (skip >= chunk end: the unit is empty).  A chunk with a deeper path takes the same descent inside the wave.  The table lives
// in the result object and is rebuilt by every batch, so nothing a rebuild, refit or flatten does to the tree can make it stale.
// Planes.  A unit's planes are wave-uniform: they are copied to LDS once per unit and read from there by broadcast — never indexed
// out of a per-lane array.
//
// Which array is walked: within.hip's rule.  The folded `trav` array for ordinary trees (a leaf entry carries the shape's own box), the
// UNFOLDED rule for uploaded FlatBvhs and single-shape trees (a leaf entry tests the shape's AABB out of the shape array), and an unfolded
// mirror of the FlatNode array (unfold.hpp) for a built tree with empty child bounds: below such a split the navigator boxes are
// Aabb::empty(), whose sums are -inf or NaN — never entered — while the folded entry would test the shape's box.
//
// Regions over an instance set (bvhgpu_instances_region_*) live here as well, beside region_unit, which they call
// unchanged: stage 1 is region_batch over the set's top level, stage 2 walks (pair, chunk) units with the planes re-expressed in the
// pair's object frame (k_instances_region_walk below).
#include <cstdio>
#include <type_traits>
#include <vector>

#include "instances.hpp"
#include "rows.hpp"
#include "unfold.hpp"
#include "walk.hpp"

namespace bvhgpu {

constexpr uint32_t REGION_ANC_MAX = 64;          // ancestors per chunk in the table: one gather step of a wave
// chunk rule (region_chunk_entries; DESIGN.md §4k: first guesses, not tuned)
constexpr uint32_t REGION_CHUNK_MIN = 1024;      // entries: 16 windows
constexpr uint32_t REGION_UNITS_TARGET = 8192;   // units a batch is cut into at least, while chunks stay above the minimum: 32 waves on each of 256 CUs
constexpr uint32_t REGION_GRID_MAX = 1u << 22;   // workgroups of a walk launch (more units than that: a workgroup takes several)

// entries per chunk: a multiple of 64, at least REGION_CHUNK_MIN, so that n regions give about REGION_UNITS_TARGET units.
// n x n_chunks < n + REGION_UNITS_TARGET whatever the tree's size.
static uint32_t region_chunk_entries(size_t n, uint32_t n_trav) {
    const size_t per_region = (REGION_UNITS_TARGET + n - 1) / n;   // chunks a region is cut into at most (n >= 1)
    size_t ce = ((size_t)n_trav + per_region - 1) / per_region;
    ce = (ce + 63) / 64 * 64;
    return (uint32_t)(ce < REGION_CHUNK_MIN ? REGION_CHUNK_MIN : ce);
}

// the plane-set test of one box; pl: the region's m planes in LDS.  CLASSIFY: `inside` = the opposite corner passes every plane as well
template <typename T, bool CLASSIFY>
__device__ __forceinline__ bool region_test(const T* pl, uint32_t m, const T lo[3], const T hi[3], bool& inside) {
    bool pass = true;
    inside = true;
    for (uint32_t j = 0; j < m; j++) {
        const T nn[3] = {pl[4 * j], pl[4 * j + 1], pl[4 * j + 2]};
        const T d = pl[4 * j + 3];
        T p[3];
        for (int k = 0; k < 3; k++) p[k] = nn[k] >= (T)0 ? hi[k] : lo[k];
        const T s = dot3<T>(nn, p) + d;
        pass = pass && s >= (T)0;
        if (CLASSIFY) {
            T o[3];
            for (int k = 0; k < 3; k++) o[k] = nn[k] >= (T)0 ? lo[k] : hi[k];
            const T so = dot3<T>(nn, o) + d;
            inside = inside && so >= (T)0;
        }
    }
    return pass;
}

__device__ __forceinline__ uint32_t region_wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// per chunk c the ancestors of its first entry s = c * chunk_entries: anc[c * REGION_ANC_MAX ..] and their count in cnt[c] (a count above
// REGION_ANC_MAX: the table holds the first REGION_ANC_MAX only and the walk descends itself).  A lane per chunk.
template <typename T>
__global__ __launch_bounds__(256) void k_region_ancestors(const TravNode<T>* __restrict__ nodes, uint32_t chunk_entries, uint32_t n_chunks,
                                                          uint32_t* __restrict__ cnt, uint32_t* __restrict__ anc) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const uint32_t s = c * chunk_entries;   // (< n_trav: the host cut the array into n_chunks)
    uint32_t i = 0, k = 0;
    while (i < s) {
        const uint32_t ex = nodes[i].exit;
        if (!trav_is_leaf(nodes[i].shape) && ex > s) {   // s is inside i's subtree
            if (k < REGION_ANC_MAX) anc[(size_t)c * REGION_ANC_MAX + k] = i;
            k++;
            i++;
        } else {
            i = ex > i ? ex : i + 1;   // (a valid array always has exit > i)
        }
    }
    cnt[c] = k;
}

// one (region, chunk) unit, by one wave.  FILL: the shapes go to shape_out[beg ..) (and their bytes to inside_out); returns the unit's count
template <typename T, bool UNFOLDED, bool FILL, bool CLASSIFY>
__device__ __forceinline__ uint32_t region_unit(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ shape_aabbs, const T* pl,
                                                uint32_t m, uint32_t c, uint32_t chunk_entries, const uint32_t* __restrict__ anc_cnt,
                                                const uint32_t* __restrict__ anc, uint32_t beg, uint32_t end, uint32_t* __restrict__ shape_out,
                                                unsigned char* __restrict__ inside_out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t s = c * chunk_entries;
    const uint32_t e = n_trav - s < chunk_entries ? n_trav : s + chunk_entries;
    // ---- chunk start: the failing ancestors of entry s
    uint32_t skip = s;
    const uint32_t na = anc_cnt[c];
    if (na <= REGION_ANC_MAX) {
        uint32_t ex = 0;
        if (lane < na) {
            const NodeRegs<T> nd = load_node(nodes + anc[(size_t)c * REGION_ANC_MAX + lane]);
            bool in;
            if (!region_test<T, false>(pl, m, nd.mn, nd.mx, in)) ex = nd.exit;
        }
        ex = region_wave_max(ex);
        skip = ex > skip ? ex : skip;
    } else {   // a path deeper than the table: k_region_ancestors' descent, every lane the same entry; the first failing ancestor has the largest exit
        uint32_t i = 0;
        while (i < s) {
            const NodeRegs<T> nd = load_node(nodes + i);
            if (!trav_is_leaf(nd.shape) && nd.exit > s) {
                bool in;
                if (!region_test<T, false>(pl, m, nd.mn, nd.mx, in)) { skip = nd.exit; break; }
                i++;
            } else {
                i = nd.exit > i ? nd.exit : i + 1;
            }
        }
    }
    skip = __builtin_amdgcn_readfirstlane(skip);
    // ---- the windows
    uint32_t base = 0;
    uint32_t i = skip;
    while (i < e) {
        const uint32_t idx = i + lane;   // (no wrap: a lane beyond e is not valid, and n_trav + 64 < 2^32)
        uint32_t ex = 0, shp = 0;
        bool report = false, in = false;
        if (idx < e) {
            const NodeRegs<T> nd = load_node(nodes + idx);
            const bool leaf = trav_is_leaf(nd.shape);
            T lo[3] = {nd.mn[0], nd.mn[1], nd.mn[2]}, hi[3] = {nd.mx[0], nd.mx[1], nd.mx[2]};
            if (UNFOLDED && leaf) {   // (a leaf entry of an unfolded array has no box of its own: the shape's)
                const T* sb = shape_aabbs + 6 * (size_t)nd.shape;
                for (int k = 0; k < 3; k++) { lo[k] = sb[k]; hi[k] = sb[3 + k]; }
            }
            const bool pass = region_test<T, FILL && CLASSIFY>(pl, m, lo, hi, in);
            if (!leaf && !pass) ex = nd.exit;
            report = leaf && pass;
            shp = nd.shape;
        }
        uint32_t incl = ex;
        if (__ballot(ex != 0) != 0ull) {   // inclusive prefix maximum over the window
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)lane >= d && o > incl) incl = o;
            }
        }
        uint32_t excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0;
        const uint32_t tot = __shfl(incl, 63);
        const uint32_t mine = excl > skip ? excl : skip;
        report = report && idx >= mine;
        const unsigned long long hit = __ballot(report);
        if (FILL && report) {
            const uint32_t pos = beg + base + (uint32_t)__popcll(hit & ((1ull << lane) - 1ull));
            if (pos < end) {   // (never false: this walk is the count pass's; a wave stays inside its own range whatever happens)
                shape_out[pos] = shp;
                if (CLASSIFY) inside_out[pos] = in ? 1 : 0;
            }
        }
        base += (uint32_t)__popcll(hit);
        skip = tot > skip ? tot : skip;
        const uint32_t next = e - i <= 64u ? e : i + 64u;
        i = skip > next ? skip : next;
        i = __builtin_amdgcn_readfirstlane(i);
    }
    return base;
}

// a workgroup is one wave and takes the units blockIdx.x, blockIdx.x + gridDim.x, ...; unit u = region u / n_chunks, chunk u % n_chunks.
// !FILL: out[u] = the unit's count.  FILL: out = the scanned counts (n_units + 1 words), the unit writes shape_out[out[u] .. out[u + 1])
template <typename T, bool UNFOLDED, bool FILL, bool CLASSIFY>
__global__ __launch_bounds__(64) void k_region_walk(const TravNode<T>* __restrict__ nodes, uint32_t n_trav, const T* __restrict__ shape_aabbs,
                                                    const T* __restrict__ planes, uint32_t m, uint32_t n_chunks, uint32_t chunk_entries, uint32_t n_units,
                                                    const uint32_t* __restrict__ anc_cnt, const uint32_t* __restrict__ anc, uint32_t* __restrict__ out,
                                                    uint32_t* __restrict__ shape_out, unsigned char* __restrict__ inside_out) {
    __shared__ T pl[4 * BVHGPU_REGION_MAX_PLANES];
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        uint32_t beg = 0, end = 0;
        if (FILL) {
            beg = out[u]; end = out[u + 1];
            if (beg == end) continue;   // (uniform over the workgroup: nothing to write)
        }
        const uint32_t q = u / n_chunks, c = u - q * n_chunks;
        __syncthreads();   // (the previous unit's planes are no longer read)
        for (uint32_t w = threadIdx.x; w < 4 * m; w += 64) pl[w] = planes[(size_t)q * 4 * m + w];
        __syncthreads();
        const uint32_t cnt = region_unit<T, UNFOLDED, FILL, CLASSIFY>(nodes, n_trav, shape_aabbs, pl, m, c, chunk_entries, anc_cnt, anc, beg, end,
                                                                       shape_out, inside_out);
        if (!FILL && threadIdx.x == 0) out[u] = cnt;
    }
}

// the caller's offsets: row q starts where its first unit starts; offsets[n] = the total (unit_offsets[n * n_chunks])
__global__ __launch_bounds__(256) void k_region_offsets(const uint32_t* __restrict__ unit_offsets, uint32_t n, uint32_t n_chunks, uint32_t* __restrict__ offsets) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) offsets[q] = unit_offsets[(size_t)q * n_chunks];
}

// ---- regions over an instance set (bvhgpu_instances_region_*; include/bvh_mi355x.h) -----------------------------------------
// Stage 1 is region_batch over the set's top level with the world planes: its rows are the (region, instance) pairs.  Stage 2 walks every
// pair's member with the planes re-expressed in the instance's object frame: the unit is (pair, chunk), unit u = pair u / nc_max, chunk
// u % nc_max, where nc_max is the largest chunk count among the members — a uniform stride, so the schedule is rows.hip's again with no
// further scan and no further host read; a unit whose chunk lies beyond its own member's array counts 0.
// MASKED (bvhgpu_instances_region_masked_*): region q carries a mask P[q] and I_q keeps the instances of stage 1's row whose mask
// shares a bit with it.  Stage 1 and the pairs are what they were; every unit of a hidden pair counts 0 — the wave learns (region, instance)
// first, one 4-byte load and one register, in front of the plane transform — so the pair has no rows and the fill, which is the unmasked
// fill walk, passes over its units by beg == end.  With
// INSTANCES_ONLY stage 1 runs into the set's own result object and the pairs are the units (stride 1): k_instances_region_visible counts 1 or
// 0, the same scan and offsets, and k_instances_region_keep writes the survivors with stage 1's inside byte.

// what the walk needs of a member, one record per member, made by every batch (instances.hip's InstTree is the ray walk's)
template <typename T> struct RegionMember {
    const TravNode<T>* nodes;   // the folded array, the uploaded array, or the unfolded mirror in the result object
    const T* aabbs;             // n x 6: the shapes' own boxes (read by the unfolded rule)
    uint32_t n_trav, unfolded;
    uint32_t chunk_entries, n_chunks;
    uint32_t anc_base;          // its first chunk in the batch's ancestor table
    uint32_t _pad;
};

// pair p belongs to the region q with top_offsets[q] <= p < top_offsets[q + 1] (stage 1's rows; empty rows repeat an offset)
__global__ __launch_bounds__(256) void k_instances_region_pairs(const uint32_t* __restrict__ top_offsets, uint32_t n, uint32_t n_pairs,
                                                                uint32_t* __restrict__ pair_region) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;   // (no wrap: the grid is ceil(n_pairs / 256) and n_pairs <= 2^32 - 1)
    if (p >= n_pairs) return;
    uint32_t lo = 0, hi = n;   // top_offsets[lo] <= p < top_offsets[hi] throughout (top_offsets[0] == 0, top_offsets[n] == n_pairs)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (top_offsets[mid] <= p) lo = mid; else hi = mid;
    }
    pair_region[p] = lo;
}

// a workgroup is one wave and takes the units blockIdx.x, blockIdx.x + gridDim.x, ...  The planes of the unit's region go to LDS in its
// instance's object frame (lane j < m: plane j; the header's formula, from the FORWARD transform); then region_unit, on the member's array.
// !FILL: out[u] = the unit's count.  FILL: out = the scanned counts; the unit writes shape_out and inst_out[out[u] .. out[u + 1])
template <typename T, bool FILL, bool CLASSIFY, bool MASKED = false>
__global__ __launch_bounds__(64) void k_instances_region_walk(const RegionMember<T>* __restrict__ members, const uint32_t* __restrict__ tree_of,
                                                              const T* __restrict__ xforms, const T* __restrict__ planes, uint32_t m,
                                                              const uint32_t* __restrict__ pair_region, const uint32_t* __restrict__ pair_inst,
                                                              uint32_t nc_max, size_t n_units, const uint32_t* __restrict__ anc_cnt,
                                                              const uint32_t* __restrict__ anc, uint32_t* __restrict__ out, uint32_t* __restrict__ inst_out,
                                                              uint32_t* __restrict__ shape_out, unsigned char* __restrict__ inside_out, InstMasks mk) {
    __shared__ T pl[4 * BVHGPU_REGION_MAX_PLANES];
    for (size_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        uint32_t beg = 0, end = 0;
        if (FILL) {
            beg = out[u]; end = out[u + 1];
            if (beg == end) continue;   // (uniform over the workgroup: nothing to write)
        }
        const uint32_t p = (uint32_t)(u / nc_max), c = (uint32_t)(u - (size_t)p * nc_max);
        const uint32_t q = __builtin_amdgcn_readfirstlane(pair_region[p]), inst = __builtin_amdgcn_readfirstlane(pair_inst[p]);
        static_assert(!(MASKED && FILL), "only the count walk looks at the masks: the fill passes over a hidden pair's units by beg == end");
        if constexpr (MASKED) {   // (uniform) a hidden pair: every unit of it counts 0
            const uint32_t pmask = mk.ray ? __builtin_amdgcn_readfirstlane(mk.ray[q]) : 0xFFFFFFFFu;
            if ((__builtin_amdgcn_readfirstlane(mk.inst[inst]) & pmask) == 0u) {
                if (threadIdx.x == 0) out[u] = 0;
                continue;
            }
        }
        const RegionMember<T>* mb = members + __builtin_amdgcn_readfirstlane(tree_of[inst]);
        const uint32_t nc = __builtin_amdgcn_readfirstlane(mb->n_chunks);
        if (c >= nc) {   // (uniform) the member's array ends in front of this chunk
            if (!FILL && threadIdx.x == 0) out[u] = 0;
            continue;
        }
        __syncthreads();   // (the previous unit's planes are no longer read)
        if (threadIdx.x < m) {
            const T* w = planes + ((size_t)q * m + threadIdx.x) * 4;
            const T* x = xforms + 12 * (size_t)inst;
            const T n0 = w[0], n1 = w[1], n2 = w[2], d = w[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const T a = x[j] * n0, b = x[4 + j] * n1, cc = x[8 + j] * n2;
                const T ab = a + b;
                pl[4 * threadIdx.x + j] = ab + cc;
            }
            const T a = n0 * x[3], b = n1 * x[7], cc = n2 * x[11];
            const T ab = a + b;
            const T abc = ab + cc;
            pl[4 * threadIdx.x + 3] = abc + d;
        }
        __syncthreads();
        const uint32_t n_trav = __builtin_amdgcn_readfirstlane(mb->n_trav), ce = __builtin_amdgcn_readfirstlane(mb->chunk_entries);
        const uint32_t ab0 = __builtin_amdgcn_readfirstlane(mb->anc_base);
        const uint32_t* ac = anc_cnt + ab0;
        const uint32_t* an = anc + (size_t)ab0 * REGION_ANC_MAX;
        uint32_t cnt;
        if (__builtin_amdgcn_readfirstlane(mb->unfolded) != 0u)   // (uniform: members of both rules meet in one launch)
            cnt = region_unit<T, true, FILL, CLASSIFY>(mb->nodes, n_trav, mb->aabbs, pl, m, c, ce, ac, an, beg, end, shape_out, inside_out);
        else
            cnt = region_unit<T, false, FILL, CLASSIFY>(mb->nodes, n_trav, mb->aabbs, pl, m, c, ce, ac, an, beg, end, shape_out, inside_out);
        if (!FILL && threadIdx.x == 0) out[u] = cnt;
        if (FILL)
            for (size_t k = (size_t)beg + threadIdx.x; k < end; k += 64) inst_out[k] = inst;   // the instance beside every shape of the unit
    }
}

// the caller's offsets: row q starts where the first unit of its first pair starts; offsets[n] = the total
__global__ __launch_bounds__(256) void k_instances_region_offsets(const uint32_t* __restrict__ unit_offsets, const uint32_t* __restrict__ top_offsets,
                                                                  uint32_t n, uint32_t nc_max, uint32_t* __restrict__ offsets) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) offsets[q] = unit_offsets[(size_t)top_offsets[q] * nc_max];
}

// MASKED with INSTANCES_ONLY: pair p (stage 1's row element p) is kept iff its instance is visible to its region
__global__ __launch_bounds__(256) void k_instances_region_visible(const uint32_t* __restrict__ pair_region, const uint32_t* __restrict__ pair_inst,
                                                                  uint32_t n_pairs, InstMasks mk, uint32_t* __restrict__ counts) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t pmask = mk.ray ? mk.ray[pair_region[p]] : 0xFFFFFFFFu;
    counts[p] = (mk.inst[pair_inst[p]] & pmask) != 0u ? 1u : 0u;
}
// ... and a kept pair goes to its place in the scanned counts, with stage 1's inside byte (top_inside: NULL without CLASSIFY)
__global__ __launch_bounds__(256) void k_instances_region_keep(const uint32_t* __restrict__ pair_offsets, const uint32_t* __restrict__ pair_inst,
                                                               const unsigned char* __restrict__ top_inside, uint32_t n_pairs, uint32_t total,
                                                               uint32_t* __restrict__ inst_out, unsigned char* __restrict__ inside_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t at = pair_offsets[p];
    if (pair_offsets[p + 1] == at || at >= total) return;   // (hidden; never beyond the total: the offsets are the scan of these counts)
    inst_out[at] = pair_inst[p];
    if (top_inside) inside_out[at] = top_inside[p];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool UNFOLDED>
static void region_launch(bvhgpu_tree* t, const TravNode<T>* nodes, uint32_t n_trav, const T* planes_dev, size_t n, uint32_t m, bool classify, bool count_only,
                          bvhgpu_hits* h) {
    hipStream_t st = t->ctx->stream;
    const T* aabbs = t->aabbs.as<T>();
    const uint32_t ce = region_chunk_entries(n, n_trav);
    const uint32_t nc = (uint32_t)(((size_t)n_trav + ce - 1) / ce);
    const size_t n_units = n * nc;   // (< n + REGION_UNITS_TARGET, and n < 2^32 - 1 with nc == 1 from n = REGION_UNITS_TARGET on)
    const uint32_t nu = (uint32_t)n_units;
    const dim3 grid((unsigned)(n_units < REGION_GRID_MAX ? n_units : REGION_GRID_MAX)), block(64);
    h->offsets.reserve((n_units + 1) * 4);
    h->rg_anc.reserve((size_t)nc * (1 + REGION_ANC_MAX) * 4);
    uint32_t* anc_cnt = h->rg_anc.as<uint32_t>();
    uint32_t* anc = anc_cnt + nc;
    hipLaunchKernelGGL((k_region_ancestors<T>), dim3((nc + 255) / 256), dim3(256), 0, st, nodes, ce, nc, anc_cnt, anc);
    uint32_t* counts = rows_begin(h, n_units, false);
    hipLaunchKernelGGL((k_region_walk<T, UNFOLDED, false, false>), grid, block, 0, st, nodes, n_trav, aabbs, planes_dev, m, nc, ce, nu, anc_cnt, anc, counts,
                       (uint32_t*)nullptr, (unsigned char*)nullptr);
    BVH_HIP(hipGetLastError());
    const RowsTotals rows = rows_scan(h, n_units, 0u, 0u);
    h->rg_chunks = nc; h->rg_chunk_entries = ce;   // (behind the scan: a batch that overflowed leaves an empty result)
    if (rows.total == 0) return;  // every row is empty (rg_offsets is all zero already)
    rows_offsets(h, n_units);
    uint32_t* unit_offsets = h->offsets.as<uint32_t>();
    hipLaunchKernelGGL(k_region_offsets, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, unit_offsets, (uint32_t)n, nc, h->rg_offsets.as<uint32_t>());
    if (!count_only) {
        h->indices.reserve((size_t)rows.total * 4);
        if (classify) h->rg_inside.reserve((size_t)rows.total);
        uint32_t* shape = h->indices.as<uint32_t>();
        if (classify) hipLaunchKernelGGL((k_region_walk<T, UNFOLDED, true, true>), grid, block, 0, st, nodes, n_trav, aabbs, planes_dev, m, nc, ce, nu, anc_cnt, anc,
                                         unit_offsets, shape, h->rg_inside.as<unsigned char>());
        else hipLaunchKernelGGL((k_region_walk<T, UNFOLDED, true, false>), grid, block, 0, st, nodes, n_trav, aabbs, planes_dev, m, nc, ce, nu, anc_cnt, anc,
                                unit_offsets, shape, (unsigned char*)nullptr);
    }
    BVH_HIP(hipGetLastError());
    h->total = rows.total;
}

template <typename T>
void region_batch(bvhgpu_tree* t, const T* planes_dev, size_t n, uint32_t m, unsigned flags, bvhgpu_hits* h) {
    bvhgpu_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const bool count_only = (flags & BVHGPU_REGION_COUNT_ONLY) != 0;
    const bool classify = (flags & BVHGPU_REGION_CLASSIFY) != 0 && !count_only;
    const bool mirror = t->exact_only && t->built && !t->unfolded && t->n >= 2;   // (see "Which array is walked" at the top)
    const bool unfolded = t->unfolded || t->n == 1 || mirror;   // a single-shape tree has one (leaf) entry and no navigator
    // the result object becomes an (empty) region result first: whatever fails below leaves it consistent
    rows_reset(h, ctx, Traits<T>::dtype, TRAVERSE_REGION, 0, count_only);
    h->rg_classify = classify; h->rg_chunks = 0; h->rg_chunk_entries = 0;
    char name[112];
    std::snprintf(name, sizeof name, "bvhgpu::k_region_walk<%s, %s, %s, %s>", walk_type_name<T>(), unfolded ? "true" : "false", count_only ? "false" : "true",
                  classify ? "true" : "false");
    h->walk_kernel = name;
    h->rg_offsets.reserve((n + 1) * 4);
    BVH_HIP(hipMemsetAsync(h->rg_offsets.p, 0, (n + 1) * 4, st));   // (no regions, an empty hierarchy, or a batch without a hit: every row is empty)
    if (n != 0 && t->n != 0) {
        ensure_flat_arrays(t);
        const TravNode<T>* nodes = t->trav.as<TravNode<T>>();
        uint32_t n_trav = (uint32_t)t->n_trav;
        if (mirror) {
            n_trav = (uint32_t)t->n_flat;
            h->unfold.reserve((size_t)n_trav * sizeof(TravNode<T>));
            hipLaunchKernelGGL((k_within_unfold<T>), dim3((n_trav + 255) / 256), dim3(256), 0, st, t->flat.as<typename Traits<T>::Flat>(), n_trav,
                               h->unfold.as<TravNode<T>>());
            BVH_HIP(hipGetLastError());
            nodes = h->unfold.as<TravNode<T>>();
        }
        if (unfolded) region_launch<T, true>(t, nodes, n_trav, planes_dev, n, m, classify, count_only, h);
        else region_launch<T, false>(t, nodes, n_trav, planes_dev, n, m, classify, count_only, h);
    }
    BVH_HIP(hipStreamSynchronize(st));   // the result is complete when the call returns
    h->n_rays = n;
    h->stats.hits = h->total;
}
template void region_batch<float>(bvhgpu_tree*, const float*, size_t, uint32_t, unsigned, bvhgpu_hits*);
template void region_batch<double>(bvhgpu_tree*, const double*, size_t, uint32_t, unsigned, bvhgpu_hits*);

// bvhgpu_instances_region_masked_* with BVHGPU_REGION_INSTANCES_ONLY: stage 1 into the set's own result object, then its pairs as units of one
// — count 1 or 0, the scan with its ONE host read, the offsets at stride 1, the survivors with stage 1's inside byte
template <typename T>
static void instances_region_only_masked(bvhgpu_instances* s, const T* planes_dev, size_t n, uint32_t m, bool classify, bool count_only, bvhgpu_hits* h,
                                         const uint32_t* region_mask_dev) {
    bvhgpu_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    rows_reset(h, ctx, Traits<T>::dtype, TRAVERSE_REGION, 0, count_only);
    h->rg_classify = classify; h->rg_chunks = 0; h->rg_chunk_entries = 0; h->rg_inst = REGION_INST_ONLY;
    h->walk_kernel = "bvhgpu::k_instances_region_visible";
    h->rg_offsets.reserve((n + 1) * 4);
    BVH_HIP(hipMemsetAsync(h->rg_offsets.p, 0, (n + 1) * 4, st));
    if (!s->rg_top) s->rg_top = new bvhgpu_hits();
    bvhgpu_hits* top = s->rg_top;
    region_batch<T>(s->top, planes_dev, n, m, classify ? BVHGPU_REGION_CLASSIFY : 0u, top);   // (synchronous: P is known behind it)
    const size_t P = (size_t)top->total;
    if (P != 0) {
        const InstMasks mk = {s->masks.as<uint32_t>(), region_mask_dev};
        const dim3 pgrid((unsigned)((P + 255) / 256)), block(256);
        h->offsets.reserve((P + 1) * 4);
        h->rg_pairs.reserve(P * 4);
        const uint32_t* top_offsets = top->rg_offsets.as<uint32_t>();
        const uint32_t* pair_inst = top->indices.as<uint32_t>();
        uint32_t* pair_region = h->rg_pairs.as<uint32_t>();
        hipLaunchKernelGGL(k_instances_region_pairs, pgrid, block, 0, st, top_offsets, (uint32_t)n, (uint32_t)P, pair_region);
        uint32_t* counts = rows_begin(h, P, false);
        hipLaunchKernelGGL(k_instances_region_visible, pgrid, block, 0, st, pair_region, pair_inst, (uint32_t)P, mk, counts);
        BVH_HIP(hipGetLastError());
        const RowsTotals rows = rows_scan(h, P, 0u, 0u);
        h->rg_chunks = top->rg_chunks; h->rg_chunk_entries = top->rg_chunk_entries;   // (how stage 1 cut the top level, as the unmasked form reports)
        if (rows.total != 0) {
            rows_offsets(h, P);
            uint32_t* pair_offsets = h->offsets.as<uint32_t>();
            hipLaunchKernelGGL(k_instances_region_offsets, dim3((unsigned)((n + 1 + 255) / 256)), block, 0, st, pair_offsets, top_offsets, (uint32_t)n, 1u,
                               h->rg_offsets.as<uint32_t>());
            if (!count_only) {
                h->indices.reserve((size_t)rows.total * 4);
                if (classify) h->rg_inside.reserve((size_t)rows.total);
                hipLaunchKernelGGL(k_instances_region_keep, pgrid, block, 0, st, pair_offsets, pair_inst,
                                   classify ? top->rg_inside.as<unsigned char>() : (const unsigned char*)nullptr, (uint32_t)P, (uint32_t)rows.total,
                                   h->indices.as<uint32_t>(), classify ? h->rg_inside.as<unsigned char>() : (unsigned char*)nullptr);
            }
            BVH_HIP(hipGetLastError());
            h->total = rows.total;
        }
    } else {
        h->rg_chunks = top->rg_chunks; h->rg_chunk_entries = top->rg_chunk_entries;
    }
    BVH_HIP(hipStreamSynchronize(st));   // the result is complete when the call returns
    h->n_rays = n;
    h->stats.hits = h->total;
}

// the regions of a batch over a committed instance set (the caller has checked commit, staleness and the members' kinds)
// masked: bvhgpu_instances_region_masked_* — the set's masks against region_mask_dev (NULL: all ones); otherwise region_mask_dev is not looked at
template <typename T>
void instances_region_batch(bvhgpu_instances* s, const T* planes_dev, size_t n, uint32_t m, unsigned flags, bvhgpu_hits* h, bool masked,
                            const uint32_t* region_mask_dev) {
    bvhgpu_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const bool count_only = (flags & BVHGPU_REGION_COUNT_ONLY) != 0;
    const bool classify = (flags & BVHGPU_REGION_CLASSIFY) != 0 && !count_only;
    if (masked && (flags & BVHGPU_REGION_INSTANCES_ONLY)) {
        instances_region_only_masked<T>(s, planes_dev, n, m, classify, count_only, h, region_mask_dev);
        return;
    }
    if (flags & BVHGPU_REGION_INSTANCES_ONLY) {   // stage 1 IS the answer: the top level's rows, straight into the caller's result object
        try {
            region_batch<T>(s->top, planes_dev, n, m, flags & (BVHGPU_REGION_COUNT_ONLY | BVHGPU_REGION_CLASSIFY), h);
        } catch (...) {   // (the empty result it leaves is this entry's as well)
            h->rg_inst = REGION_INST_ONLY;
            throw;
        }
        h->rg_inst = REGION_INST_ONLY;
        return;
    }
    // the result object becomes an (empty) instance-region result first: whatever fails below leaves it consistent
    rows_reset(h, ctx, Traits<T>::dtype, TRAVERSE_REGION, 0, count_only);
    h->rg_classify = classify; h->rg_chunks = 0; h->rg_chunk_entries = 0; h->rg_inst = REGION_INST_SHAPES;
    char name[112];
    // (the unmasked names are what they were; a masked batch names its count walk, the one launch that looks at the masks)
    if (masked) std::snprintf(name, sizeof name, "bvhgpu::k_instances_region_walk<%s, false, false, true>", walk_type_name<T>());
    else std::snprintf(name, sizeof name, "bvhgpu::k_instances_region_walk<%s, %s, %s>", walk_type_name<T>(), count_only ? "false" : "true", classify ? "true" : "false");
    h->walk_kernel = name;
    h->rg_offsets.reserve((n + 1) * 4);
    BVH_HIP(hipMemsetAsync(h->rg_offsets.p, 0, (n + 1) * 4, st));
    // ---- stage 1, into the set's own result object (rows_reset clears the one it is given); synchronous, so P is known behind it
    if (!s->rg_top) s->rg_top = new bvhgpu_hits();
    bvhgpu_hits* top = s->rg_top;
    region_batch<T>(s->top, planes_dev, n, m, 0u, top);
    const size_t P = (size_t)top->total;   // (<= 2^32 - 1: region_batch throws Fail::Overflow beyond)
    const size_t nt = s->trees.size();
    // ---- the member table: which array, how it is cut for P pairs, where its ancestor rows and its mirror start
    std::vector<RegionMember<T>> tbl(nt);
    std::vector<size_t> mirror_at(nt, (size_t)-1);
    size_t n_anc = 0, n_mirror = 0;
    uint32_t nc_max = 0, ce_max = 0;
    for (size_t k = 0; k < nt && P != 0; k++) {
        bvhgpu_tree* t = s->trees[k];
        RegionMember<T>& r = tbl[k];
        r = RegionMember<T>{nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u};
        if (t->n == 0) continue;   // (no instance of it has a finite world box: never looked up)
        ensure_flat_arrays(t);
        const bool mirror = t->exact_only && t->built && !t->unfolded && t->n >= 2;   // region_batch's rule, member by member
        r.unfolded = (t->unfolded || t->n == 1 || mirror) ? 1u : 0u;
        r.n_trav = (uint32_t)(mirror ? t->n_flat : t->n_trav);
        r.nodes = t->trav.as<TravNode<T>>();
        r.aabbs = t->aabbs.as<T>();
        if (mirror) { mirror_at[k] = n_mirror; n_mirror += r.n_trav; }
        r.chunk_entries = region_chunk_entries(P, r.n_trav);
        r.n_chunks = (uint32_t)(((size_t)r.n_trav + r.chunk_entries - 1) / r.chunk_entries);
        if (n_anc + r.n_chunks > 0xFFFFFFFFull) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::Overflow};
        r.anc_base = (uint32_t)n_anc;
        n_anc += r.n_chunks;
        nc_max = r.n_chunks > nc_max ? r.n_chunks : nc_max;
        ce_max = r.chunk_entries > ce_max ? r.chunk_entries : ce_max;
    }
    if (P != 0 && nc_max != 0) {
        const size_t n_units = P * nc_max;   // (< P + REGION_UNITS_TARGET, and nc_max == 1 from P = REGION_UNITS_TARGET on: <= 2^32 - 1)
        const dim3 grid((unsigned)(n_units < REGION_GRID_MAX ? n_units : REGION_GRID_MAX)), block(64);
        h->offsets.reserve((n_units + 1) * 4);
        h->rg_anc.reserve(n_anc * (1 + REGION_ANC_MAX) * 4);
        h->rg_pairs.reserve(P * 4);
        h->rg_members.reserve(nt * sizeof(RegionMember<T>));
        if (n_mirror) h->unfold.reserve(n_mirror * sizeof(TravNode<T>));
        uint32_t* anc_cnt = h->rg_anc.as<uint32_t>();
        uint32_t* anc = anc_cnt + n_anc;
        for (size_t k = 0; k < nt; k++) {
            RegionMember<T>& r = tbl[k];
            if (r.n_chunks == 0) continue;
            if (mirror_at[k] != (size_t)-1) {
                TravNode<T>* dst = h->unfold.as<TravNode<T>>() + mirror_at[k];
                hipLaunchKernelGGL((k_within_unfold<T>), dim3((r.n_trav + 255) / 256), dim3(256), 0, st, s->trees[k]->flat.as<typename Traits<T>::Flat>(), r.n_trav, dst);
                r.nodes = dst;
            }
            hipLaunchKernelGGL((k_region_ancestors<T>), dim3((r.n_chunks + 255) / 256), dim3(256), 0, st, r.nodes, r.chunk_entries, r.n_chunks,
                               anc_cnt + r.anc_base, anc + (size_t)r.anc_base * REGION_ANC_MAX);
        }
        BVH_HIP(hipGetLastError());
        h->rg_members_host.assign(reinterpret_cast<const unsigned char*>(tbl.data()), reinterpret_cast<const unsigned char*>(tbl.data() + nt));
        BVH_HIP(hipMemcpyAsync(h->rg_members.p, h->rg_members_host.data(), nt * sizeof(RegionMember<T>), hipMemcpyHostToDevice, st));
        const uint32_t* top_offsets = top->rg_offsets.as<uint32_t>();
        const uint32_t* pair_inst = top->indices.as<uint32_t>();
        uint32_t* pair_region = h->rg_pairs.as<uint32_t>();
        hipLaunchKernelGGL(k_instances_region_pairs, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, top_offsets, (uint32_t)n, (uint32_t)P, pair_region);
        const RegionMember<T>* members = h->rg_members.as<RegionMember<T>>();
        const uint32_t* tree_of = s->tree_of.as<uint32_t>();
        const T* xforms = s->xforms.as<T>();
        uint32_t* counts = rows_begin(h, n_units, false);
        const InstMasks mk = {masked ? s->masks.as<uint32_t>() : nullptr, masked ? region_mask_dev : nullptr};
        // one launch of the walk: FILL, CLASSIFY and MASKED as types
        auto walk = [&](auto FILL, auto CLASSIFY, auto MASKED, uint32_t* out, uint32_t* inst_out, uint32_t* shape_out, unsigned char* inside_out) {
            hipLaunchKernelGGL((k_instances_region_walk<T, decltype(FILL)::value, decltype(CLASSIFY)::value, decltype(MASKED)::value>), grid, block, 0, st, members,
                               tree_of, xforms, planes_dev, m, pair_region, pair_inst, nc_max, n_units, anc_cnt, anc, out, inst_out, shape_out, inside_out, mk);
        };
        using Yes = std::true_type;
        using No = std::false_type;
        if (masked) walk(No{}, No{}, Yes{}, counts, nullptr, nullptr, nullptr);
        else walk(No{}, No{}, No{}, counts, nullptr, nullptr, nullptr);
        BVH_HIP(hipGetLastError());
        const RowsTotals rows = rows_scan(h, n_units, 0u, 0u);
        h->rg_chunks = nc_max; h->rg_chunk_entries = ce_max;   // (behind the scan: a batch that overflowed leaves an empty result)
        if (rows.total != 0) {
            rows_offsets(h, n_units);
            uint32_t* unit_offsets = h->offsets.as<uint32_t>();
            hipLaunchKernelGGL(k_instances_region_offsets, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, unit_offsets, top_offsets, (uint32_t)n, nc_max,
                               h->rg_offsets.as<uint32_t>());
            if (!count_only) {
                h->indices.reserve((size_t)rows.total * 4);
                h->row_instance.reserve((size_t)rows.total * 4);
                if (classify) h->rg_inside.reserve((size_t)rows.total);
                uint32_t* shape = h->indices.as<uint32_t>();
                uint32_t* inst = h->row_instance.as<uint32_t>();
                unsigned char* inside = classify ? h->rg_inside.as<unsigned char>() : nullptr;
                // (masked too: every unit of a hidden pair has beg == end and is passed over before anything of it is read — no mask needed)
                if (classify) walk(Yes{}, Yes{}, No{}, unit_offsets, inst, shape, inside);
                else walk(Yes{}, No{}, No{}, unit_offsets, inst, shape, inside);
            }
            BVH_HIP(hipGetLastError());
            h->total = rows.total;
        }
    }
    BVH_HIP(hipStreamSynchronize(st));   // the result is complete when the call returns
    h->n_rays = n;
    h->stats.hits = h->total;
}
template void instances_region_batch<float>(bvhgpu_instances*, const float*, size_t, uint32_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);
template void instances_region_batch<double>(bvhgpu_instances*, const double*, size_t, uint32_t, unsigned, bvhgpu_hits*, bool, const uint32_t*);

}  // namespace bvhgpu
