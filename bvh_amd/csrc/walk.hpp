// walk.hpp — what every walk kernel over the engine's traversal arrays shares (walk_binary.hip, walk_ordered.hip, walk_wide.hip and
// query.hip's walks use the same pool records, chunking and per-lane bookkeeping): output modes, node fetch, hit records, WalkOut,
// Ray::intersects_triangle, the per-lane ray state, the hit pool's per-wave chunks and the walk epilogue; and what traverse_enqueue
// (traverse.hip) calls in those files and in csr.hip: one launcher per file, which picks its kernel instantiation itself.
#pragma once

#include "engine.hpp"

namespace bvhgpu {

constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;   // rays per workgroup of the count scan
constexpr uint32_t SCAN_FUSED_MAX_BLOCKS = 2048;   // up to this many blocks every block sums its predecessors itself
constexpr int COUNT_PLAIN = 0, COUNT_PAIR = 1, COUNT_MASKED = 2;   // how a ray's count is stored (csr.hip ray_count)
constexpr uint32_t WIDE_ITEM_BITS = 5;                 // wide walk: item = ray << 5 | j (the pool records of a batch cut into items carry it)
constexpr uint32_t WIDE_BSUM_MAX = 128;                // wide walk: 64-ray blocks per workgroup up to which the walk keeps the scan's block sums
constexpr size_t WIDE_ITEM_MAX_RAYS = (size_t)1 << 27; // wide walk: item = ray << 5 | j is a 32-bit word
constexpr unsigned long long WALK_FLAG_GUIDE_RANGE = 16ull;   // ctr[7] bit: a ray was outside the guide walk's range — the host replays in f64
constexpr uint32_t HEAP_OVERFLOW_BIT = 2u;             // ctr[7] bit: a lane's best-first heap outgrew its workspace (k_traverse_heap)

// what a walk produces besides the CSR of shape indices
enum : int {
    MODE_INDICES = 0,   // Vec<&Shape> only
    MODE_T_SLICE = 1,   // + Ray::intersection_slice_for_aabb per hit (2 scalars)
    MODE_TRIANGLES = 2, // + Ray::intersects_triangle per hit: Intersection{distance,u,v} (3 scalars)
    MODE_CLOSEST = 3,   // no CSR: per ray the candidate triangle with the smallest distance
    MODE_ANY = 4,       // no CSR: per ray the FIRST candidate (reference order) whose triangle distance is < the ray's tmax; the walk stops there
    MODE_BOX_CLOSEST = 5,   // no CSR, no triangles: per ray the shape of its list whose own AABB the ray enters first (t-slice {enter, exit}) with enter < tmax
    MODE_BOX_FIRST = 6,     // ... the FIRST shape of its list (reference order) with enter < tmax; the walk stops there
    MODE_SPHERE_CLOSEST = 7,   // no CSR, no triangles: per ray the shape of its list whose sphere (WalkOut::sphere) the ray hits nearest ({distance, exit}) with distance < tmax
    MODE_SPHERE_FIRST = 8      // ... the FIRST shape of its list (reference order) whose sphere the ray hits with distance < tmax; the walk stops there
};
// what the output modes share (the per-ray modes are MODE >= MODE_CLOSEST, the CSR modes MODE < MODE_CLOSEST)
constexpr bool mode_tris(int m) { return m >= MODE_TRIANGLES && m <= MODE_ANY; }          // the leaf stage is Ray::intersects_triangle: needs the direction and w.tris
constexpr bool mode_box(int m) { return m == MODE_BOX_CLOSEST || m == MODE_BOX_FIRST; }   // the leaf stage is the t-slice of the shape's own AABB
constexpr bool mode_sphere(int m) { return m == MODE_SPHERE_CLOSEST || m == MODE_SPHERE_FIRST; }   // the leaf stage is ray_sphere on the shape's sphere: needs the direction
constexpr bool mode_first(int m) { return m == MODE_ANY || m == MODE_BOX_FIRST || m == MODE_SPHERE_FIRST; }   // the ray ends at its first candidate
constexpr bool mode_tmax(int m) { return m == MODE_ANY || mode_box(m) || mode_sphere(m); }   // candidates are limited by the ray's tmax
constexpr bool mode_pair(int m) { return mode_box(m) || mode_sphere(m); }                 // the per-ray record is 2 scalars ({enter, exit} / {distance, exit}), not an Intersection
template <int MODE> struct ModeVals { static constexpr int N = MODE == MODE_T_SLICE ? 2 : (MODE == MODE_TRIANGLES ? 3 : 0); };

// ---- node fetch: two (f32) / four (f64) 16-byte loads per lane -------------------------------
template <typename T> struct NodeRegs { T mn[3], mx[3]; uint32_t exit, shape; };

__device__ __forceinline__ NodeRegs<float> load_node(const TravNode<float>* p) {
    const float4* q = reinterpret_cast<const float4*>(p);
    float4 a = q[0], b = q[1];
    NodeRegs<float> r;
    r.mn[0] = a.x; r.mn[1] = a.y; r.mn[2] = a.z; r.exit = __float_as_uint(a.w);
    r.mx[0] = b.x; r.mx[1] = b.y; r.mx[2] = b.z; r.shape = __float_as_uint(b.w);
    return r;
}
__device__ __forceinline__ NodeRegs<double> load_node(const TravNode<double>* p) {
    const double2* q = reinterpret_cast<const double2*>(p);
    double2 a = q[0], b = q[1], c = q[2], d = q[3];
    NodeRegs<double> r;
    r.mn[0] = a.x; r.mn[1] = a.y; r.mn[2] = b.x;
    r.mx[0] = b.y; r.mx[1] = c.x; r.mx[2] = c.y;
    unsigned long long es = (unsigned long long)__double_as_longlong(d.x);
    r.exit = (uint32_t)(es & 0xFFFFFFFFull);
    r.shape = (uint32_t)(es >> 32);
    return r;
}

struct HitRec { uint32_t ray, k, shape; };

// everything a walk kernel writes
template <typename T> struct WalkOut {
    uint32_t* counts;            // per ray: number of shapes returned
    HitRec* pool;                // hit records in arrival order
    T* pool_v;                   // ModeVals::N scalars per record
    unsigned long long pool_cap;
    unsigned long long* ctr;     // [0] pool slots taken [1] device steps [2] leaf-entry steps [4] wave steps [5] candidates (closest mode)
    const T* tris;               // the leaf primitives.  Triangle modes: n x 9 vertices.  Box modes: the n x 6 shape AABBs, read through box().  Sphere modes:
                                 // the n x 4 spheres {cx, cy, cz, r}, read through sphere() — one pointer for all, so that the kernel arguments of the
                                 // existing instantiations stay as they are
    T* closest;                  // per ray {distance,u,v} (closest mode); box modes: per ray {enter, exit}, sphere modes: {distance, exit} — 2 scalars
    uint32_t* closest_prim;      // per ray shape index or NONE
    unsigned long long* closest_key;   // closest mode with rays cut into items (f32): per ray min over its items of {key(distance) << 32 | item << 28 | shape}
                                 // (kept all-ones between batches; k_closest_resolve turns the winner into closest / closest_prim).  NULL: one lane owns the ray
    uint32_t* item_cnt;          // wide walk with several items per ray: hits of item (ray, j), written only when non-zero
    uint32_t* ray_items;         // ... and per ray the set of j that wrote one (kept all-zero between batches like counts)
    uint32_t* scan_sums;         // wide walk: hits per SCAN_BLOCK rays, added up by the workgroups as they finish (a zeroed set; NULL: k_scan_reduce does the sums)
    uint4* pool_pair;            // wide walk, whole rays, indices only: pair records {ray, k, shape, shape | NONE} (report_pair) in the pool's memory instead of the 12-byte
                                 // HitRec: 8 bytes per hit, one offset gather per two hits in the scatter.  NULL: HitRec
    uint32_t* raybuf;            // wide walk, whole rays, indices only: the first 2^stage_shift shapes of ray r go straight to raybuf[r << stage_shift | k]
    uint32_t stage_shift;        // (4 bytes per hit, no record, no atomic); only later hits of a ray become pool records.  NULL: everything through the pool
    const T* tmax;               // any-hit, box and sphere modes: per ray the end of its segment (NULL: +inf for every ray)
    uint32_t* any_key;           // any-hit mode with rays cut into items: per ray min over its items that found a candidate of {item << 28 | shape}
                                 // (kept all-ones between batches; k_any_resolve turns the winner into closest / closest_prim).  NULL: one lane owns the ray
    // box modes: shape s's own AABB {min xyz, max xyz} (the wide walk's leaf stage)
    __host__ __device__ __forceinline__ const T* box(uint32_t s) const { return tris + 6 * (size_t)s; }
    __host__ __device__ __forceinline__ void set_boxes(const T* aabbs) { tris = aabbs; }
    // sphere modes: shape s's sphere {cx, cy, cz, r} (16-byte aligned: bvhgpu_tree::spheres is an allocation of its own)
    __host__ __device__ __forceinline__ const T* sphere(uint32_t s) const { return tris + 4 * (size_t)s; }
    __host__ __device__ __forceinline__ void set_spheres(const T* spheres) { tris = spheres; }
};

// ---- Ray::intersects_triangle (ray_impl.rs:154-213), Möller–Trumbore with back-face culling.  Same
//      sequence of IEEE operations as the reference: nalgebra cross = (ay*bz - az*by, az*bx - ax*bz,
//      ax*by - ay*bx), dot = (a0*b0 + a1*b1) + a2*b2, no contraction.  Returns the Intersection fields.
template <typename T> __device__ __forceinline__ void cross3(const T a[3], const T b[3], T out[3]) {
    T p0 = a[1] * b[2], q0 = a[2] * b[1];
    T p1 = a[2] * b[0], q1 = a[0] * b[2];
    T p2 = a[0] * b[1], q2 = a[1] * b[0];
    out[0] = p0 - q0; out[1] = p1 - q1; out[2] = p2 - q2;
}
template <typename T> __device__ __forceinline__ T dot3(const T a[3], const T b[3]) {
    T x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    T s = x + y;
    return s + z;
}
template <typename T>
__device__ __forceinline__ void ray_triangle(const T o[3], const T d[3], const T* __restrict__ tri, T out[3]) {
    const T a[3] = {tri[0], tri[1], tri[2]};
    T ab[3], ac[3], uvec[3], ao[3], vvec[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ab[k] = tri[3 + k] - a[k]; ac[k] = tri[6 + k] - a[k]; }   // :170-171
    cross3<T>(d, ac, uvec);                                                                  // :176
    const T det = dot3<T>(ab, uvec);                                                         // :181
    out[0] = Traits<T>::inf(); out[1] = 0; out[2] = 0;
    if (det < Traits<T>::eps()) return;                                                      // :186-188
    const T inv_det = (T)1 / det;                                                            // :190
#pragma unroll
    for (int k = 0; k < 3; k++) ao[k] = o[k] - a[k];                                         // :193
    const T u = dot3<T>(ao, uvec) * inv_det;                                                 // :196
    out[1] = u;
    if (!(u >= (T)0 && u <= (T)1)) return;                                                   // :199-201
    cross3<T>(ao, ab, vvec);                                                                 // :204
    const T v = dot3<T>(d, vvec) * inv_det;                                                  // :207
    out[2] = v;
    if (v < (T)0 || u + v > (T)1) return;                                                    // :209-211
    const T dist = dot3<T>(ac, vvec) * inv_det;                                              // :213
    if (dist > Traits<T>::eps()) out[0] = dist;                                              // :215-219
}

// ---- the leaf stage of the sphere modes (include/bvh_mi355x.h, bvhgpu_traverse_sphere_*): the geometric form — the ray's point nearest the
//      centre, then the half chord — because b*b - a*c loses r*r against |o - c|^2 in f32 for distant origins.  Every operation is rounded once
//      in T, dot3 as above, no contraction.  out = {distance, exit}; a miss is {+inf, 0}.  Nothing is special-cased: a NaN centre, radius or
//      direction and a zero direction (a = 0: tc is NaN or inf, l is NaN) fail disc >= 0; r < 0 enters squared; an origin inside the sphere has
//      t0 <= eps and hits at t1.  `sphere` is 16-byte aligned: one 16-byte load (f32), two (f64).
__device__ __forceinline__ void load_sphere(const float* __restrict__ p, float s[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
}
__device__ __forceinline__ void load_sphere(const double* __restrict__ p, double s[4]) {
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y;
}
template <typename T>
__device__ __forceinline__ void ray_sphere(const T o[3], const T d[3], const T* __restrict__ sphere, T out[2]) {
    T s[4], f[3], l[3];
    load_sphere(sphere, s);
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = o[k] - s[k];
    const T a = dot3<T>(d, d);
    const T tc = (-dot3<T>(f, d)) / a;                 // parameter of the ray's point nearest the centre
#pragma unroll
    for (int k = 0; k < 3; k++) { const T td = tc * d[k]; l[k] = f[k] + td; }   // centre → that point
    const T rr = s[3] * s[3];
    const T disc = rr - dot3<T>(l, l);
    out[0] = Traits<T>::inf(); out[1] = 0;
    if (!(disc >= (T)0)) return;
    const T h = sqrt(disc / a);
    const T t0 = tc - h, t1 = tc + h;
    const T t = t0 > Traits<T>::eps() ? t0 : t1;
    if (t > Traits<T>::eps()) { out[0] = t; out[1] = t1; }
}

// ---- the leaf stage of the row queries: the record of shape s for the ray, whose first scalar is its DISTANCE.  prims is t->aabbs
//      (n x 6), t->tris (n x 9) or t->spheres (n x 4) by LEAF; W scalars of out[] make the record.  allhits.hip uses it; khits.hip still
//      carries its own copy (khits_record, KH_*), the same text, which is to be replaced by this one.
enum : int { LEAF_BOX = BVHGPU_LEAF_BOX, LEAF_TRIANGLE = BVHGPU_LEAF_TRIANGLE, LEAF_SPHERE = BVHGPU_LEAF_SPHERE };
template <int LEAF> struct LeafVals { static constexpr uint32_t W = LEAF == LEAF_TRIANGLE ? 3u : 2u; };
template <typename T, int LEAF>
__device__ __forceinline__ void leaf_record(const T o[3], const T d[3], const T inv[3], const T* __restrict__ prims, uint32_t s, T out[3]) {
    out[2] = 0;
    if (LEAF == LEAF_TRIANGLE) {
        ray_triangle<T>(o, d, prims + 9 * (size_t)s, out);
    } else if (LEAF == LEAF_SPHERE) {
        ray_sphere<T>(o, d, prims + 4 * (size_t)s, out);
    } else {
        const T* b = prims + 6 * (size_t)s;
        const T mn[3] = {b[0], b[1], b[2]}, mx[3] = {b[3], b[4], b[5]};
        T t0, t1;
        const bool hit = slab_hit<T>(o, inv, mn, mx, t0, t1);
        out[0] = hit ? t0 : Traits<T>::inf(); out[1] = hit ? t1 : (T)0;
    }
}

// ---- the per-lane top-k lists in LDS (knn.hip, knn_tree.hip; khits.hip still restates the rule as khits_block): k slots of (T key, u32
//      shape) per lane.  Block size: the largest of 256 / 128 / 64 lanes whose lists fit 32 KB, so that several workgroups share a CU's
//      LDS; 64 lanes above that (k = 64 in f64: 48 KB, inside the 64 KB a workgroup gets without attributes — topk_fits checks a family's
//      largest k)
template <typename T> inline unsigned topk_block(uint32_t k) {
    const size_t per_lane = (size_t)k * (sizeof(T) + 4);
    if (256 * per_lane <= 32 * 1024) return 256;
    if (128 * per_lane <= 32 * 1024) return 128;
    return 64;
}
constexpr bool topk_fits(uint32_t max_k) { return max_k * 64u * (sizeof(double) + 4u) <= 64u * 1024u; }   // the lists of 64 lanes fit a workgroup's LDS

// ---- per-lane ray state
template <typename T, int MODE> struct LaneRay {
    T o[3], inv[3];
    T d[mode_tris(MODE) || mode_sphere(MODE) ? 3 : 1];   // direction: only the triangle and sphere stages need it
    T best[MODE >= MODE_CLOSEST ? 3 : 1];  // closest Intersection so far / the any-hit candidate / box modes: {enter, exit}, sphere modes: {distance, exit} of the candidate
    T tmax;                                // any-hit, box and sphere modes: end of the segment
    uint32_t best_prim;
    uint32_t r, cnt;
    bool fin;                              // all components finite → NaN-free slab test is exact
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = 0; inv[k] = 0; }
        d[0] = 0; best[0] = 0; tmax = 0; best_prim = NONE; r = NONE; cnt = 0; fin = true;
    }
    // tmaxs: WalkOut::tmax (any-hit, box and sphere modes only)
    __device__ __forceinline__ void load(const typename Traits<T>::Ray* __restrict__ rays, uint32_t ray, const T* __restrict__ tmaxs = nullptr) {
        const typename Traits<T>::Ray* rp = rays + ray;
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = rp->o[k]; inv[k] = rp->inv[k]; }
        if (mode_tris(MODE) || mode_sphere(MODE)) {
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = rp->d[k];
        }
        if (MODE >= MODE_CLOSEST) { best[0] = Traits<T>::inf(); best[1] = 0; best[2] = 0; }
        if (mode_tmax(MODE)) tmax = tmaxs ? tmaxs[ray] : Traits<T>::inf();
        best_prim = NONE; r = ray; cnt = 0;
        fin = ray_is_finite<T>(o, inv);
    }
    // o / inv were filled by the caller (the guide walk's f32 view of an f64 ray): the rest of load()
    __device__ __forceinline__ void loaded(uint32_t ray) {
        best_prim = NONE; r = ray; cnt = 0;
        fin = ray_is_finite<T>(o, inv);
    }
    // the ray has left the tree: its Vec / closest hit is complete
    __device__ __forceinline__ void retire(const WalkOut<T>& w) {
        if (mode_pair(MODE)) {
            w.closest[2 * (size_t)r] = best[0]; w.closest[2 * (size_t)r + 1] = best[1];
            w.closest_prim[r] = best_prim;
        } else if (MODE >= MODE_CLOSEST) {
            w.closest[3 * (size_t)r] = best[0]; w.closest[3 * (size_t)r + 1] = best[1]; w.closest[3 * (size_t)r + 2] = best[2];
            w.closest_prim[r] = best_prim;
        } else {
            w.counts[r] = cnt;
        }
        r = NONE;
    }
};

// Hit records go to the pool in per-wave chunks: one global atomic per chunk instead of one per wave-step with
// a hit.  One address sustains only ≈88 atomics/µs on this chip, and a hit-heavy scene (58 M hits from 10 M
// primary rays on the stand-in atrium) made the walk 8x slower with fixed 64-record chunks; a wave's chunk size
// therefore doubles with every chunk it fills (64 → 8192), which bounds the slack by the records written.
constexpr uint32_t POOL_CHUNK_MIN = 64;     // >= 64: one wave-step reports at most 64 hits
constexpr uint32_t POOL_CHUNK_MAX = 8192;
// wave-uniform cursor into this wave's current chunk of the hit pool
struct PoolCursor { unsigned long long pos = 0; uint32_t left = 0; uint32_t next = POOL_CHUNK_MIN; };

// mark the unused tail of a wave's chunk so that k_hits_scatter skips it
__device__ __forceinline__ void pool_invalidate_tail(HitRec* pool, unsigned long long pool_cap, const PoolCursor& pc, int lane) {
    for (uint32_t j = (uint32_t)lane; j < pc.left; j += WAVE)
        if (pc.pos + j < pool_cap) pool[pc.pos + j].ray = NONE;
}

// A leaf box was hit (rec) in some lanes of the wave: do what the MODE asks for with the shape.
// t0 / t1: the box's t-slice (slab_hit's outputs) where the MODE returns or compares it (T_SLICE and the box modes).
template <typename T, int MODE>
__device__ __forceinline__ void report(bool rec, uint32_t shape, T t0, T t1, LaneRay<T, MODE>& ray, const WalkOut<T>& w,
                                       PoolCursor& pc, int lane, unsigned long long lt) {
    const unsigned long long m = __ballot(rec);
    if (!m) return;
    T vals[3] = {t0, t1, 0};
    if (mode_tris(MODE) && rec) ray_triangle<T>(ray.o, ray.d, w.tris + 9 * (size_t)shape, vals);
    if (MODE == MODE_CLOSEST) {
        if (rec) {
            if (vals[0] < ray.best[0]) { ray.best[0] = vals[0]; ray.best[1] = vals[1]; ray.best[2] = vals[2]; ray.best_prim = shape; }
            ray.cnt++;
        }
        return;
    }
    if (MODE == MODE_ANY) {   // the first candidate inside the segment ends the ray (the walk sees best_prim != NONE and empties the lane)
        if (rec && vals[0] < ray.tmax) { ray.best[0] = vals[0]; ray.best[1] = vals[1]; ray.best[2] = vals[2]; ray.best_prim = shape; }
        return;
    }
    if (mode_box(MODE)) {
        // a candidate enters its box before the segment ends (strict, in T: a NaN, zero or negative tmax admits nothing).  Closest: strictly
        // nearer than the lane's best so far, so that on equal entries the first of the list stays; first: it ends the ray like MODE_ANY
        if (rec && t0 < ray.tmax && (MODE == MODE_BOX_FIRST || t0 < ray.best[0])) { ray.best[0] = t0; ray.best[1] = t1; ray.best_prim = shape; }
        return;
    }
    if (mode_sphere(MODE)) {
        // the same rule on ray_sphere's distance: a miss is +inf, which is below no tmax (NULL tmax: +inf) — strict, so ties keep the first
        if (rec) {
            T hit[2];
            ray_sphere<T>(ray.o, ray.d, w.sphere(shape), hit);
            if (hit[0] < ray.tmax && (MODE == MODE_SPHERE_FIRST || hit[0] < ray.best[0])) { ray.best[0] = hit[0]; ray.best[1] = hit[1]; ray.best_prim = shape; }
        }
        return;
    }
    constexpr int NV = ModeVals<MODE>::N;
    const uint32_t h = (uint32_t)__popcll(m);
    if (h > pc.left) {   // wave-uniform: start a new chunk, invalidate what is left of the old one
        pool_invalidate_tail(w.pool, w.pool_cap, pc, lane);
        unsigned int blo = 0, bhi = 0;
        if (lane == 0) {
            unsigned long long b = atomicAdd(&w.ctr[0], (unsigned long long)pc.next);
            blo = (unsigned int)b; bhi = (unsigned int)(b >> 32);
        }
        blo = __builtin_amdgcn_readfirstlane(blo); bhi = __builtin_amdgcn_readfirstlane(bhi);
        pc.pos = ((unsigned long long)bhi << 32) | blo;
        pc.left = pc.next;
        pc.next = pc.next < POOL_CHUNK_MAX ? pc.next * 2 : POOL_CHUNK_MAX;
    }
    if (rec) {
        const unsigned long long slot = pc.pos + __popcll(m & lt);
        if (slot < w.pool_cap) {
            HitRec hr; hr.ray = ray.r; hr.k = ray.cnt; hr.shape = shape;
            w.pool[slot] = hr;
#pragma unroll
            for (int k = 0; k < NV; k++) w.pool_v[NV * slot + k] = vals[k];
        }
        ray.cnt++;
    }
    pc.pos += h; pc.left -= h;
}

struct __attribute__((packed, aligned(4))) DwordPair { uint32_t a, b; };   // two consecutive CSR entries, stored at once
#ifndef SCATTER8_UNROLL
#define SCATTER8_UNROLL 16
#endif
// Whole-ray index batches (WalkOut::pool_pair) write PAIR records, 16 bytes for two hits: {ray, k of the first, shape, shape | NONE}.  A lane
// keeps one hit pending and writes a record when its ray's next hit arrives — or, alone, when the ray retires (flush) — so the pool holds
// 8 bytes per hit instead of HitRec's 12, and the scatter reads one ray offset per TWO hits: the CSR assembly of a hit-heavy batch (457 M
// hits for configs[3]'s 100 M rays) is bound by exactly those dependent gathers.  Measured against the 8-byte single-hit record
// {ray, k << 25 | shape} it replaced (profiles/r4_pair_records_*_ab.log): 12.5 M incoherent rays 2.88 -> 2.75 ms per step, 10 M primary
// rays 1.914 -> 1.868; and no limit on hits per ray or shapes per scene, so no fallback format.
__device__ __forceinline__ void pool_invalidate_tail16(uint4* pool, unsigned long long pool_cap, const PoolCursor& pc, int lane) {
    for (uint32_t j = (uint32_t)lane; j < pc.left; j += WAVE)
        if (pc.pos + j < pool_cap) pool[pc.pos + j].x = NONE;
}
template <typename RAY>
__device__ __forceinline__ void report_pair(bool rec, bool flush, uint32_t shape, RAY& ray, uint32_t& pend, uint4* pool, unsigned long long pool_cap,
                                            unsigned long long* ctr, PoolCursor& pc, int lane, unsigned long long lt) {
    const bool emit = (rec || flush) && pend != NONE;
    const unsigned long long m = __ballot(emit);
    if (m) {
        const uint32_t h = (uint32_t)__popcll(m);
        if (h > pc.left) {   // wave-uniform: start a new chunk, invalidate what is left of the old one
            pool_invalidate_tail16(pool, pool_cap, pc, lane);
            unsigned int blo = 0, bhi = 0;
            if (lane == 0) {
                unsigned long long b = atomicAdd(&ctr[0], (unsigned long long)pc.next);
                blo = (unsigned int)b; bhi = (unsigned int)(b >> 32);
            }
            blo = __builtin_amdgcn_readfirstlane(blo); bhi = __builtin_amdgcn_readfirstlane(bhi);
            pc.pos = ((unsigned long long)bhi << 32) | blo;
            pc.left = pc.next;
            pc.next = pc.next < POOL_CHUNK_MAX ? pc.next * 2 : POOL_CHUNK_MAX;
        }
        if (emit) {
            const unsigned long long slot = pc.pos + __popcll(m & lt);
            if (slot < pool_cap) pool[slot] = make_uint4(ray.r, ray.cnt - 1u, pend, rec ? shape : NONE);   // (the pending hit is number cnt - 1)
        }
        pc.pos += h; pc.left -= h;
    }
    if (rec) { pend = emit ? NONE : shape; ray.cnt++; }
    else if (emit) pend = NONE;
}

template <typename T, int MODE>
__device__ __forceinline__ void walk_epilogue(const WalkOut<T>& w, PoolCursor& pc, int lane, bool stats,
                                              unsigned long long steps, unsigned long long leaf_steps,
                                              unsigned long long wsteps, unsigned long long cands) {
    if (MODE < MODE_CLOSEST) pool_invalidate_tail(w.pool, w.pool_cap, pc, lane);
    if (stats) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            steps += __shfl_down(steps, d);
            leaf_steps += __shfl_down(leaf_steps, d);
            cands += __shfl_down(cands, d);
        }
        if (lane == 0) {
            atomicAdd(&w.ctr[1], steps); atomicAdd(&w.ctr[2], leaf_steps); atomicAdd(&w.ctr[4], wsteps);
            if (MODE == MODE_CLOSEST) atomicAdd(&w.ctr[5], cands);
        }
    }
}

// a wide node (common.hpp WideNode) in registers, and its fetch from global memory / LDS
template <typename T> struct WideRegs { T mn[3][4], mx[3][4]; uint32_t ref[4]; };
template <typename T> struct WideIo {
    static constexpr int CHUNKS = (int)(sizeof(WideRegs<T>) / 16);   // 7 (f32) / 13 (f64) 16-byte chunks per node
    static_assert(sizeof(WideRegs<T>) % 16 == 0, "wide regs");
    static __device__ __forceinline__ WideRegs<T> from_global(const WideNode<T>* __restrict__ p) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        uint4 c[CHUNKS];
#pragma unroll
        for (int j = 0; j < CHUNKS; j++) c[j] = q[j];
        WideRegs<T> r;
        __builtin_memcpy(&r, c, sizeof r);
        return r;
    }
    // LDS copy: node-major, CHUNKS x 16 bytes per slot, so the chunk offsets are immediates of the ds_read_b128s
    static __device__ __forceinline__ WideRegs<T> from_lds(const uint4* nodes, uint32_t slot) {
        const uint4* q = nodes + __umul24(slot, (uint32_t)CHUNKS);   // (24-bit multiply: full rate, v_mul_lo_u32 is quarter rate)
        uint4 c[CHUNKS];
#pragma unroll
        for (int j = 0; j < CHUNKS; j++) c[j] = q[j];
        WideRegs<T> r;
        __builtin_memcpy(&r, c, sizeof r);
        return r;
    }
};

// ---- the walk launches of traverse_enqueue, one per file; each writes h->walk_kernel: the kernel's name as rocprofv3 spells it
//      (bvhgpu_hits_walk_kernel: bench.py looks its counters up under this name instead of rebuilding template strings by hand)
template <typename T> inline const char* walk_type_name() { return sizeof(T) == 4 ? "float" : "double"; }
// walk_binary.hip: k_traverse, or k_traverse_lds (use_lds; split_at != 0: every ray as two items)
template <typename T>
void launch_binary(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, bool stats,
                   bool use_lds, uint32_t split_at);
// walk_ordered.hip: k_traverse_ordered, or k_traverse_heap (best_first)
template <typename T>
void launch_ordered(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, bool ascending,
                    bool best_first, uint32_t* ovf_flag);
// walk_wide.hip: k_traverse_wide, and the number of workgroups that launch will have
template <typename T>
void launch_wide_walk(bvhgpu_tree* t, const typename Traits<T>::Ray* rays_dev, size_t n_rays, const WalkOut<T>& w, bvhgpu_hits* h, int mode, int items_log4,
                      bool use_guide, bool early_items, uint32_t* ovf_flag);
template <typename T> size_t wide_walk_grid(const bvhgpu_ctx* ctx, size_t n_rays, int items_log4, bool coherent, bool use_guide);
// csr.hip: counts → offsets → indices (+ values) behind the walk, from what traverse_enqueue has decided about the batch (the counter set
// of the batch is w.ctr); publish_counters: the 8 walk / scan counters to the host page, zeroed for the next call
struct CsrArgs {
    int count_kind;                        // COUNT_*: one count per ray, two (k_traverse_lds split), or the wide walk's masked counts
    int nv;                                // scalars per hit besides the shape index (ModeVals)
    int items_log4;                        // wide walk: 4^items_log4 items per ray
    int stage_shift;                       // staged output (WalkOut::raybuf): 2^stage_shift shapes per ray; 0: none
    bool rec8;                             // the pool holds pair records (WalkOut::pool_pair)
    uint32_t nb;                           // scan blocks of SCAN_BLOCK rays
    unsigned long long cap;                // pool capacity in records
    unsigned long long *ctr_other, *pin;   // the next batch's counter set (zeroed here), the pinned host page
    uint32_t* bsum_other;                  // the next batch's set of scan sums (zeroed here); NULL: the walk left no sums
};
template <typename T> void csr_enqueue(bvhgpu_hits* h, size_t n_rays, const WalkOut<T>& w, const CsrArgs& a);
void publish_counters(hipStream_t st, unsigned long long* ctr, unsigned long long* host_page);

}  // namespace bvhgpu
