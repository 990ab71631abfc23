// point_dist.hpp — the two shape distances of the point queries (k_nearest in nearest.hip, k_knearest in knn.hip), moved unchanged
// out of the file k_nearest used to share with the ray walks so that both walks compute the same bits:
// Shape distance = <Triangle as PointDistance>::distance_squared (testbase.rs:367-443: Embree's closest point on a
// triangle with degenerate-triangle guards) or the shape's own Aabb::min_distance_squared (UnitBox,
// testbase.rs:101-105; aabb_impl.rs:618-629).  Same operation order as the reference, no contraction.
#pragma once

#include "walk.hpp"

namespace bvhgpu {

template <typename T> __device__ __forceinline__ T aabb_min_dist2(const T mn[3], const T mx[3], const T p[3]) {
    T out[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const T size = mx[k] - mn[k];
        const T half = size * (T)0.5;
        const T centre = mn[k] + half;
        const T delta = p[k] - centre;
        const T q = fabs(delta) - half;
        out[k] = (q > (T)0) ? q : (T)0;   // x.max(0): NaN → 0
    }
    return dot3<T>(out, out);
}
template <typename T> __device__ __forceinline__ void closest_point_segment(const T p[3], const T a[3], const T b[3], T out[3]) {
    T ab[3], ap[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ap[k] = p[k] - a[k]; }
    const T m = dot3<T>(ab, ab);
    T s12 = dot3<T>(ab, ap) / m;
    s12 = s12 < (T)0 ? (T)0 : (s12 > (T)1 ? (T)1 : s12);   // f32::clamp (keeps NaN)
#pragma unroll
    for (int k = 0; k < 3; k++) { const T t = s12 * ab[k]; out[k] = a[k] + t; }
}
template <typename T> __device__ void closest_point_triangle(const T p[3], const T a[3], const T b[3], const T c[3], T out[3]) {
    const bool ab_eq = a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
    const bool bc_eq = b[0] == c[0] && b[1] == c[1] && b[2] == c[2];
    const bool ac_eq = a[0] == c[0] && a[1] == c[1] && a[2] == c[2];
    if (ab_eq && bc_eq && ac_eq) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
    if (ab_eq) { closest_point_segment<T>(p, a, c, out); return; }
    if (bc_eq || ac_eq) { closest_point_segment<T>(p, a, b, out); return; }
    T ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
    const T d1 = dot3<T>(ab, ap), d2 = dot3<T>(ac, ap);
    if (d1 <= (T)0 && d2 <= (T)0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
#pragma unroll
    for (int k = 0; k < 3; k++) bp[k] = p[k] - b[k];
    const T d3 = dot3<T>(ab, bp), d4 = dot3<T>(ac, bp);
    if (d3 >= (T)0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
#pragma unroll
    for (int k = 0; k < 3; k++) cp[k] = p[k] - c[k];
    const T d5 = dot3<T>(ab, cp), d6 = dot3<T>(ac, cp);
    if (d6 >= (T)0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
    const T m1 = d1 * d4, m2 = d3 * d2;
    const T vc = m1 - m2;
    if (vc <= (T)0 && d1 >= (T)0 && d3 <= (T)0) {
        const T den = d1 - d3;
        const T v = d1 / den;
#pragma unroll
        for (int k = 0; k < 3; k++) { const T t = v * ab[k]; out[k] = a[k] + t; }
        return;
    }
    const T m3 = d5 * d2, m4 = d1 * d6;
    const T vb = m3 - m4;
    if (vb <= (T)0 && d2 >= (T)0 && d6 <= (T)0) {
        const T den = d2 - d6;
        const T v = d2 / den;
#pragma unroll
        for (int k = 0; k < 3; k++) { const T t = v * ac[k]; out[k] = a[k] + t; }
        return;
    }
    const T m5 = d3 * d6, m6 = d5 * d4;
    const T va = m5 - m6;
    const T e43 = d4 - d3, e56 = d5 - d6;
    if (va <= (T)0 && e43 >= (T)0 && e56 >= (T)0) {
        const T den = e43 + e56;
        const T v = e43 / den;
#pragma unroll
        for (int k = 0; k < 3; k++) { const T cb = c[k] - b[k]; const T t = v * cb; out[k] = b[k] + t; }
        return;
    }
    T sum = va + vb;
    sum = sum + vc;
    const T denom = (T)1 / sum;
    const T v = vb * denom, w = vc * denom;
#pragma unroll
    for (int k = 0; k < 3; k++) { const T t1 = v * ab[k]; const T t2 = w * ac[k]; const T r = a[k] + t1; out[k] = r + t2; }
}
template <typename T> __device__ __forceinline__ T triangle_dist2(const T* __restrict__ tri, const T p[3]) {
    const T a[3] = {tri[0], tri[1], tri[2]}, b[3] = {tri[3], tri[4], tri[5]}, c[3] = {tri[6], tri[7], tri[8]};
    T nearest[3], diff[3];
    closest_point_triangle<T>(p, a, b, c, nearest);
#pragma unroll
    for (int k = 0; k < 3; k++) diff[k] = p[k] - nearest[k];
    return dot3<T>(diff, diff);
}

// The third shape distance (bvhgpu_knearest_sphere_* / _knearest_tree_sphere_* / _within_sphere_*): the squared distance
// from p to the solid ball {cx, cy, cz, r} of bvhgpu_tree_set_spheres.  Every operation rounded once in T, in this order, no contraction:
//   f[k] = p[k] - c[k];  s2 = dot3(f, f);  len = sqrt(s2) (correctly rounded);  g = len - r;  q = (g < 0) ? 0 : g;  d = q * q
// A point inside or on the ball is at distance 0.  Nothing is special-cased:
//   - a NaN in the sphere or the point gives d = NaN — NOT 0, unlike the box distance's max(0): `g < 0` is false for NaN and q keeps it.
//     The families' NaN rules then apply (never a candidate of within; accepted by k-nearest only while the list is not full);
//   - r is taken literally and never validated (as set_spheres says): a negative r adds |r|; r = +inf gives 0 unless len is +inf too,
//     which gives NaN;
//   - an s2 that overflows gives len = +inf and d = +inf.
// Lists and thresholds hold d; output distances are sqrt(d), as for the other two kinds.  The walks still prune by the tree's boxes:
// rows are "the k nearest" / "all within" in the geometric sense where every sphere lies inside its shape's box (spheres_aabbs);
// a sphere that reaches outside its box can be pruned, as the ray walks can miss it.
// `sphere` is 16-byte aligned (load_sphere, walk.hpp).
template <typename T> __device__ __forceinline__ T sphere_dist2(const T* __restrict__ sphere, const T p[3]) {
    T s[4], f[3];
    load_sphere(sphere, s);
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = p[k] - s[k];
    const T s2 = dot3<T>(f, f);
    const T len = sqrt(s2);
    const T g = len - s[3];
    const T q = (g < (T)0) ? (T)0 : g;   // (keeps NaN)
    return q * q;
}

}  // namespace bvhgpu
