// instances.hpp — what the two-level walks over an instance set share (instances.hip, instances_allhits.hip): the member table, the
// per-instance record and the one row of a 3x4 transform that re-expresses a world ray in an object's frame.
#pragma once

#include "common.hpp"

namespace bvhgpu {

// what the walk needs of a member tree, read once on entry to an instance
template <typename T> struct InstTree {
    const TravNode<T>* trav;
    const T* prims;    // the array the set's leaf kind reads: aabbs (n x 6), tris (n x 9) or spheres (n x 4) — instances_commit
    const T* aabbs;    // n x 6 (k_instances_prep only)
    uint32_t n_trav, n;
};
// per instance: Y_i row-major 3x4 and the slot of its tree; whole 16-byte chunks (f32: 4, f64: 7)
template <typename T> struct __attribute__((aligned(16))) InstRec {
    T y[12];
    uint32_t tree;
    uint32_t _pad[3];
};
static_assert(sizeof(InstRec<float>) == 64 && sizeof(InstRec<double>) == 112, "instance record");

// what a MASKED walk reads besides: the set's n u32, and NULL (all ones) or one u32 per row of the batch (a ray, a point, a region).
// Without MASKED neither is read.
struct InstMasks {
    const uint32_t* inst;
    const uint32_t* ray;
};

template <typename T> __device__ __forceinline__ InstRec<T> load_rec(const InstRec<T>* __restrict__ p) {
    constexpr int CHUNKS = (int)(sizeof(InstRec<T>) / 16);
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 c[CHUNKS];
#pragma unroll
    for (int j = 0; j < CHUNKS; j++) c[j] = q[j];
    InstRec<T> r;
    __builtin_memcpy(&r, c, sizeof r);
    return r;
}

// p -> ((m[0]*p[0] + m[1]*p[1]) + m[2]*p[2]) [+ m[3]]: one row of a 3x4 transform, every operation rounded once, in this order
template <typename T> __device__ __forceinline__ T row3(const T* m, const T p[3]) {
    const T a = m[0] * p[0], b = m[1] * p[1], c = m[2] * p[2];
    const T s = a + b;
    return s + c;
}
template <typename T> __device__ __forceinline__ T row4(const T* m, const T p[3]) {
    const T s = row3<T>(m, p);
    return s + m[3];
}

}  // namespace bvhgpu
