// tree_node.hpp — the record fetch of the walks over the BvhNode image (knn_tree.hip, instances_knn_tree.hip), moved unchanged out of
// knn_tree.hip so that both descents read a record with the same loads.
#pragma once

#include <cstddef>

#include "common.hpp"

namespace bvhgpu {

// ---- record fetch: four (f32) / seven (f64) 16-byte loads per lane; the records are 16-byte aligned (64 B / 112 B in a hipMalloc'ed array)
template <typename T> struct TreeRegs { T lmn[3], lmx[3], rmn[3], rmx[3]; uint32_t parent, l, r, shape; };

__device__ __forceinline__ TreeRegs<float> load_tree_node(const bvhgpu_node_f32* p) {
    const float4* q = reinterpret_cast<const float4*>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    const uint4 w = reinterpret_cast<const uint4*>(p)[3];
    TreeRegs<float> r;
    r.lmn[0] = a.x; r.lmn[1] = a.y; r.lmn[2] = a.z; r.lmx[0] = a.w; r.lmx[1] = b.x; r.lmx[2] = b.y;
    r.rmn[0] = b.z; r.rmn[1] = b.w; r.rmn[2] = c.x; r.rmx[0] = c.y; r.rmx[1] = c.z; r.rmx[2] = c.w;
    r.parent = w.x; r.l = w.y; r.r = w.z; r.shape = w.w;
    return r;
}
__device__ __forceinline__ TreeRegs<double> load_tree_node(const bvhgpu_node_f64* p) {
    const double2* q = reinterpret_cast<const double2*>(p);
    const double2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
    const uint4 w = reinterpret_cast<const uint4*>(p)[6];
    TreeRegs<double> r;
    r.lmn[0] = a.x; r.lmn[1] = a.y; r.lmn[2] = b.x; r.lmx[0] = b.y; r.lmx[1] = c.x; r.lmx[2] = c.y;
    r.rmn[0] = d.x; r.rmn[1] = d.y; r.rmn[2] = e.x; r.rmx[0] = e.y; r.rmx[1] = f.x; r.rmx[2] = f.y;
    r.parent = w.x; r.l = w.y; r.r = w.z; r.shape = w.w;
    return r;
}
static_assert(sizeof(bvhgpu_node_f32) == 64 && offsetof(bvhgpu_node_f32, parent) == 48, "bvhgpu_node_f32 layout");
static_assert(sizeof(bvhgpu_node_f64) == 112 && offsetof(bvhgpu_node_f64, parent) == 96, "bvhgpu_node_f64 layout");

}  // namespace bvhgpu
