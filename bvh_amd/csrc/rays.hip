// rays.hip — what a caller does with rays outside a walk: Ray::intersects_triangle for independent (ray, triangle) pairs, Ray::new
// (src/ray/ray_impl.rs:70-80), the bench ray streams (src/testbase.rs:687-691, primary rays) and the copy kernels of the host batches.
#include "walk.hpp"

namespace bvhgpu {

// ------------------------------------------------------------------------------------------------
// Ray::intersects_triangle for n independent (ray, triangle) pairs — ray_impl.rs:154-213
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ray_triangle_pairs(const typename Traits<T>::Ray* __restrict__ rays,
                                                            const T* __restrict__ tris, uint32_t n, T* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const typename Traits<T>::Ray* rp = rays + i;
    const T o[3] = {rp->o[0], rp->o[1], rp->o[2]};
    const T d[3] = {rp->d[0], rp->d[1], rp->d[2]};
    T r[3];
    ray_triangle<T>(o, d, tris + 9 * (size_t)i, r);
    out[3 * (size_t)i] = r[0]; out[3 * (size_t)i + 1] = r[1]; out[3 * (size_t)i + 2] = r[2];
}
template <typename T>
void ray_triangle_pairs(bvhgpu_ctx* ctx, const typename Traits<T>::Ray* rays_dev, const T* tris_dev, size_t n, T* out_dev) {
    if (!n) return;
    hipLaunchKernelGGL(k_ray_triangle_pairs<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rays_dev,
                       tris_dev, (uint32_t)n, out_dev);
    BVH_HIP(hipGetLastError());
}
template void ray_triangle_pairs<float>(bvhgpu_ctx*, const bvhgpu_ray_f32*, const float*, size_t, float*);
template void ray_triangle_pairs<double>(bvhgpu_ctx*, const bvhgpu_ray_f64*, const double*, size_t, double*);

// ------------------------------------------------------------------------------------------------
// Ray::new — ray_impl.rs:70-80
// ------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void ray_new(const T o[3], const T d[3], typename Traits<T>::Ray* out) {
    T xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
    T s = xx + yy;
    s = s + zz;
    T nrm = sqrt(s);  // correctly rounded (no fast-math)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        T dn = d[k] / nrm;
        out->o[k] = o[k];
        out->d[k] = dn;
        out->inv[k] = (T)1 / dn;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_rays_new(const T* __restrict__ origins, const T* __restrict__ dirs, uint32_t n,
                                                  typename Traits<T>::Ray* __restrict__ out, uint32_t stride) {
    // (a grid-stride loop: with origins / dirs in pinned HOST memory the launch is kept small — a few thousand lanes keep the PCIe link busy —
    //  so that it leaves the CUs to the build running beside it)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        // (stride 3: two arrays; stride 6 with dirs = origins + 3: origin and direction of a ray side by side)
        T o[3] = {origins[stride * (size_t)i], origins[stride * (size_t)i + 1], origins[stride * (size_t)i + 2]};
        T d[3] = {dirs[stride * (size_t)i], dirs[stride * (size_t)i + 1], dirs[stride * (size_t)i + 2]};
        ray_new<T>(o, d, out + i);
    }
}

template <typename T>
void rays_new(bvhgpu_ctx* ctx, const T* origins_dev, const T* dirs_dev, size_t n, typename Traits<T>::Ray* out_dev, hipStream_t st, unsigned max_blocks,
              unsigned stride) {
    if (!n) return;
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (max_blocks) blocks = std::min(blocks, max_blocks);
    hipLaunchKernelGGL(k_rays_new<T>, dim3(blocks), dim3(256), 0, st ? st : ctx->stream, origins_dev, dirs_dev, (uint32_t)n, out_dev, (uint32_t)stride);
    BVH_HIP(hipGetLastError());
}
template void rays_new<float>(bvhgpu_ctx*, const float*, const float*, size_t, bvhgpu_ray_f32*, hipStream_t, unsigned, unsigned);
template void rays_new<double>(bvhgpu_ctx*, const double*, const double*, size_t, bvhgpu_ray_f64*, hipStream_t, unsigned, unsigned);

// CSR offsets of one chunk of a host-resident batch (bvhgpu_traverse_host_*), moved to their place in the whole batch's array:
// out[0] holds the hits of all chunks before this one (written by the previous chunk's pass on the same stream; 0 for the first)
// (out_host: the caller's own array when it is pinned memory the device can write — the offsets then need no download)
// (first: the batch's first chunk — its base is 0 and out[0] is written here instead of read)
__global__ __launch_bounds__(256) void k_offsets_rebase(const uint32_t* __restrict__ offs, uint32_t n_plus_1, uint32_t* __restrict__ out,
                                                        uint32_t* __restrict__ out_host, uint32_t first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_plus_1) return;
    const uint32_t v = (first ? 0u : out[0]) + (i ? offs[i] : 0u);
    if (i || first) out[i] = v;        // (out[0] of a later chunk is the base itself: the previous chunk's last entry)
    if (out_host) out_host[i] = v;
}
// ... and its index list appended to the batch's (what fits into `cap` entries): base = out[0], count = offs[n_rays]
__global__ __launch_bounds__(256) void k_indices_append(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ offs, uint32_t n_rays,
                                                        const uint32_t* __restrict__ base_ptr, uint32_t* __restrict__ dst, unsigned long long cap, uint32_t first) {
    const unsigned long long base = first ? 0ull : base_ptr[0], cnt = offs[n_rays];
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < cnt && base + i < cap; i += (unsigned long long)gridDim.x * blockDim.x)
        dst[base + i] = idx[i];
}
void offsets_rebase(hipStream_t st, const uint32_t* offs_dev, size_t n_rays, uint32_t* out_dev, uint32_t* out_host, const uint32_t* idx_dev,
                    uint32_t* idx_all, size_t idx_cap, bool first) {
    // (the index list first: it reads the chunk's base out[0] and the chunk-local count, both untouched by the rebase)
    if (idx_all && idx_cap)
        hipLaunchKernelGGL(k_indices_append, dim3(128), dim3(256), 0, st, idx_dev, offs_dev, (uint32_t)n_rays, out_dev, idx_all, (unsigned long long)idx_cap,
                           first ? 1u : 0u);
    hipLaunchKernelGGL(k_offsets_rebase, dim3((unsigned)((n_rays + 1 + 255) / 256)), dim3(256), 0, st, offs_dev, (uint32_t)(n_rays + 1), out_dev, out_host,
                       first ? 1u : 0u);
    BVH_HIP(hipGetLastError());
}

// 16-byte copy (the caller's Ray structs out of pinned host memory, read by the device directly)
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
void copy16(hipStream_t st, const void* src, void* dst, size_t bytes) {   // bytes: a multiple of 4; the tail goes word by word
    const size_t n16 = bytes / 16;
    if (n16) hipLaunchKernelGGL(k_copy16, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 128)), dim3(256), 0, st, static_cast<const uint4*>(src), static_cast<uint4*>(dst), n16);
    if (bytes & 15) BVH_HIP(hipMemcpyAsync(static_cast<char*>(dst) + n16 * 16, static_cast<const char*>(src) + n16 * 16, bytes & 15, hipMemcpyDefault, st));
    BVH_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// bench ray stream: create_ray (testbase.rs:687-691) over splitmix64 (:558-564), next_point3 (:567-595).
// splitmix64's state after j draws is j*GAMMA, so ray r uses states (2r+1)*GAMMA and (2r+2)*GAMMA.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ void point3_from_state(unsigned long long state, const float* bounds, float out[3]) {
    const unsigned long long u = mix64(state);
    const long long a = (long long)((u >> 32) & 0xFFFFFFFFull) - 0x80000000ll;
    const long long b = (long long)(u & 0xFFFFFFFFull) - 0x80000000ll;
    const unsigned long long ub = (unsigned long long)b;
    const unsigned long long rot = (ub << 6) | (ub >> 58);
    const long long c = a ^ (long long)rot;
    const int r[3] = {(int)a, (int)b, (int)(unsigned int)(unsigned long long)c};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float q = (float)r[k] / 2147483648.0f;  // i32::MAX as f32 == 2^31
        float fv = (q + 1.0f) * 0.5f;
        float size = bounds[3 + k] - bounds[k];
        float off = fv * size;
        out[k] = bounds[k] + off;
    }
}

struct Bounds6 { float b[6]; };

template <typename T>
__global__ __launch_bounds__(256) void k_gen_rays(unsigned long long first, uint32_t n, Bounds6 bounds,
                                                  typename Traits<T>::Ray* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long G = 0x9E3779B97F4A7C15ull;
    const unsigned long long r = first + i;
    float o[3], d[3];
    point3_from_state((2ull * r + 1ull) * G, bounds.b, o);
    point3_from_state((2ull * r + 2ull) * G, bounds.b, d);
    T oo[3] = {(T)o[0], (T)o[1], (T)o[2]};
    T dd[3] = {(T)d[0], (T)d[1], (T)d[2]};
    ray_new<T>(oo, dd, out + i);
}

// coherent primary rays (BASELINE.json configs[2]): pinhole camera, row-major W x H image.  Definition in
// include/bvh_mi355x.h (bvhgpu_gen_primary_rays_*); every operation is a separately rounded f32 op.
struct Camera14 { float c[14]; };
template <typename T>
__global__ __launch_bounds__(256) void k_gen_primary(Camera14 cam, uint32_t width, uint32_t height, unsigned long long first,
                                                     uint32_t n, typename Traits<T>::Ray* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long id = first + i;
    const uint32_t x = (uint32_t)(id % width), y = (uint32_t)(id / width);
    float fx = (float)x + 0.5f; fx = fx / (float)width; fx = fx * 2.0f; const float sx = fx - 1.0f;
    float fy = (float)y + 0.5f; fy = fy / (float)height; fy = fy * 2.0f; const float sy = 1.0f - fy;
    const float ax = sx * cam.c[12], ay = sy * cam.c[13];
    T oo[3], dd[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float r = ax * cam.c[3 + k], u = ay * cam.c[6 + k];
        const float t = cam.c[9 + k] + r;
        const float d = t + u;
        oo[k] = (T)cam.c[k];
        dd[k] = (T)d;
    }
    ray_new<T>(oo, dd, out + i);
}
template <typename T>
void gen_primary(bvhgpu_ctx* ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first, size_t n,
                 typename Traits<T>::Ray* out_dev) {
    if (!n) return;
    Camera14 c;
    for (int k = 0; k < 14; k++) c.c[k] = cam[k];
    hipLaunchKernelGGL(k_gen_primary<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c, width, height,
                       (unsigned long long)first, (uint32_t)n, out_dev);
    BVH_HIP(hipGetLastError());
}
template void gen_primary<float>(bvhgpu_ctx*, const float*, uint32_t, uint32_t, uint64_t, size_t, bvhgpu_ray_f32*);
template void gen_primary<double>(bvhgpu_ctx*, const float*, uint32_t, uint32_t, uint64_t, size_t, bvhgpu_ray_f64*);

void gen_rays_f32(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f32* out_dev) {
    if (!n) return;
    Bounds6 b;
    for (int k = 0; k < 6; k++) b.b[k] = bounds[k];
    hipLaunchKernelGGL(k_gen_rays<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (unsigned long long)first, (uint32_t)n, b, out_dev);
    BVH_HIP(hipGetLastError());
}
void gen_rays_f64(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f64* out_dev) {
    if (!n) return;
    Bounds6 b;
    for (int k = 0; k < 6; k++) b.b[k] = bounds[k];
    hipLaunchKernelGGL(k_gen_rays<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (unsigned long long)first, (uint32_t)n, b, out_dev);
    BVH_HIP(hipGetLastError());
}

}  // namespace bvhgpu
