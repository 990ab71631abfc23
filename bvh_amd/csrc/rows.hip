// rows.hip — the five-stage schedule of a batch whose result is one variable-length row per query, as a CSR (rows.hpp, whose rows_run puts
// the stages in order for allhits.hip, within.hip, instances_allhits.hip and instances_within.hip: DESIGN.md §4h, §4i, §4m, §4n; region.hip's
// two entries, §4k and §4l, use the scan alone).  A family brings two walks, one query per lane, and the sort of its long rows:
//   k_<family>_count     counts[q] = the candidates of query q                                   (behind rows_begin)
//   k_rows_block_sums    64-bit sum per block of ROWS_SCAN_BLOCK counts; the queries of a sorted batch whose rows are longer than the
//                        family's lane_max are appended to the long-row worklist (any order), those above its lds_max counted
//   k_rows_scan_sums     exclusive scan of the block sums (one workgroup); the batch's 64-bit total
//   ... ONE host read {total, long rows, rows beyond LDS}: BVHGPU_OVERFLOW before anything is sized by the total ...      (rows_scan)
//   k_rows_scan_final    offsets[q] = block base + exclusive scan inside the block, offsets[n] = total                    (rows_offsets)
//   k_<family>_fill      walks again; lane q owns [offsets[q], offsets[q + 1]) and sorts a row up to lane_max by insertion as it fills it
//   k_<family>_sort_row  one workgroup per long row: rows_bitonic on the keys (key, position in the list) with the shape as payload, in
//                        LDS up to lds_max elements, in place in global memory beyond; then the family's finishing step.
// The three kernels here call nothing outside this file, so they are compiled once and the families reach them through the host functions.
#include "rows.hpp"

namespace bvhgpu {

// what the host reads between the scan and the fill (the first 16 bytes of the sums buffer)
struct RowsMeta { unsigned long long total; uint32_t n_long, n_beyond_lds; };

// sums[b] = the counts of block b, in 64 bits; the long rows of a sorted batch (lane_max != 0) go to the worklist
__global__ __launch_bounds__(256) void k_rows_block_sums(const uint32_t* __restrict__ counts, uint32_t n, unsigned long long* __restrict__ sums,
                                                         RowsMeta* __restrict__ meta, uint32_t* __restrict__ work, uint32_t lane_max, uint32_t lds_max) {
    __shared__ unsigned long long part[256];
    const uint32_t base = blockIdx.x * ROWS_SCAN_BLOCK + threadIdx.x * ROWS_SCAN_ITEMS;
    unsigned long long s = 0;
    for (uint32_t j = 0; j < ROWS_SCAN_ITEMS; j++) {
        const uint32_t q = base + j;
        if (q < n) {   // (base + j cannot wrap: n < 2^32 - 1 and the grid covers n)
            const uint32_t c = counts[q];
            s += c;
            if (lane_max != 0 && c > lane_max) {
                work[atomicAdd(&meta->n_long, 1u)] = q;   // (at most n entries: one per query)
                if (c > lds_max) atomicAdd(&meta->n_beyond_lds, 1u);
            }
        }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// one workgroup: sums[b] becomes the sum of the blocks in front of b; meta->total
__global__ __launch_bounds__(256) void k_rows_scan_sums(unsigned long long* __restrict__ sums, uint32_t nb, RowsMeta* __restrict__ meta) {
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += 256) {   // (nb is uniform: every thread runs every barrier)
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long own = b < nb ? sums[b] : 0ull;
        part[threadIdx.x] = own;
        __syncthreads();
        for (uint32_t w = 1; w < 256; w <<= 1) {
            const unsigned long long add = threadIdx.x >= w ? part[threadIdx.x - w] : 0ull;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const unsigned long long carry = carry_s;
        if (b < nb) sums[b] = carry + part[threadIdx.x] - own;
        __syncthreads();
        if (threadIdx.x == 255) carry_s = carry + part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) meta->total = carry_s;
}

// offsets[q] for the block's counts (the host has checked that the total fits 32 bits)
__global__ __launch_bounds__(256) void k_rows_scan_final(const uint32_t* __restrict__ counts, uint32_t n, const unsigned long long* __restrict__ sums,
                                                         const RowsMeta* __restrict__ meta, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * ROWS_SCAN_BLOCK + threadIdx.x * ROWS_SCAN_ITEMS;
    uint32_t c[ROWS_SCAN_ITEMS], own = 0;
    for (uint32_t j = 0; j < ROWS_SCAN_ITEMS; j++) {
        c[j] = base + j < n ? counts[base + j] : 0u;
        own += c[j];
    }
    part[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t w = 1; w < 256; w <<= 1) {
        const uint32_t add = threadIdx.x >= w ? part[threadIdx.x - w] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = (uint32_t)sums[blockIdx.x] + part[threadIdx.x] - own;
    for (uint32_t j = 0; j < ROWS_SCAN_ITEMS; j++) {
        if (base + j < n) offsets[base + j] = run;
        run += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n] = (uint32_t)meta->total;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static uint32_t rows_blocks(size_t n) { return (uint32_t)((n + ROWS_SCAN_BLOCK - 1) / ROWS_SCAN_BLOCK); }
static unsigned long long* sums_of(RowsMeta* meta) { return reinterpret_cast<unsigned long long*>(meta + 1); }

uint32_t* rows_begin(bvhgpu_hits* h, size_t n, bool with_work) {
    h->rows_counts.reserve(n * 4);
    h->rows_sums.reserve(sizeof(RowsMeta) + (size_t)rows_blocks(n) * sizeof(unsigned long long));
    if (with_work) h->rows_work.reserve(n * 4);
    BVH_HIP(hipMemsetAsync(h->rows_sums.p, 0, sizeof(RowsMeta), h->ctx->stream));
    return h->rows_counts.as<uint32_t>();
}

RowsTotals rows_scan(bvhgpu_hits* h, size_t n, uint32_t lane_max, uint32_t lds_max) {
    hipStream_t st = h->ctx->stream;
    RowsMeta* meta = h->rows_sums.as<RowsMeta>();
    const uint32_t nb = rows_blocks(n);
    hipLaunchKernelGGL(k_rows_block_sums, dim3(nb), dim3(256), 0, st, h->rows_counts.as<uint32_t>(), (uint32_t)n, sums_of(meta), meta,
                       h->rows_work.as<uint32_t>(), lane_max, lds_max);
    hipLaunchKernelGGL(k_rows_scan_sums, dim3(1), dim3(256), 0, st, sums_of(meta), nb, meta);
    BVH_HIP(hipGetLastError());
    RowsMeta* got = static_cast<RowsMeta*>(h->ctx->pinned);
    BVH_HIP(hipMemcpyAsync(got, meta, sizeof(RowsMeta), hipMemcpyDeviceToHost, st));
    BVH_HIP(hipStreamSynchronize(st));
    const RowsTotals r = {got->total, got->n_long, got->n_beyond_lds};
    if (r.total > 0xFFFFFFFFull) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::Overflow};
    if (r.total == 0) BVH_HIP(hipMemsetAsync(h->offsets.p, 0, (n + 1) * 4, st));   // every row is empty
    return r;
}

void rows_offsets(bvhgpu_hits* h, size_t n) {
    RowsMeta* meta = h->rows_sums.as<RowsMeta>();
    hipLaunchKernelGGL(k_rows_scan_final, dim3(rows_blocks(n)), dim3(256), 0, h->ctx->stream, h->rows_counts.as<uint32_t>(), (uint32_t)n, sums_of(meta),
                       meta, h->offsets.as<uint32_t>());
}

}  // namespace bvhgpu
