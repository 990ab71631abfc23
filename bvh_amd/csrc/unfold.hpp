// unfold.hpp — the FlatNode array of a built tree as an unfolded TravNode array, for the batches that walk `trav` but must see a leaf's
// navigator box where it differs from the shape's own (a split without SAH winner: within.hip, region.hip).
#pragma once

#include "engine.hpp"

namespace bvhgpu {

// the FlatNode array as an unfolded TravNode array, entry for entry (a non-leaf entry's entry_index is i + 1: flat_bvh.rs:104-127)
template <typename T>
__global__ __launch_bounds__(256) void k_within_unfold(const typename Traits<T>::Flat* __restrict__ flat, uint32_t n_flat, TravNode<T>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_flat) return;
    const typename Traits<T>::Flat f = flat[i];
    TravNode<T> e = {};
    for (int c = 0; c < 3; c++) { e.mn[c] = f.min[c]; e.mx[c] = f.max[c]; }
    e.exit = f.exit;
    e.shape = f.entry == NONE ? f.shape : (TRAV_INNER | SLOT_NONE);
    out[i] = e;
}

}  // namespace bvhgpu
