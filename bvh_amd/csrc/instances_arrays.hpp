// instances_arrays.hpp — which array of every member and of the top level a point walk over an instance set reads (instances_within.hip,
// instances_knn.hip): one table and one rule for both families.
#pragma once

#include <vector>

#include "instances.hpp"
#include "unfold.hpp"

namespace bvhgpu {

// one array of the table: a member's, or (the table's last row) the top level's
template <typename T> struct InstWithinArr {
    const TravNode<T>* nodes;   // the folded array, the uploaded array, or the unfolded mirror
    const T* tris;              // n x 9 (members)
    uint32_t n_trav, unfolded;
};

// The table of a committed set, made on the set's stream into the caller's buffers: region.hip's rule (RegionMember), array by array.  The
// folded `trav` array for a built tree, the UNFOLDED rule for an uploaded FlatBvh and a one-shape tree, and an unfolded mirror of the
// FlatNode array (k_within_unfold, into `mirrors`) for a built tree with empty child bounds — the top level included.  `table` receives
// n_trees + 1 rows (the last is the top level's) from `table_host`, which stays alive while the upload is in flight.  → the device table
template <typename T>
const InstWithinArr<T>* instances_array_table(bvhgpu_instances* s, DevBuf& mirrors, DevBuf& table, std::vector<unsigned char>& table_host) {
    hipStream_t st = s->ctx->stream;
    const size_t nt = s->trees.size();
    std::vector<InstWithinArr<T>> tbl(nt + 1);
    std::vector<size_t> mirror_at(nt + 1, (size_t)-1);
    size_t n_mirror = 0;
    for (size_t k = 0; k <= nt; k++) {
        bvhgpu_tree* t = k < nt ? s->trees[k] : s->top;
        InstWithinArr<T>& r = tbl[k];
        r = InstWithinArr<T>{nullptr, nullptr, 0u, 0u};
        if (t->n == 0) continue;   // (no instance of it has a finite world box: never looked up)
        ensure_flat_arrays(t);
        const bool mirror = t->exact_only && t->built && !t->unfolded && t->n >= 2;   // within_batch's rule, array by array
        r.unfolded = (t->unfolded || t->n == 1 || mirror) ? 1u : 0u;
        r.n_trav = (uint32_t)(mirror ? t->n_flat : t->n_trav);
        r.nodes = t->trav.as<TravNode<T>>();
        r.tris = t->tris.as<T>();
        if (mirror) { mirror_at[k] = n_mirror; n_mirror += r.n_trav; }
    }
    if (n_mirror) mirrors.reserve(n_mirror * sizeof(TravNode<T>));
    for (size_t k = 0; k <= nt; k++) {
        if (mirror_at[k] == (size_t)-1) continue;
        bvhgpu_tree* t = k < nt ? s->trees[k] : s->top;
        TravNode<T>* dst = mirrors.as<TravNode<T>>() + mirror_at[k];
        hipLaunchKernelGGL((k_within_unfold<T>), dim3((tbl[k].n_trav + 255) / 256), dim3(256), 0, st, t->flat.as<typename Traits<T>::Flat>(), tbl[k].n_trav, dst);
        tbl[k].nodes = dst;
    }
    BVH_HIP(hipGetLastError());
    table.reserve((nt + 1) * sizeof(InstWithinArr<T>));
    table_host.assign(reinterpret_cast<const unsigned char*>(tbl.data()), reinterpret_cast<const unsigned char*>(tbl.data() + nt + 1));
    BVH_HIP(hipMemcpyAsync(table.p, table_host.data(), (nt + 1) * sizeof(InstWithinArr<T>), hipMemcpyHostToDevice, st));
    return table.as<InstWithinArr<T>>();
}

}  // namespace bvhgpu
