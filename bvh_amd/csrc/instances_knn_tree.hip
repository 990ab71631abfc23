// instances_knn_tree.hip — the k nearest (instance, shape) pairs of every query point over an instance set, found nearest child first on
// both levels and with an optional search radius per point (bvhgpu_instances_knearest_tree_*; include/bvh_mi355x.h): the
// "tree form" beside instances_knn.hip's "flat form".
//
// Definition.  Per point p a list L of at most k triples (d, instance, shape); d is the squared WORLD distance in T.
//   full = len(L) == k,  bound = L[last].d,  with a limit m = max_dist[j]: r2 = m * m (one multiplication in T)
//   insertion: bvhgpu_knearest_*'s — a full list drops its last element, the new one goes in front of the first e with d < e.d, else at
//   the end.  Every comparison is T's <, > or <= as written; a row that holds a NaN need not be sorted (knn.hip, knn_tree.hip).
//   cmd(box, x)   = 0 if box.min[0] > box.max[0]   (a child of a split without SAH winner carries Aabb::empty(): nothing is known below it)
//                   else box.min_distance_squared(x)
//   admit_w(x)    = (max_dist == NULL || (m >= 0 && x <= r2))     && (!full || x < bound)        a leaf's d, world frame
//   admit_b(x, F) = (max_dist == NULL || (m >= 0 && x <= r2 * F)) && (!full || x < bound * F || bound * F == +inf)
//                   a child box: F = 1 at the top level (world frame: the products are r2 and bound themselves), F of the instance the
//                   walk is in below it (object frame).  A bound or a product that is +inf — a list that holds an infinite distance,
//                   or bound * F overflowing — says nothing about a box whose own distance overflowed as well, so it prunes nothing
//   top(node) over the BvhNode array of the top-level tree (the tree over the world boxes W), root = node 0, with p:
//     Leaf{shape = i}:  enter instance i
//     Node{l, l_aabb, r, r_aabb}:  c = [(l, cmd(l_aabb, p)), (r, cmd(r_aabb, p))];  if c[0].1 > c[1].1: swap   (strict >: ties and NaN keep
//                                  the left child first);  for (idx, cd) in c: if admit_b(cd, 1): top(idx)   (the second test sees the list as
//                                  the first subtree left it)
//   instance i (member t = tree_of[i]), instances_knn.hip's operation order:
//     q[c] = row4(Y_i[c], p);   F = (row3(Y_i[0], Y_i[0]) + row3(Y_i[1], Y_i[1])) + row3(Y_i[2], Y_i[2])
//     member(node) over member t's BvhNode array, root = node 0, with q:
//       Leaf{shape = s}:  w[v][c] = row4(X_i[c], tri_s[v]);  d = triangle_dist2(w, p)  (world triangle, world point);  if admit_w(d): insert (d, i, s)
//       Node{...}:        as above with cmd(., q) and admit_b(., F)
//   r2 * F is ONE multiplication in T, made on entry to the instance; bound * F is ONE multiplication in T, made on entry and whenever
//   `bound` changes.  Row j, padded to k: out_instance / out_shape / out_dist[j * k + m] = L[m].instance, L[m].shape, sqrt(L[m].d); the other
//   slots hold NONE, NONE and +inf.  A negative or NaN max_dist[j], a set without instances and a member without shapes give padding; a
//   limit of 0 keeps only distance 0.
// Why the prune is safe: |p - X v| >= |q - v| / ||Y||_F, so a world triangle with d <= r2 lies within sqrt(r2 * F) of q and one with
// d < bound within sqrt(bound * F); acceptance into a full list is strict, so what a prune skips could not have been accepted (in exact
// arithmetic; where bound * F overflows the box test is switched off instead of comparing inf < inf).  The order of a node's two children depends on the distances alone, never on the list: without prunes the walk visits all
// (instance, shape) pairs in one fixed order per point, the NEAREST-FIRST ORDER, and a row is the list built by offering every pair in
// that order with no prune at all.  Ties stay in that order — neither the flat form's double order nor leaf pre-order: the two forms may
// name different pairs at tied distances; their distances agree.
//
// k_instances_knearest_tree: one query point per lane, ONE loop — k_knearest_tree's stackless descent (record fetch load_tree_node, return
// through the records' parent words, the two child distances computed again on the way up: same inputs, same bits, same order) on two
// levels, with k_instances_knearest's state machine: a lane is either in the top-level array (point p, admit_b with F = 1) or in a member's
// (point q, admit_b with its F).  An admitted top-level leaf loads the instance record, computes q, F and the two limits and points the lane at record 0 of the
// member's array, arriving from above; when the member walk is back at its record 0 with nothing left, the lane resumes the top level at
// that leaf's parent as "came back from that leaf".  Record 0 may be a leaf on either level.  No loop is nested inside a leaf, so the lanes
// of a wave keep stepping together whatever level each is on.  X_i is read again at every member leaf rather than kept in twelve registers
// (DESIGN.md §4q has the register counts of both choices).  The list is k_instances_knearest's: dynamic LDS, three slot-major arrays
// (distances, instances, shapes), instances_knn_block's block rule, no barrier; the insertion is restated here as knn_tree.hip says it must.
//
// MASKED (bvhgpu_instances_knearest_tree_masked_*): point j carries a mask P[j].  The descent is over the SAME top-level array — the
// top level of the whole set — and a top-level leaf whose instance shares no bit with P[j] contributes nothing: one 4-byte load, then it is
// left exactly as a leaf whose member has no shapes is left (`next` stays NONE, the lane returns to the leaf's parent).  The list and the
// bounds only ever see visible pairs.  A point whose mask is 0 does not walk: its row is padding.
#include "engine.hpp"
#include "instances.hpp"
#include "point_dist.hpp"
#include "tree_node.hpp"

namespace bvhgpu {

// instances_knn.hip's rule: the largest of 256 / 128 / 64 lanes whose lists fit 32 KB of LDS, 64 lanes above that
template <typename T> inline unsigned instances_knn_tree_block(uint32_t k) {
    const size_t per_lane = (size_t)k * (sizeof(T) + 8);
    if (256 * per_lane <= 32 * 1024) return 256;
    if (128 * per_lane <= 32 * 1024) return 128;
    return 64;
}
static_assert(BVHGPU_INSTANCES_KNN_MAX_K * 64u * (sizeof(double) + 8u) <= 64u * 1024u, "the lists of 64 lanes must fit a workgroup's LDS");

// what the walk reads of a member: its BvhNode image and its triangles
template <typename T> struct InstTreeMember {
    const typename Traits<T>::Node* nodes;
    const T* tris;          // n x 9
    uint32_t n_nodes;       // 0: a member without shapes
    uint32_t _pad;
};

// cmd: nothing is known below an empty child box
template <typename T> __device__ __forceinline__ T child_min_dist2(const T mn[3], const T mx[3], const T p[3]) {
    const T md = aabb_min_dist2<T>(mn, mx, p);
    return mn[0] > mx[0] ? (T)0 : md;
}

template <typename T, bool MASKED = false>
__global__ __launch_bounds__(256) void k_instances_knearest_tree(const typename Traits<T>::Node* __restrict__ top, uint32_t n_top,
                                                                 const InstTreeMember<T>* __restrict__ members, const InstRec<T>* __restrict__ recs,
                                                                 const T* __restrict__ xforms, const T* __restrict__ points, uint32_t n, uint32_t k,
                                                                 const T* __restrict__ max_dist, uint32_t* __restrict__ out_instance,
                                                                 uint32_t* __restrict__ out_shape, T* __restrict__ out_dist, InstMasks mk) {
    using Node = typename Traits<T>::Node;
    extern __shared__ __align__(16) unsigned char iknt_lds[];
    const uint32_t block = blockDim.x;
    T* __restrict__ ld = reinterpret_cast<T*>(iknt_lds) + threadIdx.x;                                        // slot m: ld[m * block]
    uint32_t* __restrict__ li = reinterpret_cast<uint32_t*>(reinterpret_cast<T*>(iknt_lds) + (size_t)k * block) + threadIdx.x;
    uint32_t* __restrict__ ls = li + (size_t)k * block;
    const uint32_t q = blockIdx.x * block + threadIdx.x;
    if (q >= n) return;
    const T pw[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};   // the world point
    uint32_t len = 0;
    bool full = false;       // len == k
    bool has_nan = false;    // the list holds a NaN: it need not be sorted any more
    T bound = 0;             // L[k - 1].d of a full list
    const bool limited = max_dist != nullptr;
    T r2 = 0;
    bool walk = n_top != 0;
    if (limited) {
        const T m = max_dist[q];
        r2 = m * m;
        walk = walk && m >= (T)0;                // a negative or NaN limit admits nothing
    }
    uint32_t pmask = 0xFFFFFFFFu;
    if constexpr (MASKED) {
        if (mk.ray) pmask = mk.ray[q];
        walk = walk && pmask != 0u;                  // no instance is visible: no walk
    }
    T lim_r = r2;            // what a box test compares with: r2 and bound at the top level, r2 * fn and bound * fn inside an instance
    T lim_b = 0;
    T fn = 0;                // F of the instance the lane is in
    T p[3] = {pw[0], pw[1], pw[2]};
    const Node* nodes = top;
    const T* tris = nullptr;
    uint32_t n_nodes = n_top;
    uint32_t inst = NONE;    // the instance the lane is in; NONE: the top level
    uint32_t top_leaf = 0, top_parent = 0;       // the top-level leaf that sent the lane into `inst`, and that record's parent
    uint32_t cur = 0;        // the record the lane is at
    uint32_t from = NONE;    // the child it came back from; NONE: it arrived from above
#define ADMIT_BOX(x) ((!limited || (x) <= lim_r) && (!full || (x) < lim_b || lim_b == (T)INFINITY))   // admit_b: a limit of +inf prunes nothing
#define ADMIT_W(x) ((!limited || (x) <= r2) && (!full || (x) < bound))
    while (walk) {
        const TreeRegs<T> nd = load_tree_node(nodes + cur);
        uint32_t next = NONE;
        if (nd.shape != NONE) {
            if (inst != NONE) {   // a triangle of the member: the pair (inst, shape), decided in world space
                const T* tri = tris + 9 * (size_t)nd.shape;
                const T* x = xforms + 12 * (size_t)inst;
                T xr[12];
#pragma unroll
                for (int c = 0; c < 12; c++) xr[c] = x[c];
                T w[9];
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    const T tv[3] = {tri[3 * v], tri[3 * v + 1], tri[3 * v + 2]};
#pragma unroll
                    for (int c = 0; c < 3; c++) w[3 * v + c] = row4<T>(xr + 4 * c, tv);
                }
                const T d = triangle_dist2<T>(w, pw);
                if (ADMIT_W(d)) {
                    uint32_t hole = full ? k - 1 : len;   // a full list drops its last element
                    uint32_t pos;                         // in front of the first element e with d < e
                    if (!has_nan) {
                        // ascending list: that element is where a scan from the back stops, so search and shift are one loop
#pragma unroll 1
                        while (hole > 0) {
                            const T e = ld[(hole - 1) * block];
                            if (!(d < e)) break;
                            ld[hole * block] = e;
                            li[hole * block] = li[(hole - 1) * block];
                            ls[hole * block] = ls[(hole - 1) * block];
                            hole--;
                        }
                        pos = hole;
                    } else {
                        // a NaN compares false with everything, so elements in front of it may still be larger than d: search from the front
                        pos = 0;
#pragma unroll 1
                        while (pos < hole && !(d < ld[pos * block])) pos++;
#pragma unroll 1
                        for (; hole > pos; hole--) {
                            ld[hole * block] = ld[(hole - 1) * block];
                            li[hole * block] = li[(hole - 1) * block];
                            ls[hole * block] = ls[(hole - 1) * block];
                        }
                    }
                    ld[pos * block] = d;
                    li[pos * block] = inst;
                    ls[pos * block] = nd.shape;
                    has_nan = has_nan || d != d;
                    if (!full) { len++; full = len == k; }
                    if (full) { bound = ld[(k - 1) * block]; lim_b = bound * fn; }
                }
            } else {              // an instance (its box was admitted, or it is record 0): into its member with the point and the limits in the object's frame
                bool visible = true;
                if constexpr (MASKED) visible = (mk.inst[nd.shape] & pmask) != 0u;   // (hidden: `next` stays NONE, as for a member without shapes)
                if (visible) {
                    const InstRec<T> rec = load_rec<T>(recs + nd.shape);
                    const InstTreeMember<T> mb = members[rec.tree];
                    if (mb.n_nodes != 0u) {
                        top_leaf = cur; top_parent = nd.parent;
                        inst = nd.shape;
                        T f[3];
#pragma unroll
                        for (int c = 0; c < 3; c++) { p[c] = row4<T>(rec.y + 4 * c, pw); f[c] = row3<T>(rec.y + 4 * c, rec.y + 4 * c); }
                        const T f01 = f[0] + f[1];
                        fn = f01 + f[2];
                        lim_r = r2 * fn;
                        lim_b = bound * fn;
                        nodes = mb.nodes; tris = mb.tris; n_nodes = mb.n_nodes;
                        next = 0;     // record 0 of the member's array, from above
                    }
                }
            }
        } else {
            const T dl = child_min_dist2<T>(nd.lmn, nd.lmx, p), dr = child_min_dist2<T>(nd.rmn, nd.rmx, p);
            const bool swap = dl > dr;
            const uint32_t first = swap ? nd.r : nd.l, second = swap ? nd.l : nd.r;
            const T d1 = swap ? dr : dl, d2 = swap ? dl : dr;
            if (from == NONE && ADMIT_BOX(d1)) next = first;            // from above: the nearer child, if it passes
            else if (from != second && ADMIT_BOX(d2)) next = second;    // ... else, or back from the nearer one: the other child
        }
        if (next != NONE) { cur = next; from = NONE; }
        else if (cur != 0) { from = cur; cur = nd.parent; }
        else if (inst != NONE) {   // back at the member's record 0 with nothing left: the top level again, coming back from the leaf
#pragma unroll
            for (int c = 0; c < 3; c++) p[c] = pw[c];
            lim_r = r2; lim_b = bound;
            nodes = top; n_nodes = n_top; inst = NONE;
            if (top_leaf == 0) break;                                   // the top level is that one leaf
            from = top_leaf; cur = top_parent;
        } else break;                                                   // back at the top level's root with nothing left
        if (cur >= n_nodes) break;                                      // (never in a tree the builder wrote)
    }
#undef ADMIT_BOX
#undef ADMIT_W
    // row q: the distances (not squared), then the padding
    uint32_t* oi = out_instance + (size_t)q * k;
    uint32_t* os = out_shape + (size_t)q * k;
    T* od = out_dist + (size_t)q * k;
#pragma unroll 1
    for (uint32_t m = 0; m < len; m++) { oi[m] = li[m * block]; os[m] = ls[m * block]; od[m] = sqrt(ld[m * block]); }
#pragma unroll 1
    for (uint32_t m = len; m < k; m++) { oi[m] = NONE; os[m] = NONE; od[m] = (T)INFINITY; }
}

// the points of a batch over a committed instance set (the caller has checked commit, staleness, that every member was built here and
// n x k < 2^32); max_dist_dev: NULL or n limits
// masked: bvhgpu_instances_knearest_tree_masked_* — the set's masks against point_mask_dev (NULL: all ones); otherwise point_mask_dev is not looked at
template <typename T>
void instances_knearest_tree_batch(bvhgpu_instances* s, const T* points_dev, size_t n, uint32_t k, const T* max_dist_dev, uint32_t* out_instance_dev,
                                   uint32_t* out_shape_dev, T* out_dist_dev, bool masked, const uint32_t* point_mask_dev) {
    if (!n) return;
    using Node = typename Traits<T>::Node;
    hipStream_t st = s->ctx->stream;
    if (s->n == 0 || s->top == nullptr || s->top->n == 0) {   // no instance: every row is padding, written by the flat form's fill path
        instances_knearest_batch<T>(s, points_dev, n, k, out_instance_dev, out_shape_dev, out_dist_dev, false, nullptr);
        return;
    }
    // the member table: made again by every call (a member may have been rebuilt and the set updated), the allocation kept by the set
    const size_t nt = s->trees.size();
    s->knt_members_host.resize(nt * sizeof(InstTreeMember<T>));
    InstTreeMember<T>* host = reinterpret_cast<InstTreeMember<T>*>(s->knt_members_host.data());
    for (size_t t = 0; t < nt; t++) {
        const bvhgpu_tree* m = s->trees[t];
        host[t] = InstTreeMember<T>{m->nodes.as<Node>(), m->tris.as<T>(), m->n ? (uint32_t)m->n_nodes : 0u, 0u};
    }
    s->knt_members.reserve(nt * sizeof(InstTreeMember<T>));
    BVH_HIP(hipMemcpyAsync(s->knt_members.p, host, nt * sizeof(InstTreeMember<T>), hipMemcpyHostToDevice, st));
    const unsigned bs = instances_knn_tree_block<T>(k);
    const size_t lds = (size_t)bs * k * (sizeof(T) + 8);
    const dim3 grid((unsigned)((n + bs - 1) / bs));
    if (masked) {
        const InstMasks mk = {s->masks.as<uint32_t>(), point_mask_dev};
        hipLaunchKernelGGL((k_instances_knearest_tree<T, true>), grid, dim3(bs), lds, st, s->top->nodes.as<Node>(), (uint32_t)s->top->n_nodes,
                           s->knt_members.as<InstTreeMember<T>>(), s->recs.as<InstRec<T>>(), s->xforms.as<T>(), points_dev, (uint32_t)n, k, max_dist_dev,
                           out_instance_dev, out_shape_dev, out_dist_dev, mk);
    } else {
        hipLaunchKernelGGL((k_instances_knearest_tree<T, false>), grid, dim3(bs), lds, st, s->top->nodes.as<Node>(), (uint32_t)s->top->n_nodes,
                           s->knt_members.as<InstTreeMember<T>>(), s->recs.as<InstRec<T>>(), s->xforms.as<T>(), points_dev, (uint32_t)n, k, max_dist_dev,
                           out_instance_dev, out_shape_dev, out_dist_dev, InstMasks{nullptr, nullptr});
    }
    BVH_HIP(hipGetLastError());
}
template void instances_knearest_tree_batch<float>(bvhgpu_instances*, const float*, size_t, uint32_t, const float*, uint32_t*, uint32_t*, float*, bool,
                                                   const uint32_t*);
template void instances_knearest_tree_batch<double>(bvhgpu_instances*, const double*, size_t, uint32_t, const double*, uint32_t*, uint32_t*, double*, bool,
                                                    const uint32_t*);

}  // namespace bvhgpu
