"""The definition of bvhgpu_knearest_tree_* (include/bvh_mi355x.h) restated in Python over the oracle's BvhNode array
(orc.build(aabbs).nodes); not a test file, tests/test_knn_tree_cpu.py and tests/test_gpu_knn_tree.py import it.

It is BvhNode::nearest_to_recursive (bvh_node.rs:327-374) with knn_ref's list L of at most k pairs (dist2, shape) in place of
best_candidate and an optional limit per point, m = max_dist[i]:
  full = len(L) == k, bound = L[last].dist2, r2 = m * m (one multiplication in the tree's dtype)
  admit(x) = (max_dist is None or (m >= 0 and x <= r2)) and (not full or x < bound)
  visit(node), from node 0:
    leaf:  d = shape.distance_squared(p); if admit(d): drop L[last] of a full list, insert (d, shape) in front of the first e with
           d < e.dist2, else at the end
    inner: c = [(l, l_aabb.min_distance_squared(p)), (r, r_aabb.min_distance_squared(p))]; if c[0].1 > c[1].1: swap;
           for (idx, cd) in c: if admit(cd): visit(idx)          (the second test sees the list as the first subtree left it)
  row: knn_ref.row — shape[j] = L[j].shape, dist[j] = sqrt(L[j].dist2); the other slots are NONE and +inf.

The distances are knn_ref's vectorised ones (tests/test_knn_cpu.py proves them bit-equal to the oracle's scalar ones), applied to the
records' l_min / l_max / r_min / r_max.  The recursion is written with an explicit stack of pending (child, distance) pairs that are
tested when they are popped — for the second child that is after the first subtree has returned — so a chain of any depth works."""
import numpy as np

import knn_ref as kr

NONE = kr.NONE


def dists_vector(nodes, shape_aabbs, p, dtype, tris=None):
    """(dl[n_nodes], dr[n_nodes]: min_distance_squared of every record's two child boxes (leaf records: never read), d[n_shapes])"""
    p = np.asarray(p, dtype=dtype)
    with np.errstate(all="ignore"):
        dl = kr.aabb_min_dist2_v(np.ascontiguousarray(nodes["l_min"]), np.ascontiguousarray(nodes["l_max"]), p)
        dr = kr.aabb_min_dist2_v(np.ascontiguousarray(nodes["r_min"]), np.ascontiguousarray(nodes["r_max"]), p)
        if tris is not None:
            d = kr.triangle_dist2_v(np.asarray(tris, dtype=dtype).reshape(-1, 3, 3), p)
        else:
            sa = np.asarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
            d = kr.aabb_min_dist2_v(sa[:, :3], sa[:, 3:], p)
    return dl.astype(dtype, copy=False), dr.astype(dtype, copy=False), d.astype(dtype, copy=False)


def tree_lists(nodes):
    return nodes["l"].tolist(), nodes["r"].tolist(), nodes["shape"].tolist()


def walk(lists, dl, dr, d, k, r2=None):
    """one query: the list L as ([dist2], [shape]).  lists = (l, r, shape) as Python lists; dl, dr, d as Python lists of floats (an f32
    widens to a Python float exactly, so the comparisons see the same values); r2: None = no limit"""
    l, r, shape = lists
    ld, ls = [], []

    def admit(x):
        return (r2 is None or x <= r2) and (len(ld) < k or x < ld[-1])

    stack = [(0, None)]                                           # the root is visited untested
    while stack:
        idx, cd = stack.pop()
        if cd is not None and not admit(cd):
            continue
        s = shape[idx]
        if s != NONE:
            ds = d[s]
            if admit(ds):
                if len(ld) == k:
                    ld.pop(); ls.pop()
                pos = len(ld)
                for j, e in enumerate(ld):
                    if ds < e:
                        pos = j
                        break
                ld.insert(pos, ds); ls.insert(pos, s)
        else:
            a, b = (l[idx], dl[idx]), (r[idx], dr[idx])
            if a[1] > b[1]:                                     # strict >: ties and NaN keep the left child first
                a, b = b, a
            stack.append(b)
            stack.append(a)
    return ld, ls


def limits(max_dist, n, dtype):
    """max_dist (None, a scalar or n values) → per point None (no limit), False (a negative or NaN limit: nothing is admitted) or r2"""
    if max_dist is None:
        return [None] * n
    m = np.broadcast_to(np.asarray(max_dist, dtype=dtype), (n,))
    with np.errstate(all="ignore"):
        r2 = (m * m).astype(dtype)                                 # one multiplication in T
    return [r2[i].item() if m[i] >= 0 else False for i in range(n)]


def knearest_tree_limits(nodes, shape_aabbs, points, ks, tris=None, limit_sets=(None,)):
    """the definition for every point, every k of `ks` and every max_dist of `limit_sets` (None, a scalar or n values each; the distances
    of a point are computed once for all of them) → [{k: (shape[n, k] u32, dist[n, k])} per limit set]; dtype = the node array's"""
    dtype = nodes["l_min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=dtype).reshape(-1, 3, 3)
    outs = [{k: (np.full((len(pts), k), NONE, dtype=np.uint32), np.full((len(pts), k), np.inf, dtype=dtype)) for k in ks} for _ in limit_sets]
    if len(nodes) == 0:
        return outs
    tl = tree_lists(nodes)
    lims = [limits(m, len(pts), dtype) for m in limit_sets]
    for i, p in enumerate(pts):
        if all(lim[i] is False for lim in lims):
            continue
        dl, dr, d = dists_vector(nodes, sa, p, dtype, t)
        dll, drl, dsl = dl.tolist(), dr.tolist(), d.tolist()
        for out, lim in zip(outs, lims):
            if lim[i] is False:
                continue
            for k in ks:
                out[k][0][i], out[k][1][i] = kr.row(*walk(tl, dll, drl, dsl, k, lim[i]), k, dtype)
    return outs


def knearest_tree(nodes, shape_aabbs, points, ks, tris=None, max_dist=None):
    """one max_dist → {k: (shape[n, k] u32, dist[n, k])}"""
    return knearest_tree_limits(nodes, shape_aabbs, points, ks, tris, (max_dist,))[0]
