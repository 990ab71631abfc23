"""Reference for the nearest-first k-nearest point queries over instanced scenes (include/bvh_mi355x.h,
bvhgpu_instances_knearest_tree_*): the definition restated in Python over tests/instances_ref.py's Scene (its x, y, w, trees), the oracle's
BvhNode arrays (orc.build(aabbs).nodes of every member, orc.build(sc.w).nodes of the top level) and tests/instances_knn_ref.py's distances,
insertion and padding, in the set's dtype T with one rounded operation per step; not a test file.

For one query point p, L is a list of at most k triples (d, instance, shape); d is the squared WORLD distance in T.
  full = len(L) == k;  bound = L[last].d;  with a limit m = max_dist[j], r2 = m * m is one multiplication in T
  insertion: knn_ref.walk's — a full list drops its last element, the new one goes in front of the first e with d < e.d, else at the end
  every comparison is T's <, > or <= as written; a row that holds a NaN need not be sorted
  cmd(box, x)   = 0 if box.min[0] > box.max[0]         (a child of a split without SAH winner carries Aabb::empty(): nothing is known below it)
                  else box.min_distance_squared(x)
  admit_w(x)    = (max_dist is None or (m >= 0 and x <= r2))     and (not full or x < bound)       a leaf's d, world frame
  admit_b(x, F) = (max_dist is None or (m >= 0 and x <= r2 * F)) and (not full or x < bound * F or bound * F == +inf)
                  a child box: F = 1 at the top level (world frame: the products are r2 and bound themselves), F of the instance the
                  walk is in below it (object frame).  A bound or a product that is +inf — a list that holds an infinite distance, or
                  bound * F overflowing — says nothing about a box whose own distance overflowed as well, so it prunes nothing
  top(node) over the top level's BvhNode array, root = node 0, with p:
    Leaf{shape = i}:  enter instance i
    Node{l, l_aabb, r, r_aabb}:  c = [(l, cmd(l_aabb, p)), (r, cmd(r_aabb, p))];  if c[0].1 > c[1].1: swap   (strict >: ties and NaN keep left first)
                                 for (idx, cd) in c: if admit_b(cd, 1): top(idx)   (the second test sees the list as the first subtree left it)
  instance i (member t = tree_of[i]):
    q = forward(Y_i, p);  F = stretch(Y_i);  member(node) over member t's BvhNode array, root = node 0, with q:
      Leaf{shape = s}:  d = triangle_dist2(forward(X_i, tri_s), p) — the WORLD triangle and the WORLD point;  if admit_w(d): insert (d, i, s)
      Node{...}:        as above with cmd(., q) and admit_b(., F)
  r2 * F is one multiplication in T, made on entry to the instance; bound * F is one multiplication in T, made on entry and whenever bound
  changes (here: whenever it is read — the same two operands give the same product).
  A negative or NaN max_dist[j], a set without instances and a member without shapes give an empty list; a limit of 0 keeps only distance 0.

The order of a node's two children depends on the distances alone, never on the list, so without prunes the walk visits all
(instance, shape) pairs in one fixed order per point: the nearest-first order.  `rows` is the descent with its prunes; `ordered_brute` is
the same insertion over ALL pairs in that order with no box test at all, only the leaf's admit_w."""
import numpy as np

import instances_knn_ref as ikr
import instances_ref as ir
import knn_ref as kr
import knn_tree_ref as ktr
from oracle import orc

NONE = kr.NONE
INF = float("inf")
padded = ikr.padded
same_rows = ikr.same_rows


def node_arrays(sc):
    """(top level's BvhNode array, [every member's]) of the scene's current pose; kept on the scene until it is posed again"""
    key = sc.w.tobytes()
    got = sc.__dict__.get("_knn_tree_nodes")
    if got is None or got[0] != key:
        got = (key, orc.build(sc.w).nodes, [orc.build(a).nodes for a, _ in sc.trees])
        sc.__dict__["_knn_tree_nodes"] = got
    return got[1], got[2]


def has_empty_child(nodes):
    """an inner record carries Aabb::empty() (+inf / -inf) as a child box: the split had no SAH winner"""
    inner = nodes["shape"] == NONE
    return bool((np.isposinf(nodes["l_min"][inner]).all(axis=1) & np.isneginf(nodes["l_max"][inner]).all(axis=1)).any())


def _cmd(nodes, x):
    """(cmd of every record's left child box, of its right child box) for the point x, as lists of floats"""
    out = []
    for mn, mx in (("l_min", "l_max"), ("r_min", "r_max")):
        lo, hi = np.ascontiguousarray(nodes[mn]), np.ascontiguousarray(nodes[mx])
        md = kr.aabb_min_dist2_v(lo, hi, x).astype(lo.dtype)
        out.append(np.where(lo[:, 0] > hi[:, 0], lo.dtype.type(0), md).tolist())
    return out


def _descend(lists, dl, dr, admit, leaf):
    """visit() from node 0: `admit(cd)` decides a child when its turn comes (None: no box test), `leaf(shape)` handles a leaf record.
    The recursion as an explicit stack of pending (child, distance) pairs, tested when they are popped → records visited"""
    l, r, shape = lists
    stack = [(0, None)]                                           # the root is visited untested
    seen = 0
    while stack:
        idx, cd = stack.pop()
        if cd is not None and admit is not None and not admit(cd):
            continue
        seen += 1
        s = shape[idx]
        if s != NONE:
            leaf(s)
        else:
            a, b = (l[idx], dl[idx]), (r[idx], dr[idx])
            if a[1] > b[1]:                                       # strict >: ties and NaN keep the left child first
                a, b = b, a
            stack.append(b)
            stack.append(a)
    return seen


def _walk(sc, points, k, max_dist, prune, stats, cache):
    ft = sc.ft
    pts = ikr._points(sc, points)
    out = [[] for _ in pts]
    n_inst = n_entries = n_leaves = 0
    if len(sc.x) == 0:
        return out
    lim = ktr.limits(max_dist, len(pts), ft)
    top, members = node_arrays(sc)
    top_lists = ktr.tree_lists(top)
    member_lists = [ktr.tree_lists(m) for m in members]
    with np.errstate(all="ignore"):
        g = ikr._Dists(sc, pts, cache)
        big_f = g.big_f
        for j, p in enumerate(pts):
            if lim[j] is False or len(top) == 0:
                continue
            r2 = lim[j]                                           # None: no limit
            dj = g.d(j)
            ld, li, ls = [], [], []

            def admit_w(x):
                return (r2 is None or x <= r2) and (len(ld) < k or x < ld[-1])

            def enter(i):
                nonlocal n_inst, n_entries, n_leaves
                t = int(sc.tree_of[i])
                nodes = members[t]
                if len(nodes) == 0:
                    return
                n_inst += 1
                key = ("knt_cmd", j, i)
                if key not in g.c:
                    g.c[key] = _cmd(nodes, ir.forward(sc.y[i], p).astype(ft))
                dl, dr = g.c[key]
                big = big_f[i]
                r2o = None if r2 is None else ft(ft(r2) * big).item()         # r2 * F: one multiplication in T
                d = dj[i]

                def admit_o(x):
                    if r2 is not None and not x <= r2o:
                        return False
                    if len(ld) < k:
                        return True
                    lim = ft(ft(ld[-1]) * big).item()                             # bound * F: one multiplication in T
                    return x < lim or lim == INF

                def leaf(s):
                    nonlocal n_leaves
                    n_leaves += 1
                    if admit_w(d[s]):
                        ikr._offer(ld, li, ls, k, d[s], i, s)

                n_entries += _descend(member_lists[t], dl, dr, admit_o if prune else None, leaf)

            def admit_top(x):
                return (r2 is None or x <= r2) and (len(ld) < k or x < ld[-1] or ld[-1] == INF)

            tl, tr = _cmd(top, p)
            _descend(top_lists, tl, tr, admit_top if prune else None, enter)
            out[j] = list(zip(ld, li, ls))
    if stats is not None:
        stats["instances"] = n_inst
        stats["entries"] = n_entries
        stats["leaves"] = n_leaves
    return out


def rows(sc, points, k, max_dist=None, stats=None, cache=None):
    """the definition for every point → per point the list [(d, instance, shape)], at most k long.  max_dist: None, a scalar or one value
    per point.  stats (a dict, optional) receives `instances` (instances entered), `entries` (member records visited) and `leaves` (member
    leaves offered) summed over the batch; cache: instances_knn_ref._Dists' dict for ONE scene and ONE array of points"""
    return _walk(sc, points, k, max_dist, True, stats, cache)


def ordered_brute(sc, points, k, max_dist=None, stats=None, cache=None):
    """per point the list built by offering EVERY (instance, shape) pair in the nearest-first order: no box test, only the leaf's admit_w"""
    return _walk(sc, points, k, max_dist, False, stats, cache)


def knearest_tree(sc, points, k, max_dist=None):
    return padded(rows(sc, points, k, max_dist), k, sc.ft)


def special_limits(n, dtype):
    """the mix of limits no draw produces: 0, negative, NaN, +inf and one ordinary value, in turn"""
    return np.asarray([0.0, -1.0, np.nan, np.inf, 2.5])[np.arange(n) % 5].astype(dtype)


# ---------------------------------------------------------------- scenes with a split without SAH winner (shared by the CPU and GPU tests)
def far_member_scene(dtype):
    """one instance of test_within_cpu.far_scene's member (boxes so far apart that no bucket wins a split: both children of the root carry
    Aabb::empty()) under a non-uniform, mirrored scaling → (scene, member (aabbs, tris), x, points)"""
    from test_within_cpu import far_scene
    far, tris, pts, _ = far_scene(dtype)
    x = np.eye(3, 4, dtype=dtype)[None].copy()
    x[0, 0, 0], x[0, 1, 1] = 0.5, -2.0
    sc = ir.Scene([(far, tris)], [0], x, dtype)
    wt = ir.forward(sc.x[0], tris.reshape(-1, 3)).reshape(-1, 3, 3).astype(dtype)
    return sc, (far, tris), x, _far_points(pts, wt, wt)


def coincident_scene(dtype):
    """three instances of that member, two of whose world boxes coincide (a translation of 1 vanishes at 1e19): the top level's split has
    no SAH winner either → (scene, member, x, points)"""
    from test_within_cpu import far_scene
    far, tris, pts, _ = far_scene(dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (3, 1, 1))
    x[1, :, 3] = [1, 2, 3]
    x[2, 0, 0] = 0.5
    sc = ir.Scene([(far, tris)], [0, 0, 0], x, dtype)
    wt = [ir.forward(sc.x[i], tris.reshape(-1, 3)).reshape(-1, 3, 3).astype(dtype) for i in (0, 2)]
    return sc, (far, tris), x, _far_points(pts, wt[0], wt[1])


def _far_points(pts, wt_a, wt_b):
    """random points and points on world vertices"""
    return np.ascontiguousarray(np.concatenate([pts[:150], wt_a[:50, 0], wt_b[100:150, 1]]))
