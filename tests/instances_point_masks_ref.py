"""Reference for the masked point and region queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_within_masked_*,
_knearest_masked_*, _knearest_tree_masked_*, _region_masked_*); not a test file.  Instance i is visible to row j iff
(M[i] & P[j]) != 0, with M the set's masks and P the batch's (None: all ones).
  within         instances_within_ref.rows' row with the pairs of invisible instances removed
  region         instances_region_ref.reference's rows with the pairs of invisible instances removed
  knearest       instances_knn_ref.rows' loop — the incremental list, strict <, its prunes — restated with ONE addition: a top-level leaf
                 whose instance is invisible is passed over (exit_index, nothing offered)
  knearest_tree  instances_knn_tree_ref._walk's descent restated with ONE addition: `enter` returns at once for an invisible instance, as it
                 does for a member without shapes — the same top-level BvhNode array, the same order
Each has a brute force that builds no tree: all visible (instance, triangle) pairs in the family's order."""
import numpy as np

import instances_knn_ref as ikr
import instances_knn_tree_ref as iktr
import instances_ref as ir
import instances_region_ref as irr
import instances_within_ref as iwr
import knn_ref as kr
import knn_tree_ref as ktr
import region_ref as rr

NONE = kr.NONE
ALL = 0xFFFFFFFF


def row_masks(mask, n):
    """None / a scalar / n values → uint32[n]"""
    if mask is None:
        return np.full(n, ALL, dtype=np.uint32)
    r = np.asarray(mask)
    return np.full(n, int(r), dtype=np.uint32) if r.ndim == 0 else np.ascontiguousarray(r, dtype=np.uint32).reshape(n)


def _vis(M, P, n):
    """→ vis[j][i] as a bool array (n rows x instances)"""
    M = np.asarray(M, dtype=np.uint32)
    return (M[None, :] & row_masks(P, n)[:, None]) != 0


# ---- within ------------------------------------------------------------------------------------------------------------------------------
def within_filter(rows, M, P):
    """rows of instances_within_ref.rows (per point [(d, instance, shape)] in the double order) → the same without invisible instances"""
    vis = _vis(M, P, len(rows))
    return [[e for e in r if vis[j, e[1]]] for j, r in enumerate(rows)]


def within_brute(sc, points, max_dist, M, P):
    """per point the set {(instance, shape) : visible, d <= r2} over all pairs, no tree"""
    sets = iwr.brute(sc, points, max_dist)
    vis = _vis(M, P, len(sets))
    return [set(e for e in s if vis[j, e[0]]) for j, s in enumerate(sets)]


# ---- knearest (the flat form) ------------------------------------------------------------------------------------------------------------
def knn_rows(sc, points, k, M, P, cache=None):
    """instances_knn_ref.rows with the leaf skip → per point the list [(d, instance, shape)], at most k long"""
    ft = sc.ft
    pts = ikr._points(sc, points)
    out = [[] for _ in pts]
    if len(sc.x) == 0:
        return out
    vis = _vis(M, P, len(pts))
    t_entry, t_exit, t_shape = kr.flat_lists(sc.top)
    member_lists = [kr.flat_lists(f) for f in sc.flats]
    with np.errstate(all="ignore"):
        g = ikr._Dists(sc, pts, cache)
        big_f = g.big_f
        top_mn, top_mx = np.ascontiguousarray(sc.top["min"]), np.ascontiguousarray(sc.top["max"])
        for j, p in enumerate(pts):
            if not vis[j].any():
                continue                                          # (no instance is visible: an empty list whatever the walk does)
            mdt = kr.aabb_min_dist2_v(top_mn, top_mx, p).astype(ft).tolist()
            dj = g.d(j)
            ld, li, ls = [], [], []
            a, na = 0, len(t_entry)
            while a < na:
                if t_entry[a] != NONE:
                    a = t_entry[a] if (len(ld) < k or mdt[a] < ld[-1]) else t_exit[a]
                    continue
                i = t_shape[a]
                a = t_exit[a]
                if not vis[j, i]:
                    continue                                      # THE addition: a hidden instance offers nothing
                md, d = g.md(j, i), dj[i]
                entry, exit_, shape = member_lists[int(sc.tree_of[i])]
                full = len(ld) == k
                lim = ft(ft(ld[-1]) * big_f[i]).item() if full else None
                e, ne = 0, len(entry)
                while e < ne:
                    if entry[e] == NONE:
                        s = shape[e]
                        if ikr._offer(ld, li, ls, k, d[s], i, s):
                            full = len(ld) == k
                            if full:
                                lim = ft(ft(ld[-1]) * big_f[i]).item()
                        e = exit_[e]
                    else:
                        e = entry[e] if (not full or md[e] < lim) else exit_[e]
            out[j] = list(zip(ld, li, ls))
    return out


def knn_brute(sc, points, k, M, P, cache=None):
    """per point the first k of the STABLE ascending sort of all visible (instance, shape) pairs listed in the double order (no NaN among
    the distances of these scenes), no tree"""
    pts = ikr._points(sc, points)
    out = [[] for _ in pts]
    if len(sc.x) == 0:
        return out
    vis = _vis(M, P, len(pts))
    inst_order = kr.leaf_preorder(sc.top)
    shape_order = [kr.leaf_preorder(f) for f in sc.flats]
    with np.errstate(all="ignore"):
        g = ikr._Dists(sc, pts, cache)
        for j in range(len(pts)):
            dj = g.d(j)
            pairs = [(dj[i][s], i, s) for i in inst_order if vis[j, i] for s in shape_order[int(sc.tree_of[i])]]
            assert all(e[0] == e[0] for e in pairs)
            out[j] = sorted(pairs, key=lambda e: e[0])[:k]        # (sorted() is stable)
    return out


# ---- knearest_tree (the tree form) -------------------------------------------------------------------------------------------------------
def knn_tree_rows(sc, points, k, M, P, max_dist=None, cache=None, prune=True):
    """instances_knn_tree_ref._walk with the leaf skip; prune=False: every visible pair in the nearest-first order, only the leaf's admit_w"""
    ft = sc.ft
    pts = ikr._points(sc, points)
    out = [[] for _ in pts]
    if len(sc.x) == 0:
        return out
    vis = _vis(M, P, len(pts))
    lim = ktr.limits(max_dist, len(pts), ft)
    top, members = iktr.node_arrays(sc)
    top_lists = ktr.tree_lists(top)
    member_lists = [ktr.tree_lists(m) for m in members]
    with np.errstate(all="ignore"):
        g = ikr._Dists(sc, pts, cache)
        big_f = g.big_f
        for j, p in enumerate(pts):
            if lim[j] is False or len(top) == 0:
                continue
            r2 = lim[j]
            dj = g.d(j)
            ld, li, ls = [], [], []

            def admit_w(x):
                return (r2 is None or x <= r2) and (len(ld) < k or x < ld[-1])

            def enter(i):
                if not vis[j, i]:
                    return                                        # THE addition: as for a member without shapes
                t = int(sc.tree_of[i])
                nodes = members[t]
                if len(nodes) == 0:
                    return
                key = ("knt_cmd", j, i)
                if key not in g.c:
                    g.c[key] = iktr._cmd(nodes, ir.forward(sc.y[i], p).astype(ft))
                dl, dr = g.c[key]
                big = big_f[i]
                r2o = None if r2 is None else ft(ft(r2) * big).item()
                d = dj[i]

                def admit_o(x):
                    if r2 is not None and not x <= r2o:
                        return False
                    if len(ld) < k:
                        return True
                    lm = ft(ft(ld[-1]) * big).item()
                    return x < lm or lm == iktr.INF

                def leaf(s):
                    if admit_w(d[s]):
                        ikr._offer(ld, li, ls, k, d[s], i, s)

                iktr._descend(member_lists[t], dl, dr, admit_o if prune else None, leaf)

            def admit_top(x):
                return (r2 is None or x <= r2) and (len(ld) < k or x < ld[-1] or ld[-1] == iktr.INF)

            tl, tr = iktr._cmd(top, p)
            iktr._descend(top_lists, tl, tr, admit_top if prune else None, enter)
            out[j] = list(zip(ld, li, ls))
    return out


def knn_tree_brute(sc, points, k, M, P, max_dist=None, cache=None):
    return knn_tree_rows(sc, points, k, M, P, max_dist, cache, prune=False)


padded = ikr.padded


# ---- region ------------------------------------------------------------------------------------------------------------------------------
def _csr_filter(off, keep, *cols):
    n = len(off) - 1
    row = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    out = np.zeros(n + 1, dtype=np.uint32)
    out[1:] = np.cumsum(np.bincount(row[keep], minlength=n)).astype(np.uint32)
    return (out,) + tuple(np.ascontiguousarray(c[keep]) for c in cols)


def region_filter(ref, M, P):
    """instances_region_ref.reference's answers → dict(top=(offsets, instance, inside), full=(offsets, instance, shape, inside)) without
    the pairs of invisible instances"""
    M = np.asarray(M, dtype=np.uint32)
    out = {}
    for name in ("top", "full"):
        off, inst = ref[name][0], ref[name][1]
        n = len(off) - 1
        Pq = row_masks(P, n)
        row = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        keep = (M[inst.astype(np.int64)] & Pq[row]) != 0 if len(inst) else np.zeros(0, dtype=bool)
        out[name] = _csr_filter(off, keep, *ref[name][1:])
    return out


def region_brute(sc, planes, M, P):
    """no tree: per region the visible instances in the top level's leaf order whose world box passes, each with the shapes in its member's
    leaf order whose own box passes the object-space planes → per region [(instance, inside, [(shape, inside)])]"""
    ft = sc.ft
    pl = rr._planes_in(planes, ft)
    n = len(pl)
    vis = _vis(M, P, n)
    inst_order = kr.leaf_preorder(sc.top)
    shape_order = [kr.leaf_preorder(f) for f in sc.flats]
    w = np.ascontiguousarray(sc.w, dtype=ft).reshape(-1, 6)
    out = []
    for q in range(n):
        row = []
        for i in inst_order:
            if not vis[q, i] or not rr.predicate(pl[q:q + 1], w[i:i + 1, :3], w[i:i + 1, 3:])[0]:
                continue
            t = int(sc.tree_of[i])
            boxes = np.ascontiguousarray(sc.trees[t][0], dtype=ft).reshape(-1, 6)
            opl = np.repeat(irr.object_planes(sc.x[i], pl[q])[None], len(boxes), axis=0)
            ok = rr.predicate(opl, boxes[:, :3], boxes[:, 3:])
            ins = rr.inside(opl, boxes[:, :3], boxes[:, 3:])
            row.append((i, int(rr.inside(pl[q:q + 1], w[i:i + 1, :3], w[i:i + 1, 3:])[0]), [(s, int(ins[s])) for s in shape_order[t] if ok[s]]))
        out.append(row)
    return out
