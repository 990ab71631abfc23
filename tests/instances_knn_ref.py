"""Reference for the k-nearest point queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_knearest_*): the definition
restated in Python over tests/instances_ref.py's Scene (its x, y, top, flats), tests/knn_ref.py's distances and lists and
tests/instances_within_ref.py's stretch and world triangles, in the set's dtype T with one rounded operation per step; not a test file.

Per point p a list L of at most k triples (d, instance, shape), ascending in d, the squared world distance; full = len(L) == k,
bound = L[last].d; every comparison is the strict < of T; insertion is knn_ref.walk's.
  top level (the FlatNode array over the world boxes, with p):
    non-leaf entry: md = aabb.min_distance_squared(p); entry_index iff not full or md < bound, else exit_index
    leaf entry (instance i): walk instance i, then exit_index
  instance i (member t = tree_of[i]):
    q = forward(Y_i, p);  F = stretch(Y_i);  member t's FlatNode array with q:
    non-leaf entry: entered iff not full or md < bound * F (one multiplication in T, made again whenever bound changes and on entry)
    leaf entry (shape s): d = triangle_dist2(forward(X_i, tri_s), p) — the WORLD triangle and the WORLD point; accepted iff not full or
    d < bound
`brute` is the same insertion over ALL (instance, shape) pairs in the double order with no tree and no object frame."""
import numpy as np

import instances_ref as ir
import instances_within_ref as iwr
import knn_ref as kr

NONE = kr.NONE


def _offer(ld, li, ls, k, d, i, s):
    """knn_ref.walk's acceptance and insertion for one candidate → True iff the list changed"""
    full = len(ld) == k
    if full and not d < ld[-1]:
        return False
    if full:
        ld.pop(); li.pop(); ls.pop()
    pos = len(ld)
    for j, e in enumerate(ld):
        if d < e:
            pos = j
            break
    ld.insert(pos, d); li.insert(pos, i); ls.insert(pos, s)
    return True


def _points(sc, points):
    return np.ascontiguousarray(points, dtype=sc.ft).reshape(-1, 3)


class _Dists:
    """the distances of one (scene, points) pair, each computed once and shared by every k: d(j)[i][s] of point j to world triangle
    (i, s), and md(j, i)[e] of its object-frame image to entry e of instance i's member array.  `cache` (a dict the caller keeps
    for ONE scene and ONE array of points) carries them from call to call"""

    def __init__(self, sc, pts, cache):
        self.sc, self.pts, self.c = sc, pts, cache if cache is not None else {}
        if "wtris" not in self.c:
            wt = iwr.world_triangles(sc)
            self.c["wtris"] = np.ascontiguousarray(np.concatenate(wt)) if wt else np.zeros((0, 3, 3), dtype=sc.ft)
            self.c["cuts"] = np.cumsum([len(w) for w in wt])[:-1].tolist()
            self.c["F"] = [sc.ft(iwr.stretch(y)) for y in sc.y]
        self.big_f = self.c["F"]

    def d(self, j):
        key = ("d", j)
        if key not in self.c:   # (triangle_dist2_v is element-wise: all instances' triangles in one call give the same bits)
            dd = kr.triangle_dist2_v(self.c["wtris"], self.pts[j]).astype(self.sc.ft)
            self.c[key] = [a.tolist() for a in np.split(dd, self.c["cuts"])]
        return self.c[key]

    def md(self, j, i):
        key = ("md", j, i)
        if key not in self.c:
            sc = self.sc
            flat = sc.flats[int(sc.tree_of[i])]
            q = ir.forward(sc.y[i], self.pts[j]).astype(sc.ft)
            self.c[key] = kr.aabb_min_dist2_v(np.ascontiguousarray(flat["min"]), np.ascontiguousarray(flat["max"]), q).astype(sc.ft).tolist()
        return self.c[key]


def rows(sc, points, k, stats=None, cache=None):
    """the definition for every point → per point the list [(d, instance, shape)], at most k long.  stats (a dict, optional) receives
    `instances` (instances entered), `entries` (member entries visited) and `leaves` (member leaves offered) summed over the batch"""
    ft = sc.ft
    pts = _points(sc, points)
    out = [[] for _ in pts]
    n_inst = n_entries = n_leaves = 0
    if len(sc.x) == 0:
        return out
    t_entry, t_exit, t_shape = kr.flat_lists(sc.top)
    member_lists = [kr.flat_lists(f) for f in sc.flats]
    with np.errstate(all="ignore"):
        g = _Dists(sc, pts, cache)
        big_f = g.big_f
        top_mn, top_mx = np.ascontiguousarray(sc.top["min"]), np.ascontiguousarray(sc.top["max"])
        for j, p in enumerate(pts):
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
                n_inst += 1
                md, d = g.md(j, i), dj[i]
                entry, exit_, shape = member_lists[int(sc.tree_of[i])]
                full = len(ld) == k
                lim = ft(ft(ld[-1]) * big_f[i]).item() if full else None      # bound * F on entry to the instance
                e, ne = 0, len(entry)
                while e < ne:
                    n_entries += 1
                    if entry[e] == NONE:
                        s = shape[e]
                        n_leaves += 1
                        if _offer(ld, li, ls, k, d[s], i, s):
                            full = len(ld) == k
                            if full:
                                lim = ft(ft(ld[-1]) * big_f[i]).item()        # ... and whenever bound changes
                        e = exit_[e]
                    else:
                        e = entry[e] if (not full or md[e] < lim) else exit_[e]
            out[j] = list(zip(ld, li, ls))
    if stats is not None:
        stats["instances"] = n_inst
        stats["entries"] = n_entries
        stats["leaves"] = n_leaves
    return out


def brute(sc, points, k, cache=None):
    """per point the list built by offering every (instance, shape) pair in the double order — knn_ref.leaf_preorder of the top level, then
    of the member — with no tree"""
    pts = _points(sc, points)
    out = [[] for _ in pts]
    if len(sc.x) == 0:
        return out
    inst_order = kr.leaf_preorder(sc.top)
    shape_order = [kr.leaf_preorder(f) for f in sc.flats]
    with np.errstate(all="ignore"):
        g = _Dists(sc, pts, cache)
        for j in range(len(pts)):
            dj = g.d(j)
            ld, li, ls = [], [], []
            for i in inst_order:
                d = dj[i]
                for s in shape_order[int(sc.tree_of[i])]:
                    _offer(ld, li, ls, k, d[s], i, s)
            out[j] = list(zip(ld, li, ls))
    return out


def padded(list_rows, k, dtype):
    """rows → (instance[n, k] u32, shape[n, k] u32, dist[n, k]) as bvhgpu_instances_knearest_* writes them"""
    n = len(list_rows)
    inst = np.full((n, k), NONE, dtype=np.uint32)
    shape = np.full((n, k), NONE, dtype=np.uint32)
    dist = np.full((n, k), np.inf, dtype=dtype)
    with np.errstate(invalid="ignore"):
        for j, r in enumerate(list_rows):
            m = len(r)
            inst[j, :m] = [e[1] for e in r]
            shape[j, :m] = [e[2] for e in r]
            dist[j, :m] = np.sqrt(np.asarray([e[0] for e in r], dtype=dtype))
    return inst, shape, dist


def knearest(sc, points, k):
    return padded(rows(sc, points, k), k, sc.ft)


def same_rows(a, b) -> bool:
    """two lists of rows are equal element for element (two NaN distances are equal)"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if len(ra) != len(rb):
            return False
        for (da, ia, sa), (db, ib, sb) in zip(ra, rb):
            if ia != ib or sa != sb or not (da == db or (da != da and db != db)):
                return False
    return True
