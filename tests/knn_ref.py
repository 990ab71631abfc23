"""The definition of bvhgpu_knearest_* (include/bvh_mi355x.h) restated in Python over the oracle's FlatNode array; not a test file,
tests/test_knn_cpu.py and tests/test_gpu_knn.py import it.

The loop is nearest_to's (flat_bvh.rs:524-558) with `best_element` replaced by a list L of at most k pairs (dist2, shape):
  full = len(L) == k, bound = L[last].dist2
  non-leaf entry: md = node.aabb.min_distance_squared(query); entry_index iff not full or md < bound, else exit_index
  leaf entry:     d = shape.distance_squared(query); accept iff not full or d < bound; on accept drop L[last] of a full list and insert
                  (d, shape) in front of the first element e with d < e.dist2, or at the end; then exit_index
  row: shape[j] = L[j].shape, dist[j] = sqrt(L[j].dist2); the other k - len(L) slots are NONE and +inf.

Two sources for the distances.  `dists_scalar`: one oracle call per distance (orc.aabb_min_dist2 / orc.triangle_dist2), every float the
oracle's — the authority, and slow.  `dists_vector`: the same operations in the same order in numpy, per query over all boxes / shapes at
once; tests/test_knn_cpu.py proves it bit-equal to the scalar form before anything relies on it."""
import numpy as np

from oracle import orc

NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- distances: scalar (the oracle's own)
def dists_scalar(flat, shape_aabbs, p, dtype, tris=None):
    """(md[n_flat]: Aabb::min_distance_squared of every non-leaf entry's box (0 at leaf entries, never read), d[n_shapes])"""
    md = np.zeros(len(flat), dtype=dtype)
    for i in range(len(flat)):
        if flat["entry"][i] != NONE:
            md[i] = orc.aabb_min_dist2(np.concatenate([flat["min"][i], flat["max"][i]]), p, dtype)
    n = len(shape_aabbs)
    d = np.zeros(n, dtype=dtype)
    for s in range(n):
        d[s] = orc.triangle_dist2(tris[s], p, dtype) if tris is not None else orc.aabb_min_dist2(shape_aabbs[s], p, dtype)
    return md, d


# ---------------------------------------------------------------- distances: numpy, same operation order
def _dot(a, b):
    s = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def aabb_min_dist2_v(mn, mx, p):
    """Aabb::min_distance_squared (aabb_impl.rs:618-629) for boxes mn / mx (N, 3) and one point p (3,), all of one dtype"""
    size = mx - mn
    half = size * mn.dtype.type(0.5)
    centre = mn + half
    delta = p[None, :] - centre
    q = np.abs(delta) - half
    out = np.where(q > 0, q, mn.dtype.type(0))           # x.max(0): NaN -> 0
    return _dot(out, out)


def _segment_v(p, a, b):
    ab, ap = b - a, p[None, :] - a
    m = _dot(ab, ab)
    s = _dot(ab, ap) / m
    s = np.where(s < 0, a.dtype.type(0), np.where(s > 1, a.dtype.type(1), s))   # clamp keeps NaN
    return a + s[:, None] * ab


def triangle_dist2_v(tris, p):
    """<Triangle as PointDistance>::distance_squared (testbase.rs:367-443) for triangles (N, 3, 3) and one point p (3,)"""
    ft = tris.dtype.type
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    ab_eq, bc_eq, ac_eq = (a == b).all(axis=1), (b == c).all(axis=1), (a == c).all(axis=1)
    ab, ac, ap = b - a, c - a, p[None, :] - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p[None, :] - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p[None, :] - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    v_ab = d1 / (d1 - d3)
    v_ac = d2 / (d2 - d6)
    v_bc = e43 / (e43 + e56)
    denom = ft(1) / ((va + vb) + vc)
    v, w = vb * denom, vc * denom
    conds = [ab_eq & bc_eq & ac_eq, ab_eq, bc_eq | ac_eq,
             (d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    vals = [a, _segment_v(p, a, c), _segment_v(p, a, b), a, b, c,
            a + v_ab[:, None] * ab, a + v_ac[:, None] * ac, b + v_bc[:, None] * (c - b),
            (a + v[:, None] * ab) + w[:, None] * ac]
    near = vals[-1]
    for cond, val in zip(reversed(conds), reversed(vals[:-1])):       # the first condition that holds wins
        near = np.where(cond[:, None], val, near)
    diff = p[None, :] - near
    return _dot(diff, diff)


def dists_vector(flat, shape_aabbs, p, dtype, tris=None):
    p = np.asarray(p, dtype=dtype)
    with np.errstate(all="ignore"):
        md = aabb_min_dist2_v(np.ascontiguousarray(flat["min"]), np.ascontiguousarray(flat["max"]), p)
        if tris is not None:
            d = triangle_dist2_v(np.asarray(tris, dtype=dtype).reshape(-1, 3, 3), p)
        else:
            sa = np.asarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
            d = aabb_min_dist2_v(sa[:, :3], sa[:, 3:], p)
    return md.astype(dtype, copy=False), d.astype(dtype, copy=False)


# ---------------------------------------------------------------- the loop
def walk(flat_lists, md, d, k):
    """one query: the list L as ([dist2], [shape]).  flat_lists = (entry, exit, shape) as Python lists; md, d as Python lists of floats
    (an f32 widens to a Python float exactly, so < compares the same values)"""
    entry, exit_, shape = flat_lists
    ld, ls = [], []
    i, n = 0, len(entry)
    while i < n:
        full = len(ld) == k
        if entry[i] == NONE:                                  # leaf entry
            s = shape[i]
            ds = d[s]
            if not full or ds < ld[-1]:
                if full:
                    ld.pop(); ls.pop()
                pos = len(ld)
                for j, e in enumerate(ld):
                    if ds < e:
                        pos = j
                        break
                ld.insert(pos, ds); ls.insert(pos, s)
            i = exit_[i]
        else:
            i = entry[i] if (not full or md[i] < ld[-1]) else exit_[i]
    return ld, ls


def flat_lists(flat):
    return flat["entry"].tolist(), flat["exit"].tolist(), flat["shape"].tolist()


def row(ld, ls, k, dtype):
    shape = np.full(k, NONE, dtype=np.uint32)
    dist = np.full(k, np.inf, dtype=dtype)
    shape[:len(ls)] = ls
    with np.errstate(invalid="ignore"):
        dist[:len(ld)] = np.sqrt(np.asarray(ld, dtype=dtype))
    return shape, dist


def knearest(flat, shape_aabbs, points, ks, tris=None, dists=dists_vector):
    """the definition for every point and every k of `ks` → {k: (shape[n, k] u32, dist[n, k])}; dtype = the flat array's"""
    dtype = flat["min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=dtype).reshape(-1, 3, 3)
    fl = flat_lists(flat)
    out = {k: (np.full((len(pts), k), NONE, dtype=np.uint32), np.full((len(pts), k), np.inf, dtype=dtype)) for k in ks}
    if len(flat) == 0:
        return out
    for r, p in enumerate(pts):
        md, d = dists(flat, sa, p, dtype, t)
        mdl, dl = md.tolist(), d.tolist()
        for k in ks:
            out[k][0][r], out[k][1][r] = row(*walk(fl, mdl, dl, k), k, dtype)
    return out


def leaf_preorder(flat):
    """shape indices in the order the loop meets their leaf entries when nothing is pruned"""
    return [int(s) for e, s in zip(flat["entry"], flat["shape"]) if e == NONE]


def brute_force(flat, d, k):
    """the first k of a STABLE sort by dist2 of all shapes listed in leaf pre-order (no NaN in d) → ([dist2], [shape])"""
    order = leaf_preorder(flat)
    dd = np.asarray([d[s] for s in order])
    idx = np.argsort(dd, kind="stable")[:k]
    return [dd[j].item() for j in idx], [order[j] for j in idx]


def same(a, b) -> bool:
    """byte equality, except that two NaNs are equal whatever their sign and payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn)) and a[~an].tobytes() == b[~bn].tobytes()
