"""The definition of bvhgpu_within_* (include/bvh_mi355x.h) restated in Python over the oracle's FlatNode array; not a test
file, tests/test_within_cpu.py, tests/test_gpu_within.py and tests/test_gpu_fuzz_within.py import it.

The loop is nearest_to's (flat_bvh.rs:524-558) with the moving best_dist replaced by a fixed limit: point p comes with m = max_dist,
r2 = m * m (one multiplication in the tree's dtype); a negative or NaN m gives an empty row without a walk.
  non-leaf entry: md = node.aabb.min_distance_squared(p); entry_index iff md <= r2, else exit_index
  leaf entry:     d = shape.distance_squared(p); candidate (d, shape) iff d <= r2; then exit_index
  row, sorted:     the candidates in a stable ascending sort by d (equal d in the order the loop met them), distance sqrt(d)
  row, list order: the candidates in the order the loop met them
The distances are knn_ref.dists_vector's (tests/test_knn_cpu.py proves them bit-equal to the oracle's scalar ones).

`tree_candidates` restates the same candidate set recursively over the oracle's BvhNode array — every child box on the way down passes
md <= r2, the shape passes d <= r2 — for the walk-independence check: the threshold never moves, so the order of the visit is free."""
import numpy as np

import knn_ref as kr
import knn_tree_ref as ktr

NONE = kr.NONE


def limits(max_dist, n, dtype):
    """max_dist (a scalar or n values) -> per point False (a negative or NaN limit: no walk) or r2 as a Python float"""
    return ktr.limits(max_dist, n, dtype)


def walk(flat_lists, md, d, r2):
    """one query: the candidates as ([dist2], [shape]) in the order the loop meets them.  flat_lists = (entry, exit, shape) as Python
    lists; md, d as Python lists of floats (an f32 widens to a Python float exactly, so <= compares the same values)"""
    entry, exit_, shape = flat_lists
    ld, ls = [], []
    i, n = 0, len(entry)
    while i < n:
        if entry[i] == NONE:                                  # leaf entry
            s = shape[i]
            if d[s] <= r2:
                ld.append(d[s]); ls.append(s)
            i = exit_[i]
        else:
            i = entry[i] if md[i] <= r2 else exit_[i]
    return ld, ls


def sort_row(ld, ls):
    """stable ascending sort by dist2 (no NaN among candidates: NaN <= r2 is false)"""
    order = sorted(range(len(ld)), key=ld.__getitem__)       # sorted() is stable
    return [ld[j] for j in order], [ls[j] for j in order]


def rows(flat, shape_aabbs, points, max_dist, tris=None):
    """the loop for every point -> list of ([dist2], [shape]) in list order; dtype = the flat array's"""
    dtype = flat["min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=dtype).reshape(-1, 3, 3)
    out = [([], []) for _ in pts]
    if len(flat) == 0:
        return out
    fl = kr.flat_lists(flat)
    lim = limits(max_dist, len(pts), dtype)
    for i, p in enumerate(pts):
        if lim[i] is False:
            continue
        md, d = kr.dists_vector(flat, sa, p, dtype, t)
        out[i] = walk(fl, md.tolist(), d.tolist(), lim[i])
    return out


def rows_multi(flat, shape_aabbs, points, limit_sets, tris=None):
    """rows() for several max_dist arguments at once (the distances of a point are computed once for all of them)"""
    dtype = flat["min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=dtype).reshape(-1, 3, 3)
    outs = [[([], []) for _ in pts] for _ in limit_sets]
    if len(flat) == 0:
        return outs
    fl = kr.flat_lists(flat)
    lims = [limits(m, len(pts), dtype) for m in limit_sets]
    for i, p in enumerate(pts):
        if all(lim[i] is False for lim in lims):
            continue
        md, d = kr.dists_vector(flat, sa, p, dtype, t)
        mdl, dl = md.tolist(), d.tolist()
        for out, lim in zip(outs, lims):
            if lim[i] is not False:
                out[i] = walk(fl, mdl, dl, lim[i])
    return outs


def csr(list_rows, dtype, sort=True):
    """rows in list order -> (offsets[n + 1] u32, shape[total] u32, dist[total]) as bvhgpu_hits_fetch_within gives them"""
    lens = [len(r[0]) for r in list_rows]
    offsets = np.zeros(len(list_rows) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64).astype(np.uint32)
    dd, ss = [], []
    for ld, ls in list_rows:
        if sort:
            ld, ls = sort_row(ld, ls)
        dd += ld; ss += ls
    return offsets, np.asarray(ss, dtype=np.uint32), np.sqrt(np.asarray(dd, dtype=dtype))


def within(flat, shape_aabbs, points, max_dist, tris=None, sort=True):
    return csr(rows(flat, shape_aabbs, points, max_dist, tris), flat["min"].dtype.type, sort)


def tree_candidates(nodes, shape_aabbs, points, max_dist, tris=None):
    """the recursive form over the BvhNode array -> per point the candidate set as a sorted list of (dist2, shape)"""
    dtype = nodes["l_min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=dtype).reshape(-1, 3, 3)
    out = [[] for _ in pts]
    if len(nodes) == 0:
        return out
    l, r, shape = ktr.tree_lists(nodes)
    lim = limits(max_dist, len(pts), dtype)
    for i, p in enumerate(pts):
        if lim[i] is False:
            continue
        r2 = lim[i]
        dl, dr, d = (a.tolist() for a in ktr.dists_vector(nodes, sa, p, dtype, t))
        got, stack = [], [0]                                  # the root is visited untested
        while stack:
            idx = stack.pop()
            s = shape[idx]
            if s != NONE:
                if d[s] <= r2:
                    got.append((d[s], s))
            else:                                             # right first, then left: ANY order gives the same set
                if dr[idx] <= r2:
                    stack.append(r[idx])
                if dl[idx] <= r2:
                    stack.append(l[idx])
        out[i] = sorted(got)
    return out


def head_rows(offsets, shape, dist, k):
    """the first k entries of every CSR row, padded with NONE / +inf: what bvhgpu_knearest_* rows look like"""
    n = len(offsets) - 1
    hs = np.full((n, k), NONE, dtype=np.uint32)
    hd = np.full((n, k), np.inf, dtype=dist.dtype)
    for i in range(n):
        b, e = int(offsets[i]), int(offsets[i + 1])
        m = min(k, e - b)
        hs[i, :m] = shape[b:b + m]
        hd[i, :m] = dist[b:b + m]
    return hs, hd


# ---------------------------------------------------------------- the scenes the CPU and the GPU tests share
def line_scene(dtype, copies=1, n_pos=4096, seed=5):
    """`copies` zero-size shapes at every integer x = 1 .. n_pos on a line (the shape index of a copy is a seeded permutation when
    copies > 1, so that leaf pre-order is not index order), as AABBs and as degenerate (point) triangles"""
    x = np.repeat(np.arange(1, n_pos + 1), copies)
    if copies > 1:
        x = x[np.random.default_rng(seed).permutation(len(x))]
    pts = np.zeros((len(x), 3), dtype=dtype)
    pts[:, 0] = x
    return np.concatenate([pts, pts], axis=1), np.repeat(pts[:, None, :], 3, axis=1)


LANE_MAX, LDS_MAX = 32, 2048                                  # bvh_amd/csrc/within.hip WITHIN_LANE_ROW_MAX / WITHIN_LDS_ROW_MAX


def row_length_limits():
    """integer limits whose rows on line_scene(copies=1) have every length 0 .. 300, 2^j - 1 / 2^j / 2^j + 1 up to 4096 and both tier
    thresholds +- 1"""
    want = set(range(301))
    for j in range(13):
        want |= {2 ** j - 1, 2 ** j, 2 ** j + 1}
    want |= {LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1}
    return sorted(v for v in want if v <= 4096)


def row_length_case(dtype, reverse):
    """(points, limits, lengths): forward, the queries sit at x = 0 and list order is distance order; reverse, at x = 4097 and list order
    is descending distance"""
    lens = np.asarray(row_length_limits())
    pts = np.zeros((len(lens), 3), dtype=dtype)
    pts[:, 0] = 4097 if reverse else 0
    return pts, lens.astype(dtype), lens
