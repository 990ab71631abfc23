"""The sphere distance of bvhgpu_knearest_sphere_* / _knearest_tree_sphere_* / _within_sphere_* (include/bvh_mi355x.h)
restated in numpy, and the three families' definitions with it at the leaf; not a test file, tests/test_sphere_dist_cpu.py and
tests/test_gpu_sphere_dist.py import it.

The distance, every operation rounded once in the scene's dtype, in this order (one numpy ufunc each):
  f[k] = p[k] - c[k];  s2 = (f0*f0 + f1*f1) + f2*f2  (sphere_ref.dot3's order);  len = sqrt(s2);  g = len - r;  q = 0 if g < 0 else g;  d = q*q
A NaN stays NaN (g < 0 is false for it).  `sphere_dist2_v` applies them to all spheres at once, `sphere_dist2_s` to one sphere one numpy
scalar at a time; tests/test_sphere_dist_cpu.py proves the two bit-equal.

The loops are the existing references', which take distances as input: knn_ref.walk (through knn_ref.knearest(dists=...)),
knn_tree_ref.walk and within_ref.walk.  knn_tree_ref and within_ref compute their distances inside their drivers, so the drivers — not
the loops — are restated here with the sphere distance in place of the shape distance; the node distances stay knn_ref.aabb_min_dist2_v."""
import numpy as np

import knn_ref as kr
import knn_tree_ref as ktr
import within_ref as wr

NONE = kr.NONE


# ---------------------------------------------------------------- the distance
def sphere_dist2_v(spheres, p):
    """spheres (N, 4) {cx, cy, cz, r} and one point p (3,), all of one dtype -> d[N] in that dtype"""
    s = np.asarray(spheres)
    ft = s.dtype.type
    p = np.asarray(p, dtype=s.dtype)
    with np.errstate(all="ignore"):
        f = p[None, :] - s[:, :3]
        s2 = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]
        s2 = s2 + f[:, 2] * f[:, 2]
        ln = np.sqrt(s2)
        g = ln - s[:, 3]
        q = np.where(g < 0, ft(0), g)                         # keeps NaN
        return (q * q).astype(s.dtype, copy=False)


def sphere_dist2_s(sphere, p, dtype):
    """one sphere, one point: the same operations on numpy scalars of `dtype`"""
    ft = dtype
    c = [ft(sphere[0]), ft(sphere[1]), ft(sphere[2])]
    r = ft(sphere[3])
    with np.errstate(all="ignore"):
        f = [ft(ft(p[k]) - c[k]) for k in range(3)]
        x, y, z = ft(f[0] * f[0]), ft(f[1] * f[1]), ft(f[2] * f[2])
        s2 = ft(ft(x + y) + z)
        ln = ft(np.sqrt(s2))
        g = ft(ln - r)
        q = ft(0) if g < 0 else g
        return ft(q * q)


def dists(spheres):
    """a `dists` argument for knn_ref.knearest: node distances as knn_ref.dists_vector's, shape distances the spheres'"""
    def f(flat, shape_aabbs, p, dtype, tris=None):
        md, _ = kr.dists_vector(flat, shape_aabbs, p, dtype, None)
        return md, sphere_dist2_v(np.asarray(spheres, dtype=dtype).reshape(-1, 4), np.asarray(p, dtype=dtype))
    return f


# ---------------------------------------------------------------- the three families
def knearest(flat, shape_aabbs, spheres, points, ks):
    """bvhgpu_knearest_sphere_*: {k: (shape[n, k] u32, dist[n, k])}"""
    return kr.knearest(flat, shape_aabbs, points, ks, None, dists(spheres))


def knearest_tree_limits(nodes, shape_aabbs, spheres, points, ks, limit_sets=(None,)):
    """bvhgpu_knearest_tree_sphere_*: knn_tree_ref.knearest_tree_limits' driver with the sphere distance at the leaves"""
    dtype = nodes["l_min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    sp = np.ascontiguousarray(spheres, dtype=dtype).reshape(-1, 4)
    outs = [{k: (np.full((len(pts), k), NONE, dtype=np.uint32), np.full((len(pts), k), np.inf, dtype=dtype)) for k in ks} for _ in limit_sets]
    if len(nodes) == 0:
        return outs
    tl = ktr.tree_lists(nodes)
    lims = [ktr.limits(m, len(pts), dtype) for m in limit_sets]
    for i, p in enumerate(pts):
        if all(lim[i] is False for lim in lims):
            continue
        dl, dr, _ = ktr.dists_vector(nodes, sa, p, dtype, None)
        dll, drl, dsl = dl.tolist(), dr.tolist(), sphere_dist2_v(sp, p).tolist()
        for out, lim in zip(outs, lims):
            if lim[i] is False:
                continue
            for k in ks:
                out[k][0][i], out[k][1][i] = kr.row(*ktr.walk(tl, dll, drl, dsl, k, lim[i]), k, dtype)
    return outs


def knearest_tree(nodes, shape_aabbs, spheres, points, ks, max_dist=None):
    return knearest_tree_limits(nodes, shape_aabbs, spheres, points, ks, (max_dist,))[0]


def within_rows_multi(flat, shape_aabbs, spheres, points, limit_sets):
    """bvhgpu_within_sphere_*: within_ref.rows_multi's driver with the sphere distance at the leaves -> per limit set the rows in list
    order as ([dist2], [shape])"""
    dtype = flat["min"].dtype.type
    pts = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    sa = np.ascontiguousarray(shape_aabbs, dtype=dtype).reshape(-1, 6)
    sp = np.ascontiguousarray(spheres, dtype=dtype).reshape(-1, 4)
    outs = [[([], []) for _ in pts] for _ in limit_sets]
    if len(flat) == 0:
        return outs
    fl = kr.flat_lists(flat)
    lims = [wr.limits(m, len(pts), dtype) for m in limit_sets]
    for i, p in enumerate(pts):
        if all(lim[i] is False for lim in lims):
            continue
        md, _ = kr.dists_vector(flat, sa, p, dtype, None)
        mdl, dl = md.tolist(), sphere_dist2_v(sp, p).tolist()
        for out, lim in zip(outs, lims):
            if lim[i] is not False:
                out[i] = wr.walk(fl, mdl, dl, lim[i])
    return outs


def within_rows(flat, shape_aabbs, spheres, points, max_dist):
    return within_rows_multi(flat, shape_aabbs, spheres, points, (max_dist,))[0]


def within(flat, shape_aabbs, spheres, points, max_dist, sort=True):
    """(offsets, shape, dist) as bvhgpu_hits_fetch_within gives them"""
    return wr.csr(within_rows(flat, shape_aabbs, spheres, points, max_dist), flat["min"].dtype.type, sort)


def brute_rows(flat, spheres, points, k):
    """per point the first k of a STABLE sort by d of all spheres listed in leaf pre-order (rows with a NaN distance: None)"""
    dtype = flat["min"].dtype.type
    sp = np.ascontiguousarray(spheres, dtype=dtype).reshape(-1, 4)
    out = []
    for p in np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3):
        d = sphere_dist2_v(sp, p)
        out.append(None if np.isnan(d).any() else kr.brute_force(flat, d.tolist(), k))
    return out


# ---------------------------------------------------------------- the scenes the CPU and the GPU tests share
def inscribed(aabbs):
    """the sphere inscribed in every box: centre the box centre, radius half the shortest edge — every sphere lies inside its box"""
    a = np.asarray(aabbs)
    c = (a[:, :3] + a[:, 3:]) * a.dtype.type(0.5)
    r = (a[:, 3:] - a[:, :3]).min(axis=1) * a.dtype.type(0.5)
    return np.ascontiguousarray(np.concatenate([c, r[:, None]], axis=1))


def ball_scene(n, dtype, seed=7, dup_every=5):
    """n cubes of half edge 0.05 .. 0.6 in [-10, 10]^3 and the spheres inscribed in them; every `dup_every`-th shape is a copy of its
    predecessor, so equal distances straddle the k-th slot of many rows.  -> (spheres (n, 4), aabbs (n, 6))"""
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(-10, 10, size=(n, 3)).astype(dtype)
    r = rng.uniform(0.05, 0.6, size=(n, 1)).astype(dtype)
    a = np.ascontiguousarray(np.concatenate([c - r, c + r], axis=1))
    if n > dup_every:
        dst = np.arange(dup_every, n, dup_every)
        a[dst] = a[dst - 1]
    return inscribed(a), a


def enlarged(spheres, factor=6):
    """the same centres with radii `factor` times as large: the spheres reach far outside the boxes the tree was built from"""
    s = np.array(spheres, copy=True)
    s[:, 3] *= s.dtype.type(factor)
    return s


def query_points(spheres, dtype, n=300, seed=11):
    """n points: uniform over twice the scene's extent, inside balls, on their surfaces (up to rounding), at centres (ties between
    duplicates), and far outside"""
    rng = np.random.default_rng(seed)
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    if len(s) == 0:
        return rng.uniform(-20, 20, size=(n, 3)).astype(dtype)
    n_in, n_on, n_c, n_far = n // 6, n // 6, n // 10, n // 15
    parts = [rng.uniform(-20, 20, size=(n - n_in - n_on - n_c - n_far, 3))]
    u = rng.normal(size=(n_in + n_on, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pick = rng.integers(0, len(s), n_in + n_on)
    scale = np.concatenate([rng.uniform(0, 0.95, n_in), np.ones(n_on)])
    parts.append(s[pick, :3] + u * (s[pick, 3] * scale)[:, None])
    parts.append(s[rng.integers(0, len(s), n_c), :3])
    parts.append(rng.uniform(-1, 1, size=(n_far, 3)) * 1e4)
    return np.ascontiguousarray(np.concatenate(parts).astype(dtype))
