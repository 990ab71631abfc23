"""The sphere leaf stage of bvhgpu_traverse_sphere_* (include/bvh_mi355x.h) restated in numpy, and the definition of the
closest / first sphere queries applied to a CSR.  Every operation below is one numpy ufunc on arrays of the scene's dtype: rounded once in
T, and numpy's separate ufuncs do not contract — the arithmetic the kernels run (walk.hpp ray_sphere).  tests/test_sphere_hit_cpu.py pins it
on hand-made rows; tests/test_gpu_sphere_hit.py compares the GPU against sphere_match byte for byte; tools/sphere_bench.py times it as the
host reduction a caller runs today."""
import numpy as np

NONE = 0xFFFFFFFF


def dot3(a, b):
    """(a0*b0 + a1*b1) + a2*b2 per row"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def ray_sphere(o, d, spheres):
    """the leaf stage per row: o[m,3], d[m,3], spheres[m,4] = {cx, cy, cz, r}, all of one dtype T → hit[m,2] = {distance, exit} in T;
    a miss is {+inf, 0}"""
    T = spheres.dtype.type
    assert o.dtype == d.dtype == spheres.dtype
    eps = T(np.finfo(T).eps)
    with np.errstate(all="ignore"):
        f = o - spheres[:, :3]
        a = dot3(d, d)
        tc = (-dot3(f, d)) / a                       # parameter of the ray's point nearest the centre
        l = f + tc[:, None] * d                      # centre → that point
        disc = spheres[:, 3] * spheres[:, 3] - dot3(l, l)
        h = np.sqrt(disc / a)
        t0 = tc - h
        t1 = tc + h
        t = np.where(t0 > eps, t0, t1)
        hit = (disc >= 0) & (t > eps)
    out = np.zeros((len(spheres), 2), dtype=T)
    out[:, 0] = np.where(hit, t, T(np.inf))
    out[:, 1] = np.where(hit, t1, T(0))
    assert out.dtype == T
    return out


def list_hits(off, idx, rays, spheres):
    """ray_sphere for every member of every row of the CSR: hit[total,2]"""
    counts = np.diff(off.astype(np.int64))
    row = np.repeat(np.arange(len(counts)), counts)
    T = spheres.dtype
    return ray_sphere(np.ascontiguousarray(rays["o"][row], dtype=T), np.ascontiguousarray(rays["d"][row], dtype=T),
                      np.ascontiguousarray(spheres[idx.astype(np.int64)]))


def sphere_match(off, idx, rays, spheres, tmax, first, hits=None):
    """the definition on a CSR (offsets, indices of FlatBvh::traverse's lists), the rays' records and the n x 4 spheres →
    (hit{distance,exit}[n,2], shape[n]).  A member is a candidate iff it hits and distance < tmax (strict, in T; tmax None = +inf); closest:
    the smallest distance, the first of the row on equal distances; first: the first candidate of the row; none: {+inf, 0} and NONE.
    hits: list_hits(off, idx, rays, spheres) where the caller has it already."""
    n = len(off) - 1
    T = spheres.dtype
    hits = list_hits(off, idx, rays, spheres) if hits is None else hits
    counts = np.diff(off.astype(np.int64))
    t = np.full(n, np.inf, dtype=T) if tmax is None else np.asarray(tmax, dtype=T)
    total = len(hits)
    starts = off[:-1].astype(np.int64)
    rows = counts > 0
    with np.errstate(invalid="ignore"):
        ok = hits[:, 0] < np.repeat(t, counts)                            # strict, in T: a miss (+inf) and a NaN tmax admit nothing
    if not first and total:                                               # closest: of the candidates, those with the row's smallest distance
        masked = np.where(ok, hits[:, 0], np.inf).astype(T)
        rowmin = np.full(n, np.inf, dtype=T)
        rowmin[rows] = np.minimum.reduceat(masked, starts[rows])
        ok = ok & (hits[:, 0] == np.repeat(rowmin, counts))
    pos = np.where(ok, np.arange(total), total)                           # ... and of those, the first of the list
    win = np.full(n, total, dtype=np.int64)
    if total:
        win[rows] = np.minimum.reduceat(pos, starts[rows])
    found = win < total
    out = np.zeros((n, 2), dtype=T)
    out[:, 0] = np.inf
    out[found] = hits[win[found]]
    shape = np.full(n, NONE, dtype=np.uint32)
    shape[found] = idx[win[found]]
    return out, shape


# ---- the test scene: clusters of overlapping spheres, rays aimed at them from far away -----------------------------------------------
def cluster_scene(dtype, n_clusters=3000, per=12, seed=5):
    """(cluster centres[n_clusters,3] f64, spheres[n_clusters * per, 4] in dtype): centres uniform in [-1e3, 1e3]^3, each with `per` spheres
    at centre + U(-1, 1)^3 with r = U(0.3, 0.8)"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1e3, 1e3, size=(n_clusters, 3))
    c = np.repeat(centres, per, axis=0) + rng.uniform(-1, 1, size=(n_clusters * per, 3))
    r = rng.uniform(0.3, 0.8, size=(n_clusters * per, 1))
    return centres, np.concatenate([c, r], axis=1).astype(dtype)


def cluster_rays(orc, centres, n, dtype, seed):
    """n rays with origins U(-2e3, 2e3)^3 aimed at a random cluster centre + U(-0.8, 0.8)^3, a tenth of them in random directions"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2e3, 2e3, size=(n, 3)).astype(dtype)
    target = centres[rng.integers(0, len(centres), size=n)] + rng.uniform(-0.8, 0.8, size=(n, 3))
    d = (target - o).astype(dtype)
    d[: n // 10] = rng.normal(size=(n // 10, 3))
    return orc.make_rays(o, d, dtype), rng


def tmax_draw(rng, nearest, dtype):
    """per ray a segment end: the nearest distance x U(0.3, 1.7) (4e3 where nothing is hit)"""
    c = nearest.astype(np.float64)
    span = np.where(np.isfinite(c), c, 4e3)
    return (span * rng.uniform(0.3, 1.7, size=len(c))).astype(dtype)
