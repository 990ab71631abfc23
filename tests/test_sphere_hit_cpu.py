"""Closest-hit and any-hit ray queries against sphere shapes (bvhgpu_traverse_sphere_*), pinned on numpy and the oracle alone.

Definition (include/bvh_mi355x.h): L_i is FlatBvh::traverse's list for ray i; for s in L_i the leaf stage is sphere_ref.ray_sphere
on the ray's o and d and shape s's sphere {c, r}; s is a candidate iff it hits and distance < tmax[i] (strict, in T; tmax None = +inf).
closest: the candidate with the smallest distance, the first of L_i on equal distances.  first: the first candidate of L_i.  No candidate:
{+inf, 0} and NONE.  sphere_ref.sphere_match is that definition on a CSR; tests/test_gpu_sphere_hit.py compares the GPU against it byte for
byte.  The rows below are hand-made on a grid where every value of the leaf stage is exact."""
import numpy as np
import pytest

from sphere_ref import NONE, cluster_rays, cluster_scene, list_hits, ray_sphere, sphere_match

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


def _rays(o, d, dtype):
    """ray records as the Ray struct holds them; d is used as given (unit vectors on the grid, or the zero direction)"""
    o = np.asarray(o, dtype=dtype).reshape(-1, 3)
    d = np.asarray(d, dtype=dtype).reshape(-1, 3)
    rays = np.zeros(len(o), dtype=np.dtype([("o", dtype, 3), ("d", dtype, 3), ("inv", dtype, 3)]))
    rays["o"], rays["d"] = o, d
    with np.errstate(divide="ignore"):
        rays["inv"] = dtype(1) / d
    return rays


def _one(spheres, o, d, dtype, tmax=None, first=False, order=None):
    """one ray against a hand-made list: `order` is L_i (default: the shapes in index order)"""
    spheres = np.asarray(spheres, dtype=dtype).reshape(-1, 4)
    idx = np.arange(len(spheres), dtype=np.uint32) if order is None else np.asarray(order, dtype=np.uint32)
    off = np.array([0, len(idx)], dtype=np.uint32)
    hit, shape = sphere_match(off, idx, _rays([o], [d], dtype), spheres, None if tmax is None else np.array([tmax], dtype), first)
    assert hit.dtype == dtype and shape.dtype == np.uint32
    return hit[0].tolist(), int(shape[0])


MISS = ([np.inf, 0.0], NONE)
X = (1.0, 0.0, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_through_the_centre_tangent_and_beside(dtype):
    for first in (False, True):
        # through the centre: tc = 4, l = 0, disc = 1, h = 1
        assert _one([[4, 0, 0, 1]], (0, 0, 0), X, dtype, first=first) == ([3.0, 5.0], 0)
        # tangent: l = (0, -1, 0), disc == 0 hits, t0 = t1 = 4
        assert _one([[4, 1, 0, 1]], (0, 0, 0), X, dtype, first=first) == ([4.0, 4.0], 0)
        # through the corner of the sphere's box [3, 5] x [-1, 1]^2, outside the sphere: |l|^2 = 2 * 0.875^2 > 1
        assert _one([[4, 0, 0, 1]], (0, 0.875, 0.875), X, dtype, first=first) == MISS
        # a direction that is no unit vector: a = 4, tc = 2, h = sqrt(1 / 4)
        assert _one([[4, 0, 0, 1]], (0, 0, 0), (2.0, 0.0, 0.0), dtype, first=first) == ([1.5, 2.5], 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_origin_inside_and_sphere_behind(dtype):
    for first in (False, True):
        # inside: tc = -0.5, t0 = -1.5 fails t0 > eps, the hit is the exit
        assert _one([[4, 0, 0, 1]], (4.5, 0, 0), X, dtype, first=first) == ([0.5, 0.5], 0)
        # at the centre
        assert _one([[4, 0, 0, 1]], (4, 0, 0), X, dtype, first=first) == ([1.0, 1.0], 0)
        # on the surface, looking out: t0 = -2, t1 = 0 is not > eps
        assert _one([[4, 0, 0, 1]], (5, 0, 0), X, dtype, first=first) == MISS
        # on the surface, looking in: t0 = 0 is not > eps, t1 = 2
        assert _one([[4, 0, 0, 1]], (3, 0, 0), X, dtype, first=first) == ([2.0, 2.0], 0)
        # behind the origin: t0 = -5, t1 = -3
        assert _one([[4, 0, 0, 1]], (8, 0, 0), X, dtype, first=first) == MISS


@pytest.mark.parametrize("dtype", DTYPES)
def test_tmax_is_strict_and_in_T(dtype):
    for first in (False, True):
        assert _one([[4, 0, 0, 1]], (0, 0, 0), X, dtype, tmax=3.0, first=first) == MISS            # equal to the distance: not admitted
        assert _one([[4, 0, 0, 1]], (0, 0, 0), X, dtype, tmax=np.nextafter(dtype(3), dtype(4)), first=first) == ([3.0, 5.0], 0)
        for t in (np.nan, 0.0, -1.0, -np.inf):
            assert _one([[4, 0, 0, 1]], (0, 0, 0), X, dtype, tmax=t, first=first) == MISS
        assert _one([[4, 0, 0, 1]], (0, 0, 0), X, dtype, tmax=np.inf, first=first) == ([3.0, 5.0], 0)
        assert _one([[4, 0, 0, 1]], (0, 0.875, 0.875), X, dtype, tmax=np.inf, first=first) == MISS  # a miss's +inf is below no tmax


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_distances_the_first_of_the_list_wins(dtype):
    two = [[4, 0.5, 0, 1], [4, -0.5, 0, 1]]                              # mirror images: disc = 0.75 for both, the same bits
    h = np.sqrt(dtype(0.75))
    want = [float(dtype(4) - h), float(dtype(4) + h)]
    for first in (False, True):
        assert _one(two, (0, 0, 0), X, dtype, first=first, order=[0, 1]) == (want, 0)
        assert _one(two, (0, 0, 0), X, dtype, first=first, order=[1, 0]) == (want, 1)
        assert _one(two, (0, 0, 0), X, dtype, tmax=want[0], first=first, order=[1, 0]) == MISS


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_member_farther_the_modes_differ(dtype):
    far_first = [[8, 0, 0, 1], [4, 0, 0, 1], [12, 0.875, 0.875, 1]]      # L_i = far, near, and one whose box the ray passes and whose sphere it misses
    assert _one(far_first, (0, 0, 0), X, dtype, first=False) == ([3.0, 5.0], 1)
    assert _one(far_first, (0, 0, 0), X, dtype, first=True) == ([7.0, 9.0], 0)
    # a segment that ends between the two: the far one is no candidate, first skips it
    assert _one(far_first, (0, 0, 0), X, dtype, tmax=6.0, first=True) == ([3.0, 5.0], 1)
    assert _one(far_first, (0, 0, 0), X, dtype, tmax=6.0, first=False) == ([3.0, 5.0], 1)
    # first skips members that miss
    assert _one([[4, 1, 1, 1], [8, 0, 0, 1]], (0, 0, 0), X, dtype, first=True) == ([7.0, 9.0], 1)
    # several rows at once, with an empty one in between
    spheres = np.array(far_first, dtype=dtype)
    rays = _rays([(0, 0, 0), (0, 5, 5), (20, 0, 0)], [X, X, (-1.0, 0.0, 0.0)], dtype)
    off = np.array([0, 3, 3, 6], dtype=np.uint32)
    idx = np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32)
    hit, shape = sphere_match(off, idx, rays, spheres, None, False)
    assert shape.tolist() == [1, NONE, 0] and hit.tolist() == [[3.0, 5.0], [np.inf, 0.0], [11.0, 13.0]]
    hit, shape = sphere_match(off, idx, rays, spheres, None, True)
    assert shape.tolist() == [0, NONE, 0] and hit.tolist() == [[7.0, 9.0], [np.inf, 0.0], [11.0, 13.0]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_is_special_cased(dtype):
    for first in (False, True):
        assert _one([[4, 0, 0, np.nan]], (0, 0, 0), X, dtype, first=first) == MISS                  # NaN radius
        assert _one([[np.nan, 0, 0, 1]], (0, 0, 0), X, dtype, first=first) == MISS                  # NaN centre
        assert _one([[4, 0, 0, 1]], (0, 0, 0), (np.nan, 0.0, 0.0), dtype, first=first) == MISS      # NaN direction
        assert _one([[4, 0, 0, -1]], (0, 0, 0), X, dtype, first=first) == ([3.0, 5.0], 0)           # r < 0 acts like |r|
        assert _one([[4, 0, 0, 1]], (0, 0, 0), (0.0, 0.0, 0.0), dtype, first=first) == MISS         # zero direction: a = 0
        assert _one([[4, 0, 0, 1]], (4, 0, 0), (0.0, 0.0, 0.0), dtype, first=first) == MISS         # ... even from inside
        assert _one([[4, 0, 0, np.inf]], (0, 0, 0), X, dtype, first=first) == MISS                  # r = inf: t0 = -inf, t1 = +inf is below no tmax
        assert _one([[4, 0, 0, 0]], (0, 0, 0), X, dtype, first=first) == ([4.0, 4.0], 0)            # r = 0 on the ray: disc == 0


def test_f32_and_f64_restatements_agree_on_the_gpu_tests_scene(orc):
    """the scene of tests/test_gpu_sphere_hit.py (f32 values, also taken exactly into f64), the oracle's lists: both restatements name a hit
    or a miss for the same rays"""
    from bvh_amd import spheres_aabbs
    centres, s32 = cluster_scene(np.float32)
    rays32, _ = cluster_rays(orc, centres, 40000, np.float32, seed=21)
    aabbs = spheres_aabbs(s32)
    assert aabbs.dtype == np.float32 and aabbs.shape == (len(s32), 6)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    off, idx, _, _ = orc.traverse_flat(oflat, aabbs, rays32, threads=orc.max_threads())
    rays64 = np.zeros(len(rays32), dtype=np.dtype([("o", np.float64, 3), ("d", np.float64, 3), ("inv", np.float64, 3)]))
    rays64["o"], rays64["d"] = rays32["o"], rays32["d"]
    hit32, shape32 = sphere_match(off, idx, rays32, s32, None, False)
    hit64, shape64 = sphere_match(off, idx, rays64, s32.astype(np.float64), None, False)
    h32, h64 = shape32 != NONE, shape64 != NONE
    both = h32 & h64
    rel = np.abs(hit32[both, 0].astype(np.float64) - hit64[both, 0]) / hit64[both, 0]
    m32, m64 = list_hits(off, idx, rays32, s32)[:, 0], list_hits(off, idx, rays64, s32.astype(np.float64))[:, 0]
    print(f"rays hitting: f32 {h32.mean():.4f} f64 {h64.mean():.4f}; rays that differ {int((h32 != h64).sum())}; list members that differ "
          f"{int((np.isfinite(m32) != np.isfinite(m64)).sum())} of {len(m32)}; nearest distance: max relative difference {rel.max():.3g}")
    assert h64.mean() >= 0.5
    assert np.array_equal(h32, h64), np.nonzero(h32 != h64)[0][:20]


def test_spheres_aabbs():
    from bvh_amd import spheres_aabbs
    for dtype in DTYPES:
        s = np.array([[1, 2, 3, 0.5], [-4, 0, 8, 2]], dtype=dtype)
        b = spheres_aabbs(s)
        assert b.dtype == dtype and b.tolist() == [[0.5, 1.5, 2.5, 1.5, 2.5, 3.5], [-6, -2, 6, -2, 2, 10]]
    assert spheres_aabbs(np.zeros((0, 4), np.float32)).shape == (0, 6)


def test_the_python_surface_exists():
    import bvh_amd
    from bvh_amd import api
    for name in ("set_spheres", "closest_sphere_hits", "first_sphere_hits", "sphere_occluded"):
        assert callable(getattr(api._TreeBase, name, None)), name
    assert callable(getattr(api._Hits, "fetch_sphere", None))
    assert callable(getattr(api, "spheres_aabbs", None)) and bvh_amd.spheres_aabbs is api.spheres_aabbs
    from bvh_amd import _lib
    assert {"bvhgpu_tree_set_spheres_f32", "bvhgpu_tree_set_spheres_f64", "bvhgpu_traverse_sphere_f32", "bvhgpu_traverse_sphere_f64",
            "bvhgpu_hits_fetch_sphere"} <= {name for name, _, _ in _lib.SYMBOLS}
    assert _lib.load().bvhgpu_abi_version() == 7


def test_ray_sphere_keeps_the_dtype():
    for dtype in DTYPES:
        out = ray_sphere(np.zeros((2, 3), dtype), np.array([X, X], dtype), np.array([[4, 0, 0, 1], [4, 3, 0, 1]], dtype))
        assert out.dtype == dtype and out.tolist() == [[3.0, 5.0], [np.inf, 0.0]]
