"""Instanced scenes, CPU side: the scenes tests/test_gpu_instances.py runs, shown on the reference alone (tests/instances_ref.py over the
oracle) to be non-trivial; hand cases with analytic answers; and the wiring of the new HIP file into the build."""
import os

import numpy as np
import pytest

import instances_ref as ir
from sphere_ref import tmax_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF
N_RAYS = 1500
SPREAD = 6.0      # instance translations are U(-SPREAD, SPREAD)^3 around objects of extent ~ +-3.5: the world boxes overlap
SIZES = (1, 2, 37)


def _tris_aabbs(tris):
    t = tris.reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))


def member_trees(orc, dtype):
    """A: one cube (12 triangles), B: 20 cubes, C: one triangle (n == 1); cubes drawn inside [-3, 3]^3 → [(aabbs, tris)] in dtype"""
    small = np.array([-3.0] * 3 + [3.0] * 3, dtype=np.float32)
    ta, _ = orc.create_n_cubes(1, small)
    tb, _ = orc.create_n_cubes(20, small)
    tc = np.array([[[-1.5, -1.0, 0.25], [1.5, -1.0, 0.0], [0.0, 2.0, -0.25]]])
    out = []
    for t in (ta, tb, tc):
        t = np.ascontiguousarray(t.astype(dtype)).reshape(-1, 3, 3)
        out.append((_tris_aabbs(t), t))
    return out


def transforms(n, dtype, seed):
    """rotations about random axes, non-uniform scales in [0.5, 2], every fifth mirrored, translations U(-SPREAD, SPREAD)^3 → (n, 3, 4)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3, 4))
    for i in range(n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        s = rng.uniform(0.5, 2.0, size=3)
        if i % 5 == 4:
            s[int(rng.integers(0, 3))] *= -1     # negative determinant
        x[i, :, :3] = R @ np.diag(s)
        x[i, :, 3] = rng.uniform(-SPREAD, SPREAD, size=3)
    return np.ascontiguousarray(x.astype(dtype))


def tree_slots(n, seed):
    """which member each instance copies: the one-instance set is B, larger sets start A, B, C and go on at random"""
    if n == 1:
        return np.array([1], dtype=np.uint32)
    rng = np.random.default_rng(seed)
    of = rng.integers(0, 3, size=n)
    of[:min(n, 3)] = [0, 1, 2][:min(n, 3)]
    return of.astype(np.uint32)


def cluster_rays(orc, n, dtype, seed):
    """origins U(-40, 40)^3 aimed into the cluster (+-(SPREAD + 1)), a tenth in random directions"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-40, 40, size=(n, 3)).astype(dtype)
    target = rng.uniform(-(SPREAD + 1), SPREAD + 1, size=(n, 3))
    d = (target - o).astype(dtype)
    d[: n // 10] = rng.normal(size=(n // 10, 3))
    return orc.make_rays(o, d, dtype)


_CASES = {}


def case(orc, dtype, n):
    """the scene of `n` instances with its rays, drawn tmax and reference answers (computed once, never modified)"""
    key = (np.dtype(dtype).name, n)
    if key not in _CASES:
        trees = member_trees(orc, dtype)
        of, x = tree_slots(n, 100 + n), transforms(n, dtype, 200 + n)
        sc = ir.Scene(trees, of, x, dtype)
        rays = cluster_rays(orc, N_RAYS, dtype, 300 + n)
        free = sc.trace(rays)
        tmax = tmax_draw(np.random.default_rng(400 + n), free["closest"][0][:, 0], dtype)
        _CASES[key] = dict(trees=trees, tree_of=of, x=x, scene=sc, rays=rays, tmax=tmax, free=free, cut=sc.trace(rays, tmax))
    return _CASES[key]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the definition's pieces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_inverse_undoes_the_transform(dtype):
    """Y X = identity up to rounding: |entries| <= 2, condition <= 4, a dozen rounded operations per entry — 256 eps is generous and a wrong
    cofactor is off by O(1)"""
    x = transforms(64, dtype, 7)
    y = ir.inverse(x).astype(np.float64)
    x4 = np.concatenate([x.astype(np.float64), np.tile([[[0, 0, 0, 1.0]]], (64, 1, 1))], axis=1)
    y4 = np.concatenate([y, np.tile([[[0, 0, 0, 1.0]]], (64, 1, 1))], axis=1)
    err = np.abs(y4 @ x4 - np.eye(4)).max()
    assert err < 256 * np.finfo(dtype).eps * (1 + SPREAD), err
    assert (np.linalg.det(x[:, :, :3].astype(np.float64)) < 0).sum() >= 10     # mirrored instances are there


@pytest.mark.parametrize("dtype", DTYPES)
def test_world_boxes_contain_the_transformed_triangles(orc, dtype):
    c = case(orc, dtype, 37)
    sc = c["scene"]
    slack = 64 * np.finfo(dtype).eps * 16
    for i in range(37):
        _, tris = c["trees"][int(c["tree_of"][i])]
        p = ir.forward(sc.x[i].astype(np.float64), tris.reshape(-1, 3).astype(np.float64))
        assert (p >= sc.w[i, :3] - slack).all() and (p <= sc.w[i, 3:] + slack).all()


def test_join_orders_the_zeros():
    a = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -1.0]], dtype=np.float32)
    mn, mx = ir._join_min(a), ir._join_max(a)
    assert np.signbit(mn[:2]).all() and not np.signbit(mx[:2]).any() and mn[2] == -1 and mx[2] == 1


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_copies_along_x(orc, dtype):
    """one triangle in the plane x = 0 facing -x; instance 0 at x = 8, instance 1 at x = 4 (exactly representable): a ray from the origin along
    +x meets them at exactly 4 and 8"""
    tri = np.array([[[0, -1, -1], [0, 0, 1], [0, 1, -1]]], dtype=dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x[0, 0, 3], x[1, 0, 3] = 8, 4
    sc = ir.Scene([(_tris_aabbs(tri), tri)], [0, 0], x, dtype)
    rays = orc.make_rays([[0, 0, 0]], [[1, 0, 0]], dtype)
    r = sc.trace(rays)
    t = r["table"]
    assert sorted(zip(t["instance"].tolist(), t["vals"][:, 0].tolist())) == [(0, 8.0), (1, 4.0)]
    vals, inst, shape = r["closest"]
    assert vals[0, 0] == 4 and inst[0] == 1 and shape[0] == 0
    vals, inst, shape = sc.trace(rays, np.array([6], dtype=dtype))["closest"]
    assert vals[0, 0] == 4 and inst[0] == 1
    vals, inst, shape = sc.trace(rays, np.array([4], dtype=dtype))["closest"]      # strict: the hit at exactly tmax is outside
    assert np.isinf(vals[0, 0]) and inst[0] == NONE and shape[0] == NONE
    f = sc.trace(rays, np.array([9], dtype=dtype))["first"]
    assert f[1][0] == t["instance"][0] and f[0][0, 0] == t["vals"][0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree(orc, dtype):
    """a set that is one identity instance of B reproduces orc.triangle_stage's closest result bit for bit"""
    trees = member_trees(orc, dtype)
    aabbs, tris = trees[1]
    sc = ir.Scene([trees[1]], [0], np.eye(3, 4, dtype=dtype)[None], dtype)
    assert sc.w.tobytes() == ir.tree_bounds(aabbs)[None].tobytes()
    rays = cluster_rays(orc, 600, dtype, 11)
    rays["o"] *= dtype(0.2)                                  # (B sits inside [-3.5, 3.5]^3)
    flat = orc.flatten(orc.build(aabbs).nodes)
    off, idx, _, _ = orc.traverse_flat(flat, aabbs, rays)
    _, closest, prim = orc.triangle_stage(tris, rays, off, idx)
    vals, inst, shape = sc.trace(rays)["closest"]
    hit = prim != NONE
    assert hit.sum() >= 50
    assert vals.tobytes() == closest.tobytes() and shape.tobytes() == prim.tobytes()
    assert (inst[hit] == 0).all() and (inst[~hit] == NONE).all()


# ---- the scenes the GPU test runs are worth running -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scene_is_not_trivial(orc, dtype):
    c = case(orc, dtype, 37)
    free, cut = c["free"], c["cut"]
    n = N_RAYS
    hit = free["closest"][1] != NONE
    assert hit.sum() >= 20 and (~hit).sum() >= 20
    toff, _ = free["top"]
    assert (np.diff(toff.astype(np.int64)) >= 2).sum() >= 20
    t = free["table"]
    later = 0
    for j in range(n):
        lo, hi = t["cand_off"][j], t["cand_off"][j + 1]
        d = t["vals"][lo:hi, 0]
        fin = np.nonzero(np.isfinite(d))[0]
        if len(fin) and t["instance"][lo + fin[0]] != free["closest"][1][j]:
            later += 1       # the closest hit is in an instance that is not the first one to yield a hit
    differ = (free["closest"][2] != free["first"][2]) | (free["closest"][1] != free["first"][1])
    assert later >= 20 and differ.sum() >= 20
    cut_away = hit & (cut["closest"][1] == NONE)          # tmax ends the segment in front of every hit
    kept = hit & (cut["closest"][1] != NONE)
    assert cut_away.sum() >= 20 and kept.sum() >= 20, (cut_away.sum(), kept.sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_every_set_answers(orc, dtype, n):
    c = case(orc, dtype, n)
    assert (c["free"]["closest"][1] != NONE).sum() >= 5
    assert c["scene"].w.shape == (n, 6) and np.isfinite(c["scene"].w).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_repose_changes_the_answers(orc, dtype):
    c = case(orc, dtype, 37)
    sc = ir.Scene(c["trees"], c["tree_of"], c["x"], dtype)
    before = sc.trace(c["rays"])["closest"]
    after = sc.pose(transforms(37, dtype, 999)).trace(c["rays"])["closest"]
    assert sc.w.tobytes() != c["scene"].w.tobytes()
    assert (before[1] != after[1]).sum() >= 20 and before[0].tobytes() != after[0].tobytes()


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_are_built_and_bound():
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances.hip" in build_ext.SOURCES
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_instances_trace", b"k_instances_prep"):
        assert kern in blob, kern
    names = {s[0] for s in _lib.SYMBOLS}
    for sym in ("create_f32", "create_f64", "update_f32", "update_f64", "trace_f32", "trace_f64", "boxes", "info", "destroy"):
        assert "bvhgpu_instances_" + sym in names
    import bvh_amd
    from bvh_amd import api
    assert bvh_amd.Instances.__module__ == "bvh_amd.instances" and not issubclass(bvh_amd.Instances, api._TreeBase)
    for m in ("update", "closest_hits", "any_hits", "occluded", "world_boxes", "info", "close", "__enter__", "__exit__"):
        assert hasattr(bvh_amd.Instances, m), m
