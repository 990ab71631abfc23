"""Closest-hit and any-hit ray queries against sphere shapes on the GPU (bvhgpu_tree_set_spheres_* / bvhgpu_traverse_sphere_*): per ray, among
the shapes of FlatBvh::traverse's list whose sphere the ray hits with distance < tmax (strict), the nearest one (the first of the list on
equal distances) or — BVHGPU_TRAVERSE_FIRST — the first of the list.  The counterpart of tests/test_gpu_box_hit.py, case for case: every
check compares byte for byte against the oracle's CSR pushed through the definition (sphere_ref.sphere_match), across walks, dtypes, tree
kinds, replays and error paths."""
import ctypes as C

import numpy as np
import pytest

from sphere_ref import cluster_rays, cluster_scene, list_hits, sphere_match, tmax_draw
from test_gpu_any_hit import _aimed_rays, _cube_scene, _rb
from test_gpu_box_hit import WALKS, _tuned

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MODES = (("closest", False, 7), ("first", True, 8))   # (name, first, the walk kernels' MODE number)


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


def _oracle(orc, aabbs, rays, oflat=None):
    oflat = orc.flatten(orc.build(aabbs).nodes) if oflat is None else oflat
    off, idx, _, _ = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    return off, idx


def _ask(flat, rays_b, tmax, first):
    return (flat.first_sphere_hits if first else flat.closest_sphere_hits)(rays_b, tmax)


def _check(flat, rays_b, tmax, first, want):
    hit, shape = _ask(flat, rays_b, tmax, first)
    assert hit.tobytes() == want[0].tobytes()
    assert np.array_equal(shape, want[1])
    return hit, shape


def _sphere_tree(eng, spheres, ctx):
    from bvh_amd import spheres_aabbs
    flat = eng.Bvh.from_aabbs(spheres_aabbs(spheres), ctx).flatten()
    flat.set_spheres(spheres)
    return flat


def _bounding_spheres(aabbs, scale=0.6):
    """a sphere per box: the box's centre, `scale` x its half diagonal (so that a ray through the box may miss it)"""
    a = aabbs.astype(np.float64)
    c = (a[:, :3] + a[:, 3:]) / 2
    r = scale * np.linalg.norm(a[:, 3:] - a[:, :3], axis=1, keepdims=True) / 2
    return np.concatenate([c, r], axis=1).astype(aabbs.dtype)


# ---- 1. parity by walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_parity_by_walk(eng, orc, dtype):
    from bvh_amd import spheres_aabbs
    centres, spheres = cluster_scene(dtype)                              # 3 000 clusters x 12 spheres
    assert spheres.shape == (36000, 4)
    n = 40000
    rays, rng = cluster_rays(orc, centres, n, dtype, seed=21)
    aabbs = spheres_aabbs(spheres)
    off, idx = _oracle(orc, aabbs, rays)
    want_none = {first: sphere_match(off, idx, rays, spheres, None, first) for _, first, _ in MODES}
    # what the scene exercises, on the reference side: most rays hit a sphere, the nearest is often not the first of the list, and many list
    # members — boxes the ray passes — miss their sphere.  (Measured with the oracle, f32 and f64 alike: 0.84 of the rays hit; closest and first
    # differ on 0.50 of those; 0.41 of the 166 K list members miss; with tmax 0.42 of the rays keep a candidate.)
    hit = want_none[False][1] != NONE
    assert np.array_equal(hit, want_none[True][1] != NONE)
    assert hit.mean() >= 0.5, hit.mean()
    differ = (want_none[False][1][hit] != want_none[True][1][hit]).mean()
    assert differ >= 0.3, differ
    members = list_hits(off, idx, rays, spheres)[:, 0]
    assert np.isinf(members).mean() >= 0.2, np.isinf(members).mean()
    tmax = tmax_draw(rng, want_none[False][0][:, 0], dtype)
    # pinned rows: NaN, 0, -1, +inf, and exactly the distance of the first of the list (not admitted: strict <) — on rays whose first member hits
    first_hits = np.zeros(n, bool)
    rows = np.diff(off.astype(np.int64)) > 0
    first_hits[rows] = np.isfinite(members[off[:-1].astype(np.int64)[rows]])
    special = np.nonzero(first_hits)[0][:50]
    assert len(special) == 50
    tmax[special[0:10]] = np.nan
    tmax[special[10:20]] = 0
    tmax[special[20:30]] = -1
    tmax[special[30:40]] = np.inf
    tmax[special[40:50]] = members[off[special[40:50]]]
    want = {first: sphere_match(off, idx, rays, spheres, tmax, first) for _, first, _ in MODES}
    cand = want[False][1] != NONE
    assert np.array_equal(cand, want[True][1] != NONE)                   # a ray has a candidate or not, whichever one is asked for
    assert 0.2 <= cand.mean() <= 0.8, cand.mean()                        # both outcomes on at least a fifth of the rays
    for first in (False, True):
        assert np.all(want[first][1][special[:30]] == NONE) and np.all(want[first][1][special[30:40]] != NONE)
    assert not np.any(want[True][1][special[40:50]] == idx[off[special[40:50]]])
    tname = "float" if dtype == np.float32 else "double"
    for tune, kernel in WALKS:
        flat = _sphere_tree(eng, spheres, _tuned(tune))
        rb = _rb(eng, rays)
        goff, gidx, _, _ = flat.traverse_batch(rb)                       # the GPU's own CSR, through the definition
        for name, first, m in MODES:
            _check(flat, rb, None, first, want_none[first])
            assert flat.query_kernel().startswith(kernel.format(t=tname, m=m)), (tune, name, flat.query_kernel())
            assert flat._hits.info()["total"] == int(hit.sum())
            _check(flat, rb, tmax, first, want[first])
            assert flat.query_kernel().startswith(kernel.format(t=tname, m=m)), (tune, name, flat.query_kernel())
            assert flat._hits.info()["total"] == int(cand.sum())
            g = sphere_match(goff, gidx, rays, spheres, tmax, first)
            assert g[0].tobytes() == want[first][0].tobytes() and np.array_equal(g[1], want[first][1])
            # single rays (one lane per launch whatever the tuning) with the pinned segment ends
            for r in special[::5]:
                s1, p1 = _ask(flat, _rb(eng, rays[r:r + 1]), tmax[r:r + 1], first)
                assert s1.tobytes() == want[first][0][r:r + 1].tobytes() and p1[0] == want[first][1][r]
        assert np.array_equal(flat.sphere_occluded(rb, tmax), cand)


# ---- 2. a tree with a split without SAH winner -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_no_sah_winner_tree_takes_the_binary_walk(eng, orc, dtype):
    """the scene of the box test of the same name — empty child bounds, which the wide walk does not accept — with a sphere of diameter t in
    every flat box"""
    rng = np.random.default_rng(9)
    big = 1e19 if dtype == np.float32 else 1e154
    g, t = 2.0 ** 41, 2.0 ** 42
    lo = (np.round(rng.uniform(-1, 1, size=(500, 3)) * big / g) * g).astype(dtype)
    tris = np.stack([lo, lo + np.array([0, 0, t], dtype), lo + np.array([t, 0, 0], dtype)], axis=1).astype(dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1).astype(dtype)
    spheres = np.concatenate([lo + np.array([t / 2, 0, t / 2], dtype), np.full((500, 1), t / 2, dtype)], axis=1).astype(dtype)
    n = 20000
    o = (lo[rng.integers(0, 500, size=n)] + np.array([t / 4, t, t / 4], dtype)).astype(dtype)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], dtype), (n, 1))
    d[::3] = rng.normal(size=(len(d[::3]), 3))
    d[1::3, 0] = 1e-3
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    assert np.isposinf(oflat[oflat["entry"] != NONE]["min"]).all(axis=1).any()   # the tree does have empty child bounds
    off, idx = _oracle(orc, aabbs, rays, oflat)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    flat.set_spheres(spheres)
    for tmax in (None, np.where(np.arange(n) % 2 == 0, t / 2, 2 * t).astype(dtype)):
        for _, first, _ in MODES:
            want = sphere_match(off, idx, rays, spheres, tmax, first)
            _check(flat, _rb(eng, rays), tmax, first, want)
            assert "k_traverse_wide" not in flat.query_kernel(), flat.query_kernel()
            if dtype == np.float32 and tmax is None:
                assert (want[1] != NONE).sum() > 1000


# ---- 3. trees whose shapes moved -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_uploaded_flat_bvh_and_refitted_tree(eng, orc, dtype):
    from bvh_amd import FlatBvh, spheres_aabbs
    centres, spheres = cluster_scene(dtype, 1000)
    rng = np.random.default_rng(6)
    moved = spheres.astype(np.float64)
    moved[:, :3] += rng.uniform(-0.4, 0.4, size=(len(spheres), 3))
    moved = moved.astype(dtype)
    aabbs, aabbs_moved = spheres_aabbs(spheres), spheres_aabbs(moved)
    rays, _ = cluster_rays(orc, centres, 30000, dtype, seed=12)
    built = orc.build(aabbs).nodes
    oflat = orc.flatten(built)
    ctx = _tuned({})
    cases = []
    up = FlatBvh.from_flat_nodes(oflat, aabbs_moved, ctx)                # the old tree over the moved shapes: leaf tests use the shape AABBs
    up.set_spheres(moved)
    cases.append((up, _oracle(orc, aabbs_moved, rays, oflat)))
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    bvh.set_spheres(spheres)                                             # the spheres before the move: replaced below, after the refit
    bvh.refit(aabbs_moved)
    flat = bvh.flatten()
    want_stale = sphere_match(*_oracle(orc, aabbs_moved, rays, orc.flatten(orc.refit(built, aabbs_moved))), rays, spheres, None, False)
    _check(flat, _rb(eng, rays), None, False, want_stale)                # refit does not touch the spheres
    flat.set_spheres(moved)
    cases.append((flat, _oracle(orc, aabbs_moved, rays, orc.flatten(orc.refit(built, aabbs_moved)))))
    for tree, (off, idx) in cases:
        nearest = sphere_match(off, idx, rays, moved, None, False)[0][:, 0]
        assert np.isfinite(nearest).mean() > 0.3
        tmax = tmax_draw(np.random.default_rng(13), nearest, dtype)
        for _, first, _ in MODES:
            for tm in (None, tmax):
                _check(tree, _rb(eng, rays), tm, first, sphere_match(off, idx, rays, moved, tm, first))
    assert "k_traverse_wide" not in up.query_kernel() and "k_traverse_wide" in cases[1][0].query_kernel()


# ---- 4. wide-stack overflow ------------------------------------------------------------------------------------------------------
def test_sphere_hit_wide_stack_overflow_replays_through_the_binary_walk(eng, orc):
    """the chain of the box overflow test, a sphere in every box: a ray through all 400 boxes outgrows the wide walk's stack; the batch is
    replayed with the binary walk, which reads the staged HOST tmax again"""
    x = 2.0 ** np.arange(400)
    aabbs = np.stack([x, np.zeros_like(x), np.zeros_like(x), x * 1.25, np.ones_like(x), np.ones_like(x)], 1).astype(np.float64)
    spheres = np.stack([x * 1.125, np.full_like(x, 0.5), np.full_like(x, 0.5), x * 0.125], 1).astype(np.float64)
    o = np.tile([[-1.0, 0.25, 0.25]], (128, 1))
    d = np.tile([[1.0, 0.0, 0.0]], (128, 1)); d[::7] = [1.0, 1e-300, 0.0]
    rays = orc.make_rays(o, d, np.float64)
    tmax = np.concatenate([np.full(64, 0.5), np.full(32, np.inf), np.full(32, 2.0 ** 200)])
    off, idx = _oracle(orc, aabbs, rays)
    assert np.diff(off).min() == 400
    members = list_hits(off, idx, rays, spheres)[:, 0].reshape(128, 400)
    assert np.isinf(members).any(axis=1).all() and (np.isfinite(members).sum(axis=1) >= 390).all()   # the two smallest spheres are missed
    ctx = _tuned({0: 3, 3: 0})                                            # the wide walk for this small batch
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_spheres(spheres)
    for name, first, m in MODES:
        want = sphere_match(off, idx, rays, spheres, tmax, first)
        assert (want[1] == NONE).sum() == 64 and (want[1] != NONE).sum() == 64
        for items in (0, 2):
            ctx.set_tuning(1, items)
            _check(flat, _rb(eng, rays), tmax, first, want)
            assert flat.query_kernel().startswith("bvhgpu::k_traverse_lds<double, %d," % m), flat.query_kernel()   # replayed (the rays without a candidate walk all 400 boxes in either mode)
    # the result object goes on working with the wide walk afterwards
    centres, s2 = cluster_scene(np.float64, 300)
    flat2 = _sphere_tree(eng, s2, ctx)
    rays2, _ = cluster_rays(orc, centres, 5000, np.float64, seed=2)
    from bvh_amd import spheres_aabbs
    off2, idx2 = _oracle(orc, spheres_aabbs(s2), rays2)
    _check(flat2, _rb(eng, rays2), None, False, sphere_match(off2, idx2, rays2, s2, None, False))
    assert flat2.query_kernel().startswith("bvhgpu::k_traverse_wide<double, 7, 2,")


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_one_shape_empty_tree_and_empty_batch(eng, orc, dtype):
    from bvh_amd import spheres_aabbs
    ctx = _tuned({})
    spheres = np.array([[0.5, 0.5, 1.5, 0.5]], dtype=dtype)
    o = np.array([[0.5, 0.5, 0], [0.5, 0.5, 0], [0.5, 0.5, 0], [2, 2, 0], [0.5, 0.5, 3], [0.5, 0.5, 1.5], [0.0625, 0.0625, 0]], dtype=dtype)
    d = np.tile(np.array([[0, 0, 1]], dtype=dtype), (len(o), 1))
    rays = orc.make_rays(o, d, dtype)
    tmax = np.array([np.inf, 1, 1.5, np.inf, np.inf, 0, np.inf], dtype=dtype)
    aabbs = spheres_aabbs(spheres)
    off, idx = _oracle(orc, aabbs, rays)
    flat = _sphere_tree(eng, spheres, ctx)
    for _, first, _ in MODES:
        want = sphere_match(off, idx, rays, spheres, tmax, first)
        assert want[1].tolist() == [0, NONE, 0, NONE, NONE, NONE, NONE]      # (the last ray passes the box's corner, outside the sphere)
        assert want[0][0].tolist() == [1.0, 2.0] and off[-1] - off[-2] == 1
        _check(flat, _rb(eng, rays), tmax, first, want)
        assert flat._hits.info()["total"] == 2
        hit, shape = _ask(flat, _rb(eng, rays[:0]), np.zeros(0, dtype), first)
        assert hit.shape == (0, 2) and shape.shape == (0,) and flat._hits.info()["total"] == 0
        assert _ask(flat, _rb(eng, rays[:0]), None, first)[1].shape == (0,)
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx).flatten()
    empty.set_spheres(np.zeros((0, 4), dtype))
    for _, first, _ in MODES:
        hit, shape = _ask(empty, _rb(eng, rays), tmax, first)
        assert hit.tobytes() == np.tile(np.array([[np.inf, 0]], dtype), (len(rays), 1)).tobytes() and np.all(shape == NONE)
        assert empty._hits.info()["total"] == 0


# ---- 6. device memory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_device_rays_tmax_and_spheres(eng, orc, dtype):
    import torch
    from bvh_amd import BvhGpuError, RayBatch, spheres_aabbs
    centres, spheres = cluster_scene(dtype, 500)
    n = 30000
    rays, rng = cluster_rays(orc, centres, n, dtype, seed=4)
    aabbs = spheres_aabbs(spheres)
    off, idx = _oracle(orc, aabbs, rays)
    tmax = tmax_draw(rng, sphere_match(off, idx, rays, spheres, None, False)[0][:, 0], dtype)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    sdev = torch.from_numpy(spheres.copy()).cuda()
    flat.set_spheres(sdev)                                               # spheres that live in HBM
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    rb = RayBatch.from_device(dev, n, dtype)
    tdev = torch.from_numpy(tmax.copy()).cuda()
    for _, first, _ in MODES:
        _check(flat, rb, tdev, first, sphere_match(off, idx, rays, spheres, tmax, first))
        _check(flat, rb, None, first, sphere_match(off, idx, rays, spheres, None, first))
        _check(flat, _rb(eng, rays), tmax, first, sphere_match(off, idx, rays, spheres, tmax, first))
        with pytest.raises(BvhGpuError):
            _ask(flat, rb, tmax, first)                                   # host tmax for rays in HBM
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tdev, first)                       # ... and the other way round
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tmax.astype(np.float64 if dtype == np.float32 else np.float32), first)
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tmax[:-1], first)
    other = torch.float64 if dtype == np.float32 else torch.float32
    with pytest.raises(BvhGpuError):
        flat.set_spheres(sdev.to(other))                                  # a device tensor of the other dtype
    with pytest.raises(BvhGpuError):
        flat.set_spheres(sdev[:-1])                                       # ... of another shape count
    _check(flat, rb, tdev, False, sphere_match(off, idx, rays, spheres, tmax, False))   # the refusals left the tree's spheres alone


# ---- 7. one result object, every kind of batch -------------------------------------------------------------------------------------
def test_sphere_hit_result_object_reused_across_kinds(eng, orc):
    """one result object: CSR, closest hit, any hit, box, sphere — on the wide walk over items (the per-ray key and count buffers stay
    clean); every fetch refuses the result of another kind.  The tree holds triangles and spheres at once."""
    from bvh_amd import _lib, testbase as tb
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    from test_box_hit_cpu import box_match
    from test_gpu_any_hit import first_match
    lib = _lib.load()
    tris, aabbs = _cube_scene(tb, np.float32)
    spheres = _bounding_spheres(aabbs)
    n = 40000
    rays, rng = _aimed_rays(orc, tris, n, np.float32, seed=8)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    oisect, oclosest, oprim = orc.triangle_stage(tris, rays, off, idx)
    nearest = sphere_match(off, idx, rays, spheres, None, False)
    assert 0.3 < (nearest[1] != NONE).mean() and np.isinf(list_hits(off, idx, rays, spheres)[:, 0]).mean() > 0.1
    tmax = tmax_draw(rng, nearest[0][:, 0], np.float32)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    flat.set_triangles(tris)
    flat.set_spheres(spheres)
    rb = _rb(eng, rays)
    h = flat._hits.h
    buf3, buf2, shp, offs = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
    po, pi = C.c_void_p(), C.c_void_p()

    def refused_except(kind):
        calls = {"csr": lambda: lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST),
                 "sphere": lambda: lib.bvhgpu_hits_fetch_sphere(h, ptr(buf2), ptr(shp), HOST),
                 "box": lambda: lib.bvhgpu_hits_fetch_box(h, ptr(buf2), ptr(shp), HOST),
                 "any": lambda: lib.bvhgpu_hits_fetch_any(h, ptr(buf3), ptr(shp), HOST),
                 "closest": lambda: lib.bvhgpu_hits_fetch_closest(h, ptr(buf3), ptr(shp), HOST)}
        for k, call in calls.items():
            assert call() == (OK if k == kind else INVALID_ARG), (kind, k)
            if kind == "sphere" and k != kind:
                assert "bvhgpu_hits_fetch_sphere" in lib.bvhgpu_last_error(flat.ctx._h).decode(), k   # the refusal names the right call
        assert lib.bvhgpu_hits_fetch_triangles(h, ptr(buf3), HOST) == INVALID_ARG
        assert lib.bvhgpu_hits_device(h, C.byref(po), C.byref(pi), None) == (OK if kind == "csr" else INVALID_ARG)

    for _ in range(2):
        goff, gidx, _, _ = flat.traverse_batch(rb)
        assert np.array_equal(goff, off) and np.array_equal(gidx, idx)
        refused_except("csr")
        for _, first, _ in MODES:
            _check(flat, rb, tmax, first, sphere_match(off, idx, rays, spheres, tmax, first))
            assert flat.query_kernel().startswith("bvhgpu::k_traverse_wide<float, %d, 2," % (8 if first else 7))
            refused_except("sphere")
        isect, shape = flat.any_hits(rb, tmax)
        w = first_match(off, idx, oisect, tmax)
        assert isect.tobytes() == w[0].tobytes() and np.array_equal(shape, w[1])
        refused_except("any")
        _check(flat, rb, None, False, nearest)
        sl, shape = flat.closest_box_hits(rb, tmax)
        w = box_match(off, idx, ts, tmax, False)
        assert sl.tobytes() == w[0].tobytes() and np.array_equal(shape, w[1])
        refused_except("box")
        _check(flat, rb, None, True, sphere_match(off, idx, rays, spheres, None, True))
        cl, prim, _ = flat.closest_hits(rb)
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
        refused_except("closest")
        _check(flat, rb, tmax, False, sphere_match(off, idx, rays, spheres, tmax, False))
    goff, gidx, _, _ = flat.traverse_batch(rb)
    assert np.array_equal(goff, off) and np.array_equal(gidx, idx)


# ---- 8. triangles and spheres in one tree ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sphere_hit_tree_with_triangles_and_spheres(eng, orc, dtype):
    """closest_hits reads the triangles, closest_sphere_hits the spheres, whichever was set last"""
    from bvh_amd import testbase as tb
    tris, aabbs = _cube_scene(tb, dtype, 500)
    spheres = _bounding_spheres(aabbs)
    rays, _ = _aimed_rays(orc, tris, 20000, dtype, seed=14)
    off, idx = _oracle(orc, aabbs, rays)
    _, oclosest, oprim = orc.triangle_stage(tris, rays, off, idx)
    want = sphere_match(off, idx, rays, spheres, None, False)
    assert (want[1] != NONE).mean() > 0.3 and (want[1] != oprim).mean() > 0.1
    for order in ("tris-first", "spheres-first"):
        flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
        if order == "tris-first":
            flat.set_triangles(tris); flat.set_spheres(spheres)
        else:
            flat.set_spheres(spheres); flat.set_triangles(tris)
        for _ in range(2):
            cl, prim, _ = flat.closest_hits(_rb(eng, rays))
            assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
            _check(flat, _rb(eng, rays), None, False, want)


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------
def test_sphere_hit_errors(eng, orc):
    from bvh_amd import BvhGpuError, Context, _lib, spheres_aabbs
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, ptr
    lib = _lib.load()
    ctx = Context(0)
    spheres = np.array([[0.5, 0.5, 1.25, 0.25], [0.5, 0.5, 2.25, 0.25]], dtype=np.float32)
    aabbs = spheres_aabbs(spheres)
    rays = np.ascontiguousarray(orc.make_rays(np.array([[0.5, 0.5, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float32))
    rays64 = np.ascontiguousarray(orc.make_rays(np.array([[0.5, 0.5, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float64))
    tmax = np.full(4, 2.25, np.float32)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    h = C.c_void_p()
    f32 = lib.bvhgpu_traverse_sphere_f32
    assert f32(bvh._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == NOT_FLATTENED
    flat = bvh.flatten()
    # no spheres set
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == INVALID_ARG
    assert "bvhgpu_tree_set_spheres" in lib.bvhgpu_last_error(ctx._h).decode()
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_spheres"):
        flat.closest_sphere_hits(_rb(eng, rays))
    # wrong n, wrong dtype, NULL
    set32, set64 = lib.bvhgpu_tree_set_spheres_f32, lib.bvhgpu_tree_set_spheres_f64
    assert set32(flat._t, ptr(spheres), 1, HOST) == INVALID_ARG and set32(flat._t, ptr(spheres), 3, HOST) == INVALID_ARG
    assert set64(flat._t, ptr(spheres.astype(np.float64)), 2, HOST) == DTYPE_MISMATCH
    assert set32(flat._t, None, 2, HOST) == INVALID_ARG and set32(None, ptr(spheres), 2, HOST) == INVALID_ARG
    assert set32(flat._t, ptr(spheres), 2, 7) == INVALID_ARG                                # no such memory kind
    with pytest.raises(BvhGpuError):
        flat.set_spheres(spheres.astype(np.float64))
    with pytest.raises(BvhGpuError):
        flat.set_spheres(spheres[:1])
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == INVALID_ARG        # the refused calls set nothing
    assert set32(flat._t, ptr(spheres), 2, HOST) == OK
    assert lib.bvhgpu_traverse_sphere_f64(flat._t, ptr(rays64), None, 4, HOST, 0, C.byref(h)) == DTYPE_MISMATCH
    for bad in (1, 2, 4, 8, 32, 64, 128, 256, 512, 2048, 1 << 20, 1 << 29, 1 << 30, 1 << 31, 1024 | 1, 16 | 2):   # T_SLICE, STATS, ... and the internal marks
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, bad, C.byref(h)) == INVALID_ARG, bad
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, 7, 0, C.byref(h)) == INVALID_ARG           # no such memory kind
    assert f32(flat._t, None, None, 4, HOST, 0, C.byref(h)) == INVALID_ARG                  # NULL rays
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, None) == INVALID_ARG              # NULL result
    assert f32(flat._t, None, None, 0, HOST, 0, C.byref(h)) == OK                           # an empty batch
    hit = np.zeros((4, 2), np.float32)
    shape = np.zeros(4, np.uint32)
    total = C.c_uint64()
    off, idx = _oracle(orc, aabbs, rays)
    for flags in (0, 16, 1024, 1024 | 16):                                                  # COHERENT is a hint, FIRST selects the mode
        want = sphere_match(off, idx, rays, spheres, tmax, (flags & 1024) != 0)
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, flags, C.byref(h)) == OK
        assert lib.bvhgpu_hits_fetch_sphere(h, ptr(hit), ptr(shape), HOST) == OK
        assert np.array_equal(shape, want[1]) and hit.tobytes() == want[0].tobytes() and np.all(shape != NONE)
        assert lib.bvhgpu_hits_info(h, None, C.byref(total), None) == OK and total.value == 4
        assert lib.bvhgpu_hits_fetch_sphere(h, None, ptr(shape), HOST) == OK and lib.bvhgpu_hits_fetch_sphere(h, ptr(hit), None, HOST) == OK
    # the public traverse entry ignores the sphere mark: an ordinary CSR batch comes out, which _fetch_sphere refuses
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), 4, HOST, 1 << 29, C.byref(h)) == OK
    assert lib.bvhgpu_hits_fetch_sphere(h, ptr(hit), ptr(shape), HOST) == INVALID_ARG
    offs = np.zeros(5, np.uint32)
    assert lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST) == OK and offs[-1] == 8
    lib.bvhgpu_hits_destroy(h)
    # a ray dtype that differs, on the Python surface
    with pytest.raises(BvhGpuError):
        flat.closest_sphere_hits(_rb(eng, rays64))
    with pytest.raises(BvhGpuError):
        flat.first_sphere_hits(_rb(eng, rays64))
    # a rebuild with the same shape count keeps the spheres, one to another count drops them
    bvh.rebuild(aabbs[::-1].copy())
    flat = bvh.flatten()
    assert flat.closest_sphere_hits(_rb(eng, rays))[1].tolist() == [0, 0, 0, 0]            # (shape 0's sphere is still the nearer one)
    bvh.rebuild(np.concatenate([aabbs, aabbs[:1] + 8]))
    flat = bvh.flatten()
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_spheres"):
        flat.closest_sphere_hits(_rb(eng, rays))
    # a scene import has none
    bvh.rebuild(aabbs)
    flat = bvh.flatten()
    flat.set_spheres(spheres)
    assert flat.sphere_occluded(_rb(eng, rays)).all()
    blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
    flat.scene_export(blob)
    imported = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_spheres"):
        imported.closest_sphere_hits(_rb(eng, rays))
    imported.set_spheres(spheres)
    assert imported.closest_sphere_hits(_rb(eng, rays))[1].tolist() == [0, 0, 0, 0]
