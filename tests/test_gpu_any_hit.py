"""Any-hit (occlusion) queries on the GPU (bvhgpu_traverse_any_*): per ray the FIRST shape of FlatBvh::traverse's list whose
Ray::intersects_triangle distance is < tmax (strict), with that Intersection.  Every check compares byte for byte against the
oracle's CSR row and triangle stage (the definition), across walks, dtypes, tree shapes, replays and error paths."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


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


def _rb(eng, rays):
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    return eng.RayBatch(len(rays), dt, host=np.ascontiguousarray(rays))


def first_match(off, idx, oisect, tmax):
    """the definition on the oracle's CSR: per row the first j with oisect[j, 0] < tmax[row] → (isect[n,3], shape[n])"""
    n = len(off) - 1
    counts = np.diff(off.astype(np.int64))
    t = np.full(n, np.inf, dtype=oisect.dtype) if tmax is None else np.asarray(tmax, dtype=oisect.dtype)
    total = len(oisect)
    with np.errstate(invalid="ignore"):
        ok = oisect[:, 0] < np.repeat(t, counts)
    pos = np.where(ok, np.arange(total), total)
    first = np.full(n, total, dtype=np.int64)
    rows = counts > 0
    if total:
        first[rows] = np.minimum.reduceat(pos, off[:-1].astype(np.int64)[rows])
    found = first < total
    isect = np.zeros((n, 3), dtype=oisect.dtype)
    isect[:, 0] = np.inf
    isect[found] = oisect[first[found]]
    shape = np.full(n, NONE, dtype=np.uint32)
    shape[found] = idx[first[found]]
    return isect, shape


def _oracle(orc, tris, aabbs, rays, oflat=None):
    oflat = orc.flatten(orc.build(aabbs).nodes) if oflat is None else oflat
    off, idx, _, _ = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    oisect, oclosest, oprim = orc.triangle_stage(tris, rays, off, idx)
    return off, idx, oisect, oclosest, oprim


def _check(flat, rays_b, tmax, want):
    isect, shape = flat.any_hits(rays_b, tmax)
    assert isect.tobytes() == want[0].tobytes()
    assert np.array_equal(shape, want[1])
    return isect, shape


def _cube_scene(tb, dtype, n_cubes=3000):
    tris32, aabbs32 = tb.create_n_cubes(n_cubes)
    return tris32.astype(dtype), aabbs32.astype(dtype)


def _aimed_rays(orc, tris, n, dtype, seed):
    """rays aimed at cubes from far away, a tenth of them in random directions (set up like the triangle-stage test)"""
    rng = np.random.default_rng(seed)
    nc = len(tris) // 12
    centres = tris.reshape(nc, 36, 3).mean(axis=1)
    target = centres[rng.integers(0, nc, size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3))
    o = rng.uniform(-1e5, 1e5, size=(n, 3)).astype(dtype)
    d = (target - o).astype(dtype)
    d[: n // 10] = rng.normal(size=(n // 10, 3))
    return orc.make_rays(o, d, dtype), rng


def _tmax_draw(rng, oclosest, dtype):
    """per ray a segment end around the nearest hit: about half of the rays that hit something are occluded"""
    n = len(oclosest)
    c = oclosest[:, 0].astype(np.float64)
    span = np.where(np.isfinite(c), c, 2e5)
    return (span * rng.uniform(0.3, 1.7, size=n)).astype(dtype)


WALKS = [  # (tuning, kernel-name prefix) — {t} is the dtype's name
    ({0: 0, 3: 0}, "bvhgpu::k_traverse<{t}, 4, false>"),
    ({0: 2, 3: 0}, "bvhgpu::k_traverse_lds<{t}, 4, false>"),
    ({0: 3, 3: 0, 1: 0}, "bvhgpu::k_traverse_wide<{t}, 4, 0,"),
    ({0: 3, 3: 0, 1: 2}, "bvhgpu::k_traverse_wide<{t}, 4, 2,"),
    ({}, "bvhgpu::k_traverse_wide<{t}, 4, 2,"),   # default tuning: 40 K rays go to the wide walk, 16 items per ray
]


# ---- 1. parity by walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_parity_by_walk(eng, orc, dtype):
    from bvh_amd import Context, testbase as tb
    tris, aabbs = _cube_scene(tb, dtype)
    n = 40000
    rays, rng = _aimed_rays(orc, tris, n, dtype, seed=11)
    off, idx, oisect, oclosest, oprim = _oracle(orc, tris, aabbs, rays)
    tmax = _tmax_draw(rng, oclosest, dtype)
    # pinned rows: NaN, 0, -1, +inf, and exactly the first candidate's distance (not occluded by it: strict <)
    hit_rows = np.nonzero(np.isfinite(oisect[off[:-1].clip(max=len(oisect) - 1), 0]) & (np.diff(off) > 0))[0]
    special = hit_rows[:50]
    tmax[special[0:10]] = np.nan
    tmax[special[10:20]] = 0
    tmax[special[20:30]] = -1
    tmax[special[30:40]] = np.inf
    tmax[special[40:50]] = oisect[off[special[40:50]], 0]
    want_none = first_match(off, idx, oisect, None)
    want = first_match(off, idx, oisect, tmax)
    occ = want[1] != NONE
    assert 0.2 < occ.mean() < 0.8, occ.mean()                            # both outcomes on at least a fifth of the rays
    assert np.all(want[1][special[:30]] == NONE) and np.all(want[1][special[30:40]] != NONE)
    assert not np.any(want[1][special[40:50]] == idx[off[special[40:50]]])
    tname = "float" if dtype == np.float32 else "double"
    for tune, kernel in WALKS:
        ctx = Context(0)
        for k, v in tune.items():
            ctx.set_tuning(k, v)
        flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris)
        rb = _rb(eng, rays)
        _check(flat, rb, None, want_none)
        assert flat.query_kernel().startswith(kernel.format(t=tname)), (tune, flat.query_kernel())
        _check(flat, rb, tmax, want)
        assert flat.query_kernel().startswith(kernel.format(t=tname)), (tune, flat.query_kernel())
        assert flat._hits.info()["total"] == int(occ.sum())
        assert np.array_equal(flat.occluded(rb, tmax), occ)
        # the GPU's own triangle stage on the same rays gives the same answer through the definition
        goff, gidx, gisect, _ = flat.intersect_triangles(rb)
        g = first_match(goff, gidx, gisect, tmax)
        assert g[0].tobytes() == want[0].tobytes() and np.array_equal(g[1], want[1])
        # single rays (one lane per launch whatever the tuning) with the pinned segment ends
        for r in special[::5]:
            i1, s1 = flat.any_hits(_rb(eng, rays[r:r + 1]), tmax[r:r + 1])
            assert i1.tobytes() == want[0][r:r + 1].tobytes() and s1[0] == want[1][r]


# ---- 2. order, not distance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_is_first_in_order_not_nearest(eng, orc, dtype):
    """overlapping coplanar-plane triangles whose centroids lie far apart sit in different subtrees (different items of a ray): the
    first candidate in the reference's order is often not the nearest one"""
    from bvh_amd import Context, testbase as tb
    tris, _ = _cube_scene(tb, dtype)
    planes = np.arange(-400, 401, 50, dtype=np.float64)
    big = []
    for z in planes:
        big.append([[-2000.0, -600.0, z], [300.0, -600.0, z], [-400.0, 1200.0, z]])
        big.append([[-300.0, -600.0, z], [2000.0, -600.0, z], [400.0, 1200.0, z]])
    tris_t = np.concatenate([tris.reshape(-1, 3, 3), np.array(big).astype(dtype)]).astype(dtype)
    aabbs_t = np.concatenate([tris_t.min(axis=1), tris_t.max(axis=1)], axis=1).astype(dtype)
    rng = np.random.default_rng(5)
    m = 30000
    o = rng.uniform(-150, 150, size=(m, 3)); o[:, 2] = rng.choice(np.concatenate([planes - 25.0, [-1000.0]]), size=m)
    d = np.tile(np.array([[0.0, 0.0, 1.0]]), (m, 1)); d[m // 2:] *= -1.0
    rays = orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)
    off, idx, oisect, oclosest, oprim = _oracle(orc, tris_t, aabbs_t, rays)
    want = first_match(off, idx, oisect, None)
    differs = (want[1] != NONE) & (want[1] != oprim)
    assert differs.sum() > 300, differs.sum()
    for tune in ({}, {0: 0}):                                            # the wide walk over items; one lane per ray
        ctx = Context(0)
        for k, v in tune.items():
            ctx.set_tuning(k, v)
        flat = eng.Bvh.from_aabbs(aabbs_t, ctx).flatten()
        flat.set_triangles(tris_t)
        _check(flat, _rb(eng, rays), None, want)
        cl, prim, _ = flat.closest_hits(_rb(eng, rays))
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
        assert np.all(prim[differs] != want[1][differs])


# ---- 3. edge trees and inputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_no_sah_winner_tree_takes_the_binary_walk(eng, orc, dtype):
    """shapes spread so far apart that every surface area overflows: splits without SAH winner leave empty child bounds, which the
    wide walk does not accept — the binary walk answers.  The triangles sit on a grid of 2^41 with sides of 2^42 and each ray starts
    2^42 above one of them, so that in f32 every step of Ray::intersects_triangle is exact and finite (in f64 the same triangles
    are far below the coordinates' resolution: degenerate, never hit)."""
    from bvh_amd import Context
    rng = np.random.default_rng(9)
    big = 1e19 if dtype == np.float32 else 1e154
    g, t = 2.0 ** 41, 2.0 ** 42
    lo = (np.round(rng.uniform(-1, 1, size=(500, 3)) * big / g) * g).astype(dtype)
    tris = np.stack([lo, lo + np.array([0, 0, t], dtype), lo + np.array([t, 0, 0], dtype)], axis=1).astype(dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1).astype(dtype)
    n = 20000
    o = (lo[rng.integers(0, 500, size=n)] + np.array([t / 4, t, t / 4], dtype)).astype(dtype)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], dtype), (n, 1))
    d[::3] = rng.normal(size=(len(d[::3]), 3))
    d[1::3, 0] = 1e-3                                                    # (finite inverse directions as well)
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    assert np.isposinf(oflat[oflat["entry"] != NONE]["min"]).all(axis=1).any()   # the tree does have empty child bounds
    off, idx, oisect, _, _ = _oracle(orc, tris, aabbs, rays, oflat)
    ctx = Context(0)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    for tmax in (None, np.where(np.arange(n) % 2 == 0, t / 2, 2 * t).astype(dtype)):
        want = first_match(off, idx, oisect, tmax)
        _check(flat, _rb(eng, rays), tmax, want)
        assert "k_traverse_wide" not in flat.query_kernel(), flat.query_kernel()
        if dtype == np.float32:
            assert (want[1] != NONE).sum() > 1000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_one_shape_and_empty_batch(eng, orc, dtype):
    from bvh_amd import Context
    ctx = Context(0)
    tris = np.array([[[0, 0, 1], [0, 1, 1], [1, 0, 1]]], dtype=dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    o = np.array([[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0], [2, 2, 0], [0.25, 0.25, 2]], dtype=dtype)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]], dtype=dtype)
    rays = orc.make_rays(o, d, dtype)
    tmax = np.array([np.inf, 1, 1.5, np.inf, np.inf], dtype=dtype)
    off, idx, oisect, _, _ = _oracle(orc, tris, aabbs, rays)
    want = first_match(off, idx, oisect, tmax)
    assert want[1].tolist() == [0, NONE, 0, NONE, NONE]
    _check(flat, _rb(eng, rays), tmax, want)
    isect, shape = flat.any_hits(_rb(eng, rays[:0]), np.zeros(0, dtype))
    assert isect.shape == (0, 3) and shape.shape == (0,)
    assert flat._hits.info()["total"] == 0
    isect, shape = flat.any_hits(_rb(eng, rays[:0]))
    assert shape.shape == (0,)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_device_rays_and_tmax(eng, orc, dtype):
    import torch
    from bvh_amd import BvhGpuError, Context, RayBatch, testbase as tb
    ctx = Context(0)
    tris, aabbs = _cube_scene(tb, dtype, 500)
    n = 30000
    rays, rng = _aimed_rays(orc, tris, n, dtype, seed=4)
    off, idx, oisect, oclosest, _ = _oracle(orc, tris, aabbs, rays)
    tmax = _tmax_draw(rng, oclosest, dtype)
    want = first_match(off, idx, oisect, tmax)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    rb = RayBatch.from_device(dev, n, dtype)
    tdev = torch.from_numpy(tmax.copy()).cuda()
    _check(flat, rb, tdev, want)
    _check(flat, rb, None, first_match(off, idx, oisect, None))
    with pytest.raises(BvhGpuError):
        flat.any_hits(rb, tmax)                                           # host tmax for rays in HBM
    with pytest.raises(BvhGpuError):
        flat.any_hits(_rb(eng, rays), tdev)                               # ... and the other way round
    with pytest.raises(BvhGpuError):
        flat.any_hits(_rb(eng, rays), tmax.astype(np.float64 if dtype == np.float32 else np.float32))
    with pytest.raises(BvhGpuError):
        flat.any_hits(_rb(eng, rays), tmax[:-1])


def test_any_hit_wide_stack_overflow_replays_through_the_binary_walk(eng, orc):
    """the deep tree of the query overflow test: a ray through all 400 boxes outgrows the wide walk's stack; the batch is replayed
    with the binary walk, which reads the staged tmax again"""
    from bvh_amd import Context
    x = 2.0 ** np.arange(400)
    aabbs = np.stack([x, np.zeros_like(x), np.zeros_like(x), x * 1.25, np.ones_like(x), np.ones_like(x)], 1).astype(np.float64)
    px = x * 1.125
    tris = np.stack([np.stack([px, np.zeros_like(x), np.zeros_like(x)], 1), np.stack([px, np.zeros_like(x), np.ones_like(x)], 1),
                     np.stack([px, np.ones_like(x), np.zeros_like(x)], 1)], axis=1)
    o = np.tile([[-1.0, 0.25, 0.25]], (128, 1))
    d = np.tile([[1.0, 0.0, 0.0]], (128, 1)); d[::7] = [1.0, 1e-300, 0.0]
    rays = orc.make_rays(o, d, np.float64)
    tmax = np.concatenate([np.full(64, 0.5), np.full(32, np.inf), np.full(32, 2.0 ** 200)])
    off, idx, oisect, _, _ = _oracle(orc, tris, aabbs, rays)
    assert np.diff(off).min() == 400
    want = first_match(off, idx, oisect, tmax)
    assert (want[1] == NONE).sum() == 64 and (want[1] != NONE).sum() == 64
    ctx = Context(0)
    ctx.set_tuning(0, 3); ctx.set_tuning(3, 0)                            # the wide walk for this small batch
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    for items in (0, 2):
        ctx.set_tuning(1, items)
        _check(flat, _rb(eng, rays), tmax, want)
        assert flat.query_kernel().startswith("bvhgpu::k_traverse_lds<double, 4,"), flat.query_kernel()   # replayed
    # the result object goes on working with the wide walk afterwards
    from bvh_amd import testbase as tb
    tris_c, aabbs_c = _cube_scene(tb, np.float64, 300)
    flat2 = eng.Bvh.from_aabbs(aabbs_c, ctx).flatten()
    flat2.set_triangles(tris_c)
    rays2, _ = _aimed_rays(orc, tris_c, 5000, np.float64, seed=2)
    off2, idx2, oisect2, _, _ = _oracle(orc, tris_c, aabbs_c, rays2)
    _check(flat2, _rb(eng, rays2), None, first_match(off2, idx2, oisect2, None))
    assert flat2.query_kernel().startswith("bvhgpu::k_traverse_wide<double, 4, 2,")


def test_any_hit_result_object_reused_across_kinds(eng, orc):
    """one result object: CSR, any hit, closest hit, CSR — on the wide walk over items (the per-ray key and count buffers stay clean)"""
    from bvh_amd import Context, testbase as tb
    ctx = Context(0)
    tris, aabbs = _cube_scene(tb, np.float32)
    rays, rng = _aimed_rays(orc, tris, 40000, np.float32, seed=8)
    off, idx, oisect, oclosest, oprim = _oracle(orc, tris, aabbs, rays)
    tmax = _tmax_draw(rng, oclosest, np.float32)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    rb = _rb(eng, rays)
    for _ in range(2):
        goff, gidx, _, _ = flat.traverse_batch(rb)
        assert np.array_equal(goff, off) and np.array_equal(gidx, idx)
        _check(flat, rb, tmax, first_match(off, idx, oisect, tmax))
        cl, prim, _ = flat.closest_hits(rb)
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
        _check(flat, rb, None, first_match(off, idx, oisect, None))
    goff, gidx, _, _ = flat.traverse_batch(rb)
    assert np.array_equal(goff, off) and np.array_equal(gidx, idx)


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------
def test_any_hit_errors(eng, orc):
    from bvh_amd import Context, _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, ptr
    lib = _lib.load()
    ctx = Context(0)
    tris = np.array([[[0, 0, 1], [0, 1, 1], [1, 0, 1]], [[0, 0, 2], [0, 1, 2], [1, 0, 2]]], dtype=np.float32)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    rays = np.ascontiguousarray(orc.make_rays(np.array([[0.25, 0.25, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float32))
    rays64 = np.ascontiguousarray(orc.make_rays(np.array([[0.25, 0.25, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float64))
    tmax = np.full(4, 1.5, np.float32)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    bvh.set_triangles(tris)
    h = C.c_void_p()
    f32 = lib.bvhgpu_traverse_any_f32
    assert f32(bvh._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == NOT_FLATTENED
    flat = bvh.flatten()
    bare = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    assert f32(bare._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == INVALID_ARG        # no triangles
    assert lib.bvhgpu_traverse_any_f64(flat._t, ptr(rays64), None, 4, HOST, 0, C.byref(h)) == DTYPE_MISMATCH
    for bad in (1, 2, 4, 8, 32, 64, 128, 256, 512, 1 << 20, 1 << 31):
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, bad, C.byref(h)) == INVALID_ARG, bad
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, 7, 0, C.byref(h)) == INVALID_ARG           # no such memory kind
    assert f32(flat._t, None, None, 4, HOST, 0, C.byref(h)) == INVALID_ARG                  # NULL rays
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, None) == INVALID_ARG              # NULL result
    assert f32(flat._t, None, None, 0, HOST, 0, C.byref(h)) == OK                           # an empty batch
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 16, C.byref(h)) == OK                # COHERENT is a hint
    isect = np.zeros((4, 3), np.float32)
    shape = np.zeros(4, np.uint32)
    assert lib.bvhgpu_hits_fetch_any(h, ptr(isect), ptr(shape), HOST) == OK
    assert shape.tolist() == [0] * 4 and isect[:, 0].tolist() == [1.0] * 4
    total = C.c_uint64()
    assert lib.bvhgpu_hits_info(h, None, C.byref(total), None) == OK and total.value == 4
    offs = np.zeros(5, np.uint32)
    assert lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST) == INVALID_ARG
    assert lib.bvhgpu_hits_fetch_triangles(h, ptr(isect), HOST) == INVALID_ARG
    assert lib.bvhgpu_hits_fetch_closest(h, ptr(isect), ptr(shape), HOST) == INVALID_ARG
    po, pi = C.c_void_p(), C.c_void_p()
    assert lib.bvhgpu_hits_device(h, C.byref(po), C.byref(pi), None) == INVALID_ARG
    # ... and _fetch_any on the other kinds of result
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), 4, HOST, 0, C.byref(h)) == OK
    assert lib.bvhgpu_hits_fetch_any(h, ptr(isect), ptr(shape), HOST) == INVALID_ARG
    assert lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST) == OK
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), 4, HOST, 8, C.byref(h)) == OK        # CLOSEST
    assert lib.bvhgpu_hits_fetch_any(h, ptr(isect), ptr(shape), HOST) == INVALID_ARG
    lib.bvhgpu_hits_destroy(h)
    assert DEVICE == 1


# ---- 5. scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_hit_1m_rays_of_the_bench_stream(eng, orc, dtype):
    """configs[1]: create_n_cubes(10000), 1 M rays of the bench stream with a tmax draw, default tuning.  The stream almost never meets a
    triangle of this sparse scene, so the same 1 M origins are also re-aimed at random cubes: a batch where half of the rays are occluded."""
    from bvh_amd import Context, testbase as tb
    tris32, aabbs32 = tb.create_n_cubes(10000)
    tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
    n = 1_000_000
    stream = orc.create_rays(0, n, dtype=dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    ctx = Context(0)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    rng = np.random.default_rng(1)
    centres = tris.reshape(-1, 36, 3).astype(np.float64).mean(axis=1)
    target = centres[rng.integers(0, len(centres), size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3))
    aimed = orc.make_rays(stream["o"], (target - stream["o"].astype(np.float64)).astype(dtype), dtype)
    for rays, draw in ((stream, "uniform"), (aimed, "around the nearest hit")):
        off, idx, oisect, oclosest, _ = _oracle(orc, tris, aabbs, rays, oflat)
        if draw == "uniform":
            tmax = rng.uniform(0, 3e5, size=n).astype(dtype)
            tmax[::4] = np.inf
        else:
            tmax = _tmax_draw(rng, oclosest, dtype)
        want = first_match(off, idx, oisect, tmax)
        occ = want[1] != NONE
        if draw != "uniform":
            assert 0.2 < occ.mean() < 0.8, occ.mean()
        _check(flat, _rb(eng, rays), tmax, want)
        assert flat.query_kernel().startswith("bvhgpu::k_traverse_wide<"), flat.query_kernel()
        assert flat._hits.info()["total"] == int(occ.sum())
