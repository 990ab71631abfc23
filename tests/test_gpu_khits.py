"""Multi-hit ray queries on the GPU (bvhgpu_traverse_khits_*): row i is the candidates of FlatBvh::traverse's list — the members whose
leaf-stage distance is < tmax[i], strict — in a stable ascending sort by distance, cut to the first k, then padding.  Every check compares
shapes and values byte for byte against the oracle's CSR pushed through the definition (khits_ref.khits_match); tests/test_khits_cpu.py
shows on the oracle alone that the scenes used here truncate, tie and come in reversed order."""

import numpy as np
import pytest

import khits_ref as kr
from sphere_ref import cluster_rays, cluster_scene, list_hits, tmax_draw
from test_gpu_any_hit import _rb
from test_khits_cpu import cluster_case, cube_case, pair_row_case, triangle_row_case

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
# both sides of every block-size threshold (256 / 128 / 64 lanes by the lists' bytes: k x (sizeof(T) + 4) x lanes <= 32 KB), 1 and the maximum
KS = {np.float32: (1, 2, 4, 16, 17, 32, 33, 64), np.float64: (1, 2, 4, 10, 11, 21, 22, 64)}


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


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.Context(0)


def _dev_rays(eng, rays):
    import torch
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    return eng.RayBatch.from_device(dev, len(rays), dt)


def _check(tree, rb, k, leaf, tmax, want, label=None):
    """khits_batch against (vals, shape) of khits_match, byte for byte; rays in HBM come back as torch tensors, shape as int32"""
    vals, shape = tree.khits_batch(rb, k, leaf, tmax)
    if not isinstance(vals, np.ndarray):
        import torch
        assert shape.dtype == torch.int32 and vals.is_cuda and shape.is_cuda
        vals, shape = vals.cpu().numpy(), shape.cpu().numpy().view(np.uint32)
    assert shape.dtype == np.uint32 and vals.dtype == want[0].dtype
    assert shape.shape == want[1].shape and vals.shape == want[0].shape, label
    assert shape.tobytes() == want[1].tobytes(), label
    assert vals.tobytes() == want[0].tobytes(), label
    return vals, shape


def _sphere_tree(eng, spheres, aabbs, ctx):
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_spheres(spheres)
    return flat


def _drawn_tmax(case, dtype, seed=31):
    """segment ends around each ray's nearest sphere distance, with pinned rows: NaN, 0, -1, +inf and exactly the nearest distance"""
    nearest = kr.khits_match(case["off"], case["idx"], case["sphere"], None, 1)[0][:, 0, 0]
    tmax = tmax_draw(np.random.default_rng(seed), nearest, dtype)
    hit = np.nonzero(np.isfinite(nearest))[0][:50]
    assert len(hit) == 50
    tmax[hit[0:10]] = np.nan
    tmax[hit[10:20]] = 0
    tmax[hit[20:30]] = -1
    tmax[hit[30:40]] = np.inf
    tmax[hit[40:50]] = nearest[hit[40:50]]
    return tmax


# ---- 1. the cluster scene: every k around the block-size thresholds, host and device memory -------------------------------------------
@pytest.mark.parametrize("leaf", ["box", "sphere"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_cluster_scene(eng, orc, ctx, dtype, leaf):
    import torch
    case = cluster_case(orc, dtype)
    off, idx, rays, rec = case["off"], case["idx"], case["rays"], case[leaf]
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    tmax = _drawn_tmax(case, dtype)
    rb_host, rb_dev = _rb(eng, rays), _dev_rays(eng, rays)
    tdev = torch.from_numpy(tmax.copy()).cuda()
    c_all, c_cut = kr.candidate_counts(off, rec), kr.candidate_counts(off, rec, tmax)
    assert (c_all > 4).mean() >= 0.10 and c_cut.sum() < c_all.sum() and (c_cut > 1).mean() > 0.05
    for k in KS[dtype]:
        for tm_host, tm_dev in ((None, None), (tmax, tdev)):
            want = kr.khits_match(off, idx, rec, tm_host, k)
            _check(flat, rb_host, k, leaf, tm_host, want, (k, "host"))
            _check(flat, rb_dev, k, leaf, tm_dev, want, (k, "device"))


# ---- 2. triangles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_triangle_parity(eng, orc, ctx, dtype):
    """12 000 triangles; 20 000 rays of the bench stream (they pass boxes and hit no triangle: rows of padding after a full walk) and
    20 000 rays aimed at the cubes"""
    for name in ("stream", "aimed"):
        case = cube_case(orc, dtype, name)
        off, idx, rays, rec = case["off"], case["idx"], case["rays"], case["triangle"]
        flat = eng.Bvh.from_aabbs(case["aabbs"], ctx).flatten()
        flat.set_triangles(case["tris"])
        c = case["closest"][:, 0].astype(np.float64)
        tmax = np.where(np.isfinite(c), c * np.random.default_rng(4).uniform(0.3, 1.7, size=len(c)), 4e5).astype(dtype)
        for k in (1, 4, 64):
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), k, "triangle", tm, kr.khits_match(off, idx, rec, tm, k), (name, k))
        _check(flat, _dev_rays(eng, rays), 4, "triangle", None, kr.khits_match(off, idx, rec, None, 4), (name, "device"))


# ---- 3. rows longer than k, ties, reversed lists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_row_scenes(eng, orc, ctx, dtype):
    case = pair_row_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rb = _rb(eng, case["rays"])
    # odd rays end exactly at a member's distance (strict: it and everything behind it stay out): +x ray i meets its second pair at 18 + i,
    # -x ray 32 + i enters the larger sphere of its second pair at 110 + i (the triangle rows: 18 + i is a pair there too)
    i = np.arange(64)
    tmax = np.where(i % 2 == 0, 100.0, np.where(i < 32, 18.0 + i, 110.0 + (i - 32))).astype(dtype)
    for leaf in ("box", "sphere"):
        for k in (1, 7, 63, 64):
            for tm in (None, tmax):
                _check(flat, rb, k, leaf, tm, kr.khits_match(case["off"], case["idx"], case[leaf], tm, k), (leaf, k))
        vals, shape = flat.khits_batch(rb, 7, leaf)
        # ray 0 from x = -10 along +x: the pairs at p = 0, 8, 16, the smaller shape (odd index) first in the list; exits p + 2 and p + 6
        assert shape[0].tolist() == [1, 0, 3, 2, 5, 4, 7]
        assert vals[0].tolist() == [[10, 12], [10, 16], [18, 20], [18, 24], [26, 28], [26, 32], [34, 36]]
        # ray 32 from x = 900 along -x: the pair at p = 792 first — the larger shape is entered at 900 - 798, the smaller at 900 - 794
        assert shape[32, :4].tolist() == [198, 199, 196, 197]
        assert vals[32, :4].tolist() == [[102, 108], [106, 108], [110, 116], [114, 116]]
    for alternate in (False, True):
        case = triangle_row_case(orc, dtype, alternate)
        flat = eng.Bvh.from_aabbs(case["aabbs"], ctx).flatten()
        flat.set_triangles(case["tris"])
        rb = _rb(eng, case["rays"])
        for k in (1, 7, 63, 64):
            for tm in (None, tmax):
                _check(flat, rb, k, "triangle", tm, kr.khits_match(case["off"], case["idx"], case["triangle"], tm, k), (alternate, k))
        vals, shape = flat.khits_batch(rb, 7, "triangle")
        if not alternate:
            assert shape[0].tolist() == [1, 0, 3, 2, 5, 4, 7] and vals[0, :, 0].tolist() == [10, 10, 18, 18, 26, 26, 34]
            assert vals[0, :2].tolist() == [[10, 0.375, 0.375], [10, 0.21875, 0.46875]]
            assert np.all(shape[32:] == NONE) and vals[32:].tobytes() == np.tile(np.array([np.inf, 0, 0], dtype), (32, 7, 1)).tobytes()
        else:
            assert shape[0].tolist() == [1, 0, 5, 4, 9, 8, 13] and vals[0, :, 0].tolist() == [10, 10, 26, 26, 42, 42, 58]
            assert shape[40, :4].tolist() == [199, 198, 195, 194] and vals[40, :2].tolist() == [[116, 0.375, 0.375], [116, 0.46875, 0.21875]]


# ---- 4. ray counts around the wave and the block ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_ray_counts(eng, orc, ctx, dtype):
    """k = 4 runs 256 lanes per block, k = 17 (f32) / 11 (f64) 128, k = 64 runs 64: 0, 1, a wave -1 / +0 / +1, and each block size + 1"""
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    tmax = _drawn_tmax(case, dtype)
    for k in (4, 17 if dtype == np.float32 else 11, 64):
        want = {leaf: kr.khits_match(case["off"], case["idx"], case[leaf], tmax, k) for leaf in ("box", "sphere")}
        for n in (0, 1, 63, 64, 65, 129, 257):
            for leaf in ("box", "sphere"):
                for rb in (_rb(eng, case["rays"][:n]), _dev_rays(eng, case["rays"][:n])) if n else (_rb(eng, case["rays"][:0]),):
                    tm = tmax[:n]
                    if rb.mem != 0:
                        import torch
                        tm = torch.from_numpy(tm.copy()).cuda()
                    _check(flat, rb, k, leaf, tm, (want[leaf][0][:n], want[leaf][1][:n]), (k, n, leaf))
    vals, shape = flat.khits_batch(_rb(eng, case["rays"][:0]), 5, "sphere")
    assert vals.shape == (0, 5, 2) and shape.shape == (0, 5)


# ---- 5. every kind of tree ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_tree_kinds(eng, orc, ctx, dtype):
    from bvh_amd import FlatBvh, spheres_aabbs
    centres, spheres = cluster_scene(dtype, 1000)
    rng = np.random.default_rng(6)
    moved = spheres.astype(np.float64)
    moved[:, :3] += rng.uniform(-0.4, 0.4, size=(len(spheres), 3))
    moved = moved.astype(dtype)
    aabbs, aabbs_moved = spheres_aabbs(spheres), spheres_aabbs(moved)
    rays, _ = cluster_rays(orc, centres, 8000, dtype, seed=12)
    built = orc.build(aabbs).nodes
    oflat = orc.flatten(built)

    def csr(flat_nodes, boxes):
        off, idx, ts, _ = orc.traverse_flat(flat_nodes, boxes, rays, want_t=True, threads=orc.max_threads())
        return off, idx, ts

    cases = []
    tree = _sphere_tree(eng, spheres, aabbs, ctx)                         # built here
    cases.append(("built", tree, csr(oflat, aabbs), spheres))
    up = FlatBvh.from_flat_nodes(oflat, aabbs_moved, ctx)                 # an uploaded FlatBvh: the old tree over the moved shapes
    up.set_spheres(moved)
    cases.append(("uploaded", up, csr(oflat, aabbs_moved), moved))
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)                                  # refitted: boxes moved, then refit
    bvh.refit(aabbs_moved)
    refitted = bvh.flatten()
    refitted.set_spheres(moved)
    cases.append(("refitted", refitted, csr(orc.flatten(orc.refit(built, aabbs_moved)), aabbs_moved), moved))
    blob = np.zeros(tree.scene_nbytes(), dtype=np.uint8)                  # scene-imported (carries no spheres)
    tree.scene_export(blob)
    imported = FlatBvh.scene_import(blob, len(blob), ctx)
    imported.set_spheres(spheres)
    cases.append(("imported", imported, csr(oflat, aabbs), spheres))
    for name, t, (off, idx, ts), sph in cases:
        recs = {"box": ts, "sphere": list_hits(off, idx, rays, sph)}
        tmax = tmax_draw(np.random.default_rng(13), kr.khits_match(off, idx, recs["sphere"], None, 1)[0][:, 0, 0], dtype)
        for leaf in ("box", "sphere"):
            assert kr.candidate_counts(off, recs[leaf]).max() > 3
            for k in (1, 3, 64):
                for tm in (None, tmax):
                    _check(t, _rb(eng, rays), k, leaf, tm, kr.khits_match(off, idx, recs[leaf], tm, k), (name, leaf, k))
    # a Bvh flattens in place first
    _check(eng.Bvh.from_aabbs(aabbs, ctx), _rb(eng, rays), 3, "box", None, kr.khits_match(*cases[0][2][:2], cases[0][2][2], None, 3), "Bvh")
    # one shape: a single (leaf) entry
    one = np.array([[0.5, 0.5, 1.5, 0.5]], dtype=dtype)
    o = np.array([[0.5, 0.5, 0], [0.5, 0.5, 0], [2, 2, 0], [0.5, 0.5, 3], [0.0625, 0.0625, 0]], dtype=dtype)
    r1 = orc.make_rays(o, np.tile(np.array([[0, 0, 1]], dtype=dtype), (len(o), 1)), dtype)
    t1 = np.array([np.inf, 1, np.inf, np.inf, np.inf], dtype=dtype)
    ab1 = spheres_aabbs(one)
    off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(ab1).nodes), ab1, r1, want_t=True)
    single = _sphere_tree(eng, one, ab1, ctx)
    for leaf, rec in (("box", ts), ("sphere", list_hits(off, idx, r1, one))):
        for k in (1, 2, 64):
            want = kr.khits_match(off, idx, rec, t1, k)
            _check(single, _rb(eng, r1), k, leaf, t1, want, ("one", leaf, k))
    assert kr.khits_match(off, idx, ts, t1, 2)[1].tolist() == [[0, NONE], [NONE, NONE], [NONE, NONE], [NONE, NONE], [0, NONE]]
    assert kr.khits_match(off, idx, list_hits(off, idx, r1, one), t1, 2)[1].tolist() == [[0, NONE]] + [[NONE, NONE]] * 4
    # no shapes: every slot is padding, for every leaf kind
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx).flatten()
    empty.set_spheres(np.zeros((0, 4), dtype))
    empty.set_triangles(np.zeros((0, 9), dtype))
    for leaf, w in (("box", 2), ("sphere", 2), ("triangle", 3)):
        for rb in (_rb(eng, r1), _dev_rays(eng, r1)):
            for k in (1, 5, 64):
                pad = np.zeros((len(r1), k, w), dtype)
                pad[:, :, 0] = np.inf
                _check(empty, rb, k, leaf, None, (pad, np.full((len(r1), k), NONE, np.uint32)), ("empty", leaf, k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_tree_with_empty_child_bounds(eng, orc, ctx, dtype):
    """the scene of the box and sphere tests of that name: splits without SAH winner leave empty child bounds in the tree"""
    rng = np.random.default_rng(9)
    big = 1e19 if dtype == np.float32 else 1e154
    g, t = 2.0 ** 41, 2.0 ** 42
    lo = (np.round(rng.uniform(-1, 1, size=(500, 3)) * big / g) * g).astype(dtype)
    tris = np.stack([lo, lo + np.array([0, 0, t], dtype), lo + np.array([t, 0, 0], dtype)], axis=1).astype(dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1).astype(dtype)
    spheres = np.concatenate([lo + np.array([t / 2, 0, t / 2], dtype), np.full((500, 1), t / 2, dtype)], axis=1).astype(dtype)
    n = 5000
    o = (lo[rng.integers(0, 500, size=n)] + np.array([t / 4, t, t / 4], dtype)).astype(dtype)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], dtype), (n, 1))
    d[::3] = rng.normal(size=(len(d[::3]), 3))
    d[1::3, 0] = 1e-3
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    assert np.isposinf(oflat[oflat["entry"] != NONE]["min"]).all(axis=1).any()   # the tree does have empty child bounds
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    isect, _, _ = orc.triangle_stage(tris, rays, off, idx)
    flat = _sphere_tree(eng, spheres, aabbs, ctx)
    flat.set_triangles(tris)
    tmax = np.where(np.arange(n) % 2 == 0, t / 2, 2 * t).astype(dtype)
    for leaf, rec in (("box", ts), ("sphere", list_hits(off, idx, rays, spheres)), ("triangle", isect)):
        assert leaf == "triangle" or kr.candidate_counts(off, rec).sum() > 500, leaf   # (in f64 no ray of this scene hits a triangle)
        for k in (1, 4):
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), k, leaf, tm, kr.khits_match(off, idx, rec, tm, k), (leaf, k))


# ---- 6. floating-point extremes ------------------------------------------------------------------------------------------------------
def _extreme_values(dtype):
    fi = np.finfo(dtype)
    return [np.nan, np.inf, -np.inf, float(fi.max), -float(fi.max), float(fi.smallest_subnormal), -float(fi.smallest_subnormal), -0.0]


def _extreme_rays(rays, dtype):
    """three of every four rays get one component of o, d or inv replaced by NaN / ±inf / ±max-finite / ±subnormal / -0"""
    r = rays.copy()
    vals = _extreme_values(dtype)
    i = np.arange(len(r))
    field, axis, v = i % 3, (i // 3) % 3, (i // 9) % len(vals)
    touch = i % 4 != 3
    with np.errstate(over="ignore"):
        for f, name in enumerate(("o", "d", "inv")):
            for a in range(3):
                m = touch & (field == f) & (axis == a)
                r[name][m, a] = np.asarray(vals, dtype=dtype)[v[m]]
    return r


def _extreme_tmax(n, dtype, seed):
    vals = _extreme_values(dtype) + [0.0, 1.0, 50.0, 3e3]
    t = np.asarray(vals, dtype=dtype)[np.arange(n) % len(vals)]
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=n) < 0.3, rng.uniform(0, 4e3, size=n).astype(dtype), t).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_fp_extremes(eng, orc, ctx, dtype):
    from test_gpu_fp_extremes import _caller_rays, _flat_plane_scene
    from bvh_amd import spheres_aabbs
    # (a) the cluster scene with NaN / inf / max-finite / subnormal / -0 in the rays' records and in tmax
    centres, spheres = cluster_scene(dtype, 500)
    aabbs = spheres_aabbs(spheres)
    base, _ = cluster_rays(orc, centres, 6000, dtype, seed=3)
    rays = _extreme_rays(np.ascontiguousarray(base), dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    recs = {"box": ts, "sphere": list_hits(off, idx, rays, spheres)}
    assert not np.isnan(ts[:, 0]).any()                                   # an entry is max(tmin, 0) of a slab test that rejects NaN
    assert not np.isnan(recs["sphere"][:, 0]).any()
    touched = np.arange(len(rays)) % 4 != 3
    counts = np.diff(off.astype(np.int64))
    assert (counts[touched] > 0).sum() > 200 and (counts[touched] == 0).sum() > 200
    tmax = _extreme_tmax(len(rays), dtype, seed=5)
    flat = _sphere_tree(eng, spheres, aabbs, ctx)
    for leaf in ("box", "sphere"):
        for k in (1, 4, 64):
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), k, leaf, tm, kr.khits_match(off, idx, recs[leaf], tm, k), (leaf, k))
    _check(flat, _dev_rays(eng, rays), 4, "sphere", None, kr.khits_match(off, idx, recs["sphere"], None, 4), "device")
    # (b) caller-built Ray records (inv = ±0 with overflowing differences, subnormal and huge inv, inv that is not 1/d) over triangles in
    # the plane x = 2^104 (2^971)
    tris, taabbs, X = _flat_plane_scene(dtype)
    crays, m = _caller_rays(dtype, X, 6000, seed=3)
    oflat = orc.flatten(orc.build(taabbs).nodes)
    off, idx, ts, _ = orc.traverse_flat(oflat, taabbs, crays, want_t=True, threads=orc.max_threads())
    isect, closest, _ = orc.triangle_stage(tris, crays, off, idx)
    assert not np.isnan(isect[:, 0]).any() and np.isfinite(closest[:, 0]).sum() > 50
    c = closest[:, 0].astype(np.float64)
    with np.errstate(over="ignore"):
        tmax = np.where(np.isfinite(c), c * np.random.default_rng(8).uniform(0.3, 1.7, size=len(c)), np.inf).astype(dtype)
    tmax[::7] = _extreme_tmax(len(tmax[::7]), dtype, seed=6)
    tflat = eng.Bvh.from_aabbs(taabbs, ctx).flatten()
    tflat.set_triangles(tris)
    for leaf, rec in (("box", ts), ("triangle", isect)):
        for k in (1, 4, 64):
            for tm in (None, tmax):
                _check(tflat, _rb(eng, crays), k, leaf, tm, kr.khits_match(off, idx, rec, tm, k), (leaf, k))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_khits_refusals(eng, orc):
    from bvh_amd import BvhGpuError, Context, _lib, spheres_aabbs
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, OVERFLOW, ptr
    lib = _lib.load()
    ctx = Context(0)
    spheres = np.array([[0.5, 0.5, 1.25, 0.25], [0.5, 0.5, 2.25, 0.25]], dtype=np.float32)
    aabbs = spheres_aabbs(spheres)
    o, d = np.array([[0.5, 0.5, 0]] * 4), np.array([[0, 0, 1]] * 4)
    rays = np.ascontiguousarray(orc.make_rays(o, d, np.float32))
    rays64 = np.ascontiguousarray(orc.make_rays(o, d, np.float64))
    tmax = np.full(4, 2.25, np.float32)
    f32, f64 = lib.bvhgpu_traverse_khits_f32, lib.bvhgpu_traverse_khits_f64
    SENT_S, SENT_V = 0xABCD1234, np.float32(-77.5)
    shape = np.full((4, 64), SENT_S, np.uint32)
    vals = np.full((4, 64, 3), SENT_V, np.float32)
    vals64 = np.full((4, 64, 3), -77.5, np.float64)

    def refused(rc, status, word, handle=ctx._h):
        assert rc == status, (rc, status, word)
        msg = lib.bvhgpu_last_error(handle).decode()
        assert word in msg, (word, msg)
        assert np.all(shape == SENT_S) and np.all(vals == SENT_V) and np.all(vals64 == -77.5), word   # a refused call touches no buffer

    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    refused(f32(None, ptr(rays), ptr(tmax), 4, HOST, 0, 2, ptr(shape), ptr(vals)), INVALID_ARG, "NULL tree", None)
    refused(f64(bvh._t, ptr(rays64), None, 4, HOST, 0, 2, ptr(shape), ptr(vals64)), DTYPE_MISMATCH, "dtype")
    refused(f32(bvh._t, ptr(rays), ptr(tmax), 4, HOST, 0, 2, ptr(shape), ptr(vals)), NOT_FLATTENED, "bvhgpu_flatten")
    flat = bvh.flatten()
    for k in (0, 65, 0xFFFFFFFF):
        refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, k, ptr(shape), ptr(vals)), INVALID_ARG, "BVHGPU_KHITS_MAX_K")
    refused(f32(flat._t, None, ptr(tmax), 4, HOST, 0, 2, ptr(shape), ptr(vals)), INVALID_ARG, "NULL argument")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, 2, None, ptr(vals)), INVALID_ARG, "NULL argument")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, 2, ptr(shape), None), INVALID_ARG, "NULL argument")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, 7, 0, 2, ptr(shape), ptr(vals)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    for leaf in (3, -1, 1 << 20):
        refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, leaf, 2, ptr(shape), ptr(vals)), INVALID_ARG, "BVHGPU_LEAF_BOX")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 1, 2, ptr(shape), ptr(vals)), INVALID_ARG, "bvhgpu_tree_set_triangles")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 2, 2, ptr(shape), ptr(vals)), INVALID_ARG, "bvhgpu_tree_set_spheres")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 0xFFFFFFFF, HOST, 0, 1, ptr(shape), ptr(vals)), OVERFLOW, "rays x k")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 1 << 26, HOST, 0, 64, ptr(shape), ptr(vals)), OVERFLOW, "rays x k")
    # the order of the checks: the first broken rule names itself
    refused(f32(flat._t, None, None, 4, 7, 9, 0, None, None), INVALID_ARG, "BVHGPU_KHITS_MAX_K")
    refused(f32(flat._t, None, None, 4, 7, 9, 2, None, None), INVALID_ARG, "NULL argument")
    refused(f32(flat._t, ptr(rays), None, 4, 7, 9, 2, ptr(shape), ptr(vals)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    refused(f32(flat._t, ptr(rays), None, 1 << 26, HOST, 9, 64, ptr(shape), ptr(vals)), INVALID_ARG, "BVHGPU_LEAF_BOX")
    refused(f32(flat._t, ptr(rays), None, 1 << 26, HOST, 2, 64, ptr(shape), ptr(vals)), INVALID_ARG, "bvhgpu_tree_set_spheres")
    # the Python surface
    rb = _rb(eng, rays)
    with pytest.raises(BvhGpuError, match="BVHGPU_KHITS_MAX_K"):
        flat.khits_batch(rb, 0)
    with pytest.raises(BvhGpuError, match="BVHGPU_KHITS_MAX_K"):
        flat.khits_batch(rb, 65)
    with pytest.raises(BvhGpuError, match="leaf"):
        flat.khits_batch(rb, 2, "cone")
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_spheres"):
        flat.khits_batch(rb, 2, "sphere")
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_triangles"):
        flat.khits_batch(rb, 2, "triangle")
    with pytest.raises(BvhGpuError):
        flat.khits_batch(_rb(eng, rays64), 2)                             # a ray dtype that differs
    with pytest.raises(BvhGpuError):
        flat.khits_batch(rb, 2, "box", tmax[:-1])
    with pytest.raises(BvhGpuError):
        flat.khits_batch(rb, 2, "box", tmax.astype(np.float64))
    # ... and a valid call after all that works: an empty batch with NULL pointers, then rows
    assert f32(flat._t, None, None, 0, HOST, 0, 2, None, None) == OK
    flat.set_spheres(spheres)
    off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(aabbs).nodes), aabbs, rays, want_t=True)
    out_s, out_v = np.zeros((4, 2), np.uint32), np.zeros((4, 2, 2), np.float32)
    for leaf, rec in ((0, ts), (2, list_hits(off, idx, rays, spheres))):
        want = kr.khits_match(off, idx, rec, tmax, 2)
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, leaf, 2, ptr(out_s), ptr(out_v)) == OK
        assert out_s.tobytes() == want[1].tobytes() and out_v.tobytes() == want[0].tobytes()
    assert want[1].tolist() == [[0, 1]] * 4 and want[0][0].tolist() == [[1.0, 1.5], [2.0, 2.5]]   # (both spheres start before tmax = 2.25)
    assert np.all(shape == SENT_S) and np.all(vals == SENT_V)


# ---- 8. neighbours -------------------------------------------------------------------------------------------------------------------
def test_khits_between_other_batches_on_one_tree(eng, orc, ctx):
    """a khits_batch between two traverse_batch / knearest_batch calls on the same tree and context leaves their results unchanged (it
    shares the context's staging buffer and the tree's arrays with them, and no result object)"""
    dtype = np.float32
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rb = _rb(eng, case["rays"])
    pts = np.random.default_rng(1).uniform(-1e3, 1e3, size=(3000, 3)).astype(dtype)
    off0, idx0, ts0, _ = flat.traverse_batch(rb, want_t=True)
    assert off0.tobytes() == case["off"].tobytes() and idx0.tobytes() == case["idx"].tobytes() and ts0.tobytes() == case["box"].tobytes()
    kn0 = flat.knearest_batch(pts, 5)
    cs0 = flat.closest_sphere_hits(rb)
    for leaf in ("box", "sphere"):
        for k in (1, 64):
            _check(flat, rb, k, leaf, None, kr.khits_match(case["off"], case["idx"], case[leaf], None, k), (leaf, k))
            off1, idx1, ts1, _ = flat.traverse_batch(rb, want_t=True)
            assert off1.tobytes() == off0.tobytes() and idx1.tobytes() == idx0.tobytes() and ts1.tobytes() == ts0.tobytes()
            kn1 = flat.knearest_batch(pts, 5)
            assert kn1[0].tobytes() == kn0[0].tobytes() and kn1[1].tobytes() == kn0[1].tobytes()
            _check(flat, _dev_rays(eng, case["rays"]), k, leaf, None, kr.khits_match(case["off"], case["idx"], case[leaf], None, k), (leaf, k, "device"))
            cs1 = flat.closest_sphere_hits(rb)
            assert cs1[0].tobytes() == cs0[0].tobytes() and cs1[1].tobytes() == cs0[1].tobytes()


# ---- 9. against the existing closest walks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_k1_equals_the_existing_closest_walks(eng, orc, ctx, dtype):
    """k = 1 rows with tmax None against closest_box_hits, closest_sphere_hits (cluster scene) and closest_hits (cube scene), GPU against
    GPU: a difference here with the other tests of this file passing is a finding about those walks"""
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rb = _rb(eng, case["rays"])
    vals, shape = flat.khits_batch(rb, 1, "box")
    sl, prim = flat.closest_box_hits(rb)
    assert vals[:, 0].tobytes() == sl.tobytes() and np.array_equal(shape[:, 0], prim)
    vals, shape = flat.khits_batch(rb, 1, "sphere")
    hit, prim = flat.closest_sphere_hits(rb)
    assert vals[:, 0].tobytes() == hit.tobytes() and np.array_equal(shape[:, 0], prim)
    for name in ("stream", "aimed"):
        case = cube_case(orc, dtype, name)
        tflat = eng.Bvh.from_aabbs(case["aabbs"], ctx).flatten()
        tflat.set_triangles(case["tris"])
        rb = _rb(eng, case["rays"])
        vals, shape = tflat.khits_batch(rb, 1, "triangle")
        isect, prim, _ = tflat.closest_hits(rb)
        assert vals[:, 0].tobytes() == isect.tobytes() and np.array_equal(shape[:, 0], prim), name
