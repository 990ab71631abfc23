"""Closest-hit and any-hit ray queries against the shapes' own boxes on the GPU (bvhgpu_traverse_box_*): per ray, among the shapes of
FlatBvh::traverse's list whose Ray::intersection_slice_for_aabb entry is < tmax (strict), the one entered first (the first of the list on
equal entries) or — BVHGPU_TRAVERSE_FIRST — the first of the list.  No triangles are set anywhere in this file.  Every check compares byte
for byte against the oracle's CSR row with t-slices pushed through the definition (test_box_hit_cpu.box_match), across walks, dtypes,
tree kinds, replays and error paths."""
import ctypes as C

import numpy as np
import pytest

from test_box_hit_cpu import box_match, three_box_scene
from test_gpu_any_hit import _aimed_rays, _cube_scene, _rb

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MODES = (("closest", False, 5), ("first", True, 6))   # (name, first, the walk kernels' MODE number)


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
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    return off, idx, ts


def _ask(flat, rays_b, tmax, first):
    return (flat.first_box_hits if first else flat.closest_box_hits)(rays_b, tmax)


def _check(flat, rays_b, tmax, first, want):
    sl, shape = _ask(flat, rays_b, tmax, first)
    assert sl.tobytes() == want[0].tobytes()
    assert np.array_equal(shape, want[1])
    return sl, shape


def _tmax_draw(rng, nearest, dtype):
    """per ray a segment end around the nearest entry (2e5 where nothing is hit): about half of the rays that hit keep a candidate"""
    c = nearest.astype(np.float64)
    span = np.where(np.isfinite(c), c, 2e5)
    return (span * rng.uniform(0.3, 1.7, size=len(c))).astype(dtype)


WALKS = [  # (tuning, kernel-name prefix) — {t} is the dtype's name, {m} the mode number
    ({0: 0, 3: 0}, "bvhgpu::k_traverse<{t}, {m}, false>"),
    ({0: 2, 3: 0}, "bvhgpu::k_traverse_lds<{t}, {m}, false>"),
    ({0: 3, 3: 0, 1: 0}, "bvhgpu::k_traverse_wide<{t}, {m}, 0,"),
    ({0: 3, 3: 0, 1: 2}, "bvhgpu::k_traverse_wide<{t}, {m}, 2,"),
    ({}, "bvhgpu::k_traverse_wide<{t}, {m}, 2,"),   # default tuning: 40 K rays go to the wide walk, 16 items per ray
]


def _tuned(tune):
    from bvh_amd import Context
    ctx = Context(0)
    for k, v in tune.items():
        ctx.set_tuning(k, v)
    return ctx


# ---- 1. parity by walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_parity_by_walk(eng, orc, dtype):
    from bvh_amd import testbase as tb
    _, aabbs = _cube_scene(tb, dtype)                                    # 36 000 triangle boxes, taken as bare AABBs
    tris, _ = _cube_scene(tb, dtype)
    n = 40000
    rays, rng = _aimed_rays(orc, tris, n, dtype, seed=11)
    off, idx, ts = _oracle(orc, aabbs, rays)
    want_none = {first: box_match(off, idx, ts, None, first) for _, first, _ in MODES}
    # what the scene exercises: most rays have a list, the nearest box is often not the first of the list, and the smallest entry is shared
    counts = np.diff(off.astype(np.int64))
    hit = counts > 0
    assert hit.mean() >= 0.5, hit.mean()
    assert (want_none[False][1][hit] != want_none[True][1][hit]).mean() >= 0.3
    rowmin = np.minimum.reduceat(ts[:, 0], off[:-1].astype(np.int64)[hit])
    shared = np.add.reduceat((ts[:, 0] == np.repeat(rowmin, counts[hit])).astype(np.int64), off[:-1].astype(np.int64)[hit])
    assert (shared >= 2).mean() >= 0.9, (shared >= 2).mean()
    tmax = _tmax_draw(rng, want_none[False][0][:, 0], dtype)
    # pinned rows: NaN, 0, -1, +inf, and exactly the entry of the first of the list (not admitted: strict <)
    special = np.nonzero(hit)[0][:50]
    tmax[special[0:10]] = np.nan
    tmax[special[10:20]] = 0
    tmax[special[20:30]] = -1
    tmax[special[30:40]] = np.inf
    tmax[special[40:50]] = ts[off[special[40:50]], 0]
    want = {first: box_match(off, idx, ts, tmax, first) for _, first, _ in MODES}
    cand = want[False][1] != NONE
    assert np.array_equal(cand, want[True][1] != NONE)                   # a ray has a candidate or not, whichever one is asked for
    assert 0.2 <= cand.mean() <= 0.8, cand.mean()                        # both outcomes on at least a fifth of the rays
    for first in (False, True):
        assert np.all(want[first][1][special[:30]] == NONE) and np.all(want[first][1][special[30:40]] != NONE)
    assert not np.any(want[True][1][special[40:50]] == idx[off[special[40:50]]])
    tname = "float" if dtype == np.float32 else "double"
    for tune, kernel in WALKS:
        flat = eng.Bvh.from_aabbs(aabbs, _tuned(tune)).flatten()
        rb = _rb(eng, rays)
        goff, gidx, gts, _ = flat.traverse_batch(rb, want_t=True)        # the GPU's own CSR with t-slices, through the definition
        for name, first, m in MODES:
            _check(flat, rb, None, first, want_none[first])
            assert flat.query_kernel().startswith(kernel.format(t=tname, m=m)), (tune, name, flat.query_kernel())
            _check(flat, rb, tmax, first, want[first])
            assert flat.query_kernel().startswith(kernel.format(t=tname, m=m)), (tune, name, flat.query_kernel())
            assert flat._hits.info()["total"] == int(cand.sum())
            g = box_match(goff, gidx, gts, tmax, first)
            assert g[0].tobytes() == want[first][0].tobytes() and np.array_equal(g[1], want[first][1])
            # single rays (one lane per launch whatever the tuning) with the pinned segment ends
            for r in special[::5]:
                s1, p1 = _ask(flat, _rb(eng, rays[r:r + 1]), tmax[r:r + 1], first)
                assert s1.tobytes() == want[first][0][r:r + 1].tobytes() and p1[0] == want[first][1][r]
        assert np.array_equal(flat.box_occluded(rb, tmax), cand)


# ---- 2. a node's entry is no lower bound for the shapes below it -----------------------------------------------------------------
INVERTED_SHIFT = (262144.0, 512.0, -1024.0)   # beside the cube scene (its bounds end at 1e5), on a grid where 3, 3.25 and 3.5 stay exact


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_inverted_box_below_a_later_node(eng, orc, dtype):
    """test_box_hit_cpu's three boxes inside the cube scene: the inverted box is entered at 3, an inner node above it only at 3.5 — a walk
    that skipped nodes by their entry (against tmax or against the best so far) would answer NONE / the wrong shape"""
    from bvh_amd import testbase as tb
    _, cubes = _cube_scene(tb, dtype)
    three, ray = three_box_scene(orc, dtype, INVERTED_SHIFT)
    aabbs = np.concatenate([cubes, three]).astype(dtype)
    inv = len(cubes) + 2
    oflat = orc.flatten(orc.build(aabbs).nodes)
    leaf = int(np.nonzero((oflat["entry"] == NONE) & (oflat["shape"] == inv))[0][0])
    above = np.nonzero((oflat["entry"][:leaf] != NONE) & (oflat["exit"][:leaf] > leaf))[0]
    enters = [orc.ray_slice(ray[0], np.concatenate([oflat["min"][i], oflat["max"][i]])) for i in above]
    assert all(e is not None for e in enters) and max(e[0] for e in enters) == 3.5   # every node above it is hit, one of them later than the box
    n = 40000
    rays = np.repeat(ray, n)
    tmax = np.where(np.arange(n) % 2 == 0, np.inf, 3.25).astype(dtype)
    off, idx, ts = _oracle(orc, aabbs, rays[:2], oflat)
    assert ts[idx == inv, 0].tolist() == [3.0, 3.0]
    want = {}
    for _, first, _ in MODES:
        for tm in (None, tmax):
            w2 = box_match(off, idx, ts, None if tm is None else tm[:2], first)
            want[first, tm is None] = (np.tile(w2[0], (n // 2, 1)), np.tile(w2[1], n // 2))
    assert np.all(want[False, True][1] == inv) and np.all(want[False, False][1] == inv)
    assert np.all(want[True, False][1][1::2] == inv) and np.all(want[True, False][1][0::2] != inv)
    tname = "float" if dtype == np.float32 else "double"
    for tune, kernel in WALKS:
        flat = eng.Bvh.from_aabbs(aabbs, _tuned(tune)).flatten()
        rb = _rb(eng, rays)
        for name, first, m in MODES:
            for tm in (None, tmax):
                _check(flat, rb, tm, first, want[first, tm is None])
                assert flat.query_kernel().startswith(kernel.format(t=tname, m=m)), (tune, name, flat.query_kernel())


# ---- 3. origins inside boxes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_origin_inside_enters_at_plus_zero(eng, orc, dtype):
    from bvh_amd import testbase as tb
    tris, _ = _cube_scene(tb, dtype)
    v = tris.reshape(-1, 36, 3)
    aabbs = np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1).astype(dtype)      # the 3000 whole cubes
    rng = np.random.default_rng(3)
    centres = (aabbs[:, :3].astype(np.float64) + aabbs[:, 3:].astype(np.float64)) / 2
    pick = rng.integers(0, len(aabbs), size=20000)
    rays = orc.make_rays(centres[pick].astype(dtype), rng.normal(size=(len(pick), 3)).astype(dtype), dtype)
    off, idx, ts = _oracle(orc, aabbs, rays)
    # closest: every ray starts inside a box, so the smallest entry is +0.  first: the first of the list is whichever box the tree's order
    # puts first, which the ray may enter later; it is the origin's own cube — entered at +0 — on the rows counted here
    own_first = idx[off[:-1]] == pick
    assert own_first.mean() >= 0.9, own_first.mean()
    zero = np.zeros(len(rays), dtype)
    for tune in ({}, {0: 0}, {0: 3, 3: 0, 1: 0}):
        flat = eng.Bvh.from_aabbs(aabbs, _tuned(tune)).flatten()
        for _, first, _ in MODES:
            sl, shape = _check(flat, _rb(eng, rays), None, first, box_match(off, idx, ts, None, first))
            assert np.all(shape != NONE)
            rows = own_first if first else np.ones(len(rays), bool)
            assert sl[rows, 0].tobytes() == zero[rows].tobytes()                  # +0 bitwise
            if first:
                assert np.array_equal(shape[rows], pick[rows].astype(np.uint32))
            _check(flat, _rb(eng, rays), np.zeros(len(rays), dtype), first, box_match(off, idx, ts, np.zeros(len(rays), dtype), first))


# ---- 4. a tree with a split without SAH winner -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_no_sah_winner_tree_takes_the_binary_walk(eng, orc, dtype):
    """the scene of the any-hit test of the same name: empty child bounds, which the wide walk does not accept"""
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
    d[1::3, 0] = 1e-3
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    assert np.isposinf(oflat[oflat["entry"] != NONE]["min"]).all(axis=1).any()   # the tree does have empty child bounds
    off, idx, ts = _oracle(orc, aabbs, rays, oflat)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    for tmax in (None, np.where(np.arange(n) % 2 == 0, t / 2, 2 * t).astype(dtype)):
        for _, first, _ in MODES:
            want = box_match(off, idx, ts, tmax, first)
            _check(flat, _rb(eng, rays), tmax, first, want)
            assert "k_traverse_wide" not in flat.query_kernel(), flat.query_kernel()
            if dtype == np.float32 and tmax is None:
                assert (want[1] != NONE).sum() > 1000


# ---- 5. trees whose shapes moved -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_uploaded_flat_bvh_and_refitted_tree(eng, orc, dtype):
    from bvh_amd import FlatBvh, testbase as tb
    tris, aabbs = _cube_scene(tb, dtype, 1000)
    rng = np.random.default_rng(6)
    step = rng.uniform(-0.4, 0.4, size=(len(aabbs), 3))
    moved = (aabbs.astype(np.float64) + np.concatenate([step, step], axis=1)).astype(dtype)
    rays, rng = _aimed_rays(orc, tris, 30000, dtype, seed=12)
    built = orc.build(aabbs).nodes
    oflat = orc.flatten(built)
    ctx = _tuned({})
    cases = []
    up = FlatBvh.from_flat_nodes(oflat, moved, ctx)                      # the old tree over the moved shapes: leaf tests use the shape AABBs
    cases.append((up, _oracle(orc, moved, rays, oflat)))
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    bvh.refit(moved)
    cases.append((bvh.flatten(), _oracle(orc, moved, rays, orc.flatten(orc.refit(built, moved)))))
    for flat, (off, idx, ts) in cases:
        nearest = box_match(off, idx, ts, None, False)[0][:, 0]
        assert np.isfinite(nearest).mean() > 0.3
        tmax = _tmax_draw(np.random.default_rng(13), nearest, dtype)
        for _, first, _ in MODES:
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), tm, first, box_match(off, idx, ts, tm, first))
    assert "k_traverse_wide" not in up.query_kernel() and "k_traverse_wide" in cases[1][0].query_kernel()


# ---- 6. wide-stack overflow ------------------------------------------------------------------------------------------------------
def test_box_hit_wide_stack_overflow_replays_through_the_binary_walk(eng, orc):
    """the deep tree of the any-hit overflow test: a ray through all 400 boxes outgrows the wide walk's stack; the batch is replayed
    with the binary walk, which reads the staged HOST tmax again"""
    from bvh_amd import testbase as tb
    x = 2.0 ** np.arange(400)
    aabbs = np.stack([x, np.zeros_like(x), np.zeros_like(x), x * 1.25, np.ones_like(x), np.ones_like(x)], 1).astype(np.float64)
    o = np.tile([[-1.0, 0.25, 0.25]], (128, 1))
    d = np.tile([[1.0, 0.0, 0.0]], (128, 1)); d[::7] = [1.0, 1e-300, 0.0]
    rays = orc.make_rays(o, d, np.float64)
    tmax = np.concatenate([np.full(64, 0.5), np.full(32, np.inf), np.full(32, 2.0 ** 200)])
    off, idx, ts = _oracle(orc, aabbs, rays)
    assert np.diff(off).min() == 400
    ctx = _tuned({0: 3, 3: 0})                                            # the wide walk for this small batch
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    for name, first, m in MODES:
        want = box_match(off, idx, ts, tmax, first)
        assert (want[1] == NONE).sum() == 64 and (want[1] != NONE).sum() == 64
        for items in (0, 2):
            ctx.set_tuning(1, items)
            _check(flat, _rb(eng, rays), tmax, first, want)
            assert flat.query_kernel().startswith("bvhgpu::k_traverse_lds<double, %d," % m), flat.query_kernel()   # replayed (the rays without a candidate walk all 400 boxes in either mode)
    # the result object goes on working with the wide walk afterwards
    tris_c, aabbs_c = _cube_scene(tb, np.float64, 300)
    flat2 = eng.Bvh.from_aabbs(aabbs_c, ctx).flatten()
    rays2, _ = _aimed_rays(orc, tris_c, 5000, np.float64, seed=2)
    off2, idx2, ts2 = _oracle(orc, aabbs_c, rays2)
    _check(flat2, _rb(eng, rays2), None, False, box_match(off2, idx2, ts2, None, False))
    assert flat2.query_kernel().startswith("bvhgpu::k_traverse_wide<double, 5, 2,")


# ---- 7. edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_one_shape_empty_tree_and_empty_batch(eng, orc, dtype):
    ctx = _tuned({})
    aabbs = np.array([[0, 0, 1, 1, 1, 2]], dtype=dtype)
    o = np.array([[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0], [2, 2, 0], [0.25, 0.25, 3], [0.5, 0.5, 1.5]], dtype=dtype)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], dtype=dtype)
    rays = orc.make_rays(o, d, dtype)
    tmax = np.array([np.inf, 1, 1.5, np.inf, np.inf, 0], dtype=dtype)
    off, idx, ts = _oracle(orc, aabbs, rays)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    for _, first, _ in MODES:
        want = box_match(off, idx, ts, tmax, first)
        assert want[1].tolist() == [0, NONE, 0, NONE, NONE, NONE]
        _check(flat, _rb(eng, rays), tmax, first, want)
        assert flat._hits.info()["total"] == 2
        sl, shape = _ask(flat, _rb(eng, rays[:0]), np.zeros(0, dtype), first)
        assert sl.shape == (0, 2) and shape.shape == (0,) and flat._hits.info()["total"] == 0
        assert _ask(flat, _rb(eng, rays[:0]), None, first)[1].shape == (0,)
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx).flatten()
    for _, first, _ in MODES:
        sl, shape = _ask(empty, _rb(eng, rays), tmax, first)
        assert sl.tobytes() == np.tile(np.array([[np.inf, 0]], dtype), (len(rays), 1)).tobytes() and np.all(shape == NONE)
        assert empty._hits.info()["total"] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_hit_device_rays_and_tmax(eng, orc, dtype):
    import torch
    from bvh_amd import BvhGpuError, RayBatch, testbase as tb
    tris, aabbs = _cube_scene(tb, dtype, 500)
    n = 30000
    rays, rng = _aimed_rays(orc, tris, n, dtype, seed=4)
    off, idx, ts = _oracle(orc, aabbs, rays)
    tmax = _tmax_draw(rng, box_match(off, idx, ts, None, False)[0][:, 0], dtype)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    rb = RayBatch.from_device(dev, n, dtype)
    tdev = torch.from_numpy(tmax.copy()).cuda()
    for _, first, _ in MODES:
        _check(flat, rb, tdev, first, box_match(off, idx, ts, tmax, first))
        _check(flat, rb, None, first, box_match(off, idx, ts, None, first))
        with pytest.raises(BvhGpuError):
            _ask(flat, rb, tmax, first)                                   # host tmax for rays in HBM
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tdev, first)                       # ... and the other way round
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tmax.astype(np.float64 if dtype == np.float32 else np.float32), first)
        with pytest.raises(BvhGpuError):
            _ask(flat, _rb(eng, rays), tmax[:-1], first)


def test_box_hit_result_object_reused_across_kinds(eng, orc):
    """one result object: CSR, box, any hit, closest hit — on the wide walk over items (the per-ray key and count buffers stay clean);
    every fetch refuses the result of another kind"""
    from bvh_amd import _lib, testbase as tb
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    from test_gpu_any_hit import first_match
    lib = _lib.load()
    tris, aabbs = _cube_scene(tb, np.float32)
    n = 40000
    rays, rng = _aimed_rays(orc, tris, n, np.float32, seed=8)
    off, idx, ts = _oracle(orc, aabbs, rays)
    oisect, oclosest, oprim = orc.triangle_stage(tris, rays, off, idx)
    tmax = _tmax_draw(rng, box_match(off, idx, ts, None, False)[0][:, 0], np.float32)
    flat = eng.Bvh.from_aabbs(aabbs, _tuned({})).flatten()
    flat.set_triangles(tris)                                             # (for the any-hit and closest-hit batches in between)
    rb = _rb(eng, rays)
    h = flat._hits.h
    buf3, buf2, shp, offs = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
    po, pi = C.c_void_p(), C.c_void_p()

    def refused_except(kind):
        calls = {"csr": lambda: lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST),
                 "box": lambda: lib.bvhgpu_hits_fetch_box(h, ptr(buf2), ptr(shp), HOST),
                 "any": lambda: lib.bvhgpu_hits_fetch_any(h, ptr(buf3), ptr(shp), HOST),
                 "closest": lambda: lib.bvhgpu_hits_fetch_closest(h, ptr(buf3), ptr(shp), HOST)}
        for k, call in calls.items():
            assert call() == (OK if k == kind else INVALID_ARG), (kind, k)
        assert lib.bvhgpu_hits_fetch_triangles(h, ptr(buf3), HOST) == INVALID_ARG
        assert lib.bvhgpu_hits_device(h, C.byref(po), C.byref(pi), None) == (OK if kind == "csr" else INVALID_ARG)

    for _ in range(2):
        goff, gidx, _, _ = flat.traverse_batch(rb)
        assert np.array_equal(goff, off) and np.array_equal(gidx, idx)
        refused_except("csr")
        for _, first, _ in MODES:
            _check(flat, rb, tmax, first, box_match(off, idx, ts, tmax, first))
            refused_except("box")
        isect, shape = flat.any_hits(rb, tmax)
        w = first_match(off, idx, oisect, tmax)
        assert isect.tobytes() == w[0].tobytes() and np.array_equal(shape, w[1])
        refused_except("any")
        _check(flat, rb, None, False, box_match(off, idx, ts, None, False))
        cl, prim, _ = flat.closest_hits(rb)
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
        refused_except("closest")
        _check(flat, rb, None, True, box_match(off, idx, ts, None, True))
    goff, gidx, _, _ = flat.traverse_batch(rb)
    assert np.array_equal(goff, off) and np.array_equal(gidx, idx)


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_box_hit_errors(eng, orc):
    from bvh_amd import Context, _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, ptr
    lib = _lib.load()
    ctx = Context(0)
    aabbs = np.array([[0, 0, 1, 1, 1, 1.5], [0, 0, 2, 1, 1, 2.5]], dtype=np.float32)
    rays = np.ascontiguousarray(orc.make_rays(np.array([[0.25, 0.25, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float32))
    rays64 = np.ascontiguousarray(orc.make_rays(np.array([[0.25, 0.25, 0]] * 4), np.array([[0, 0, 1]] * 4), np.float64))
    tmax = np.full(4, 2.25, np.float32)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    h = C.c_void_p()
    f32 = lib.bvhgpu_traverse_box_f32
    assert f32(bvh._t, ptr(rays), ptr(tmax), 4, HOST, 0, C.byref(h)) == NOT_FLATTENED
    flat = bvh.flatten()
    assert lib.bvhgpu_traverse_box_f64(flat._t, ptr(rays64), None, 4, HOST, 0, C.byref(h)) == DTYPE_MISMATCH
    for bad in (1, 2, 4, 8, 32, 64, 128, 256, 512, 2048, 1 << 20, 1 << 30, 1 << 31, 1024 | 1, 16 | 2):   # T_SLICE, STATS, ... and the internal marks
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, bad, C.byref(h)) == INVALID_ARG, bad
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, 7, 0, C.byref(h)) == INVALID_ARG           # no such memory kind
    assert f32(flat._t, None, None, 4, HOST, 0, C.byref(h)) == INVALID_ARG                  # NULL rays
    assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, None) == INVALID_ARG              # NULL result
    assert f32(flat._t, None, None, 0, HOST, 0, C.byref(h)) == OK                           # an empty batch
    sl = np.zeros((4, 2), np.float32)
    shape = np.zeros(4, np.uint32)
    total = C.c_uint64()
    off, idx, ts = _oracle(orc, aabbs, rays)
    for flags in (0, 16, 1024, 1024 | 16):                                                  # COHERENT is a hint, FIRST selects the mode
        want = box_match(off, idx, ts, tmax, (flags & 1024) != 0)
        assert f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, flags, C.byref(h)) == OK
        assert lib.bvhgpu_hits_fetch_box(h, ptr(sl), ptr(shape), HOST) == OK
        assert np.array_equal(shape, want[1]) and sl.tobytes() == want[0].tobytes() and np.all(shape != NONE)
        assert lib.bvhgpu_hits_info(h, None, C.byref(total), None) == OK and total.value == 4
        assert lib.bvhgpu_hits_fetch_box(h, None, ptr(shape), HOST) == OK and lib.bvhgpu_hits_fetch_box(h, ptr(sl), None, HOST) == OK
    # the public traverse entry ignores the box mark: an ordinary CSR batch comes out, which _fetch_box refuses
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), 4, HOST, 1 << 30, C.byref(h)) == OK
    assert lib.bvhgpu_hits_fetch_box(h, ptr(sl), ptr(shape), HOST) == INVALID_ARG
    offs = np.zeros(5, np.uint32)
    assert lib.bvhgpu_hits_fetch(h, ptr(offs), None, None, HOST) == OK and offs[-1] == 8
    lib.bvhgpu_hits_destroy(h)
    # the Python surface: tmax of the wrong dtype, length or memory is covered by test_box_hit_device_rays_and_tmax; a ray dtype that differs
    from bvh_amd import BvhGpuError
    with pytest.raises(BvhGpuError):
        flat.closest_box_hits(_rb(eng, rays64))
    with pytest.raises(BvhGpuError):
        flat.first_box_hits(_rb(eng, rays64))
