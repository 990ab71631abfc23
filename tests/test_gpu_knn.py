"""bvhgpu_knearest_* on the MI355X against its definition restated on the CPU (tests/knn_ref.py, over the oracle's FlatNode array and with
distances proven equal to the oracle's by tests/test_knn_cpu.py): shapes equal and distance bits equal (two NaNs count as equal) for
every scene, k, kind, dtype and memory space below."""
import numpy as np
import pytest

import knn_ref as kr
from test_knn_cpu import cube_scene, extreme_points, half_grid_queries, integer_cloud

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
KS = [1, 2, 3, 8, 33, 64]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


def _device_call(flat, pts, k, triangles):
    """torch tensor in, torch tensors out (shape as int32: NONE reads as -1) → numpy in the HOST call's dtypes"""
    import torch
    tp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    s, d = flat.knearest_batch(tp, k, triangles=triangles)
    assert s.is_cuda and d.is_cuda and s.dtype == torch.int32 and d.dtype == tp.dtype and tuple(s.shape) == tuple(d.shape) == (len(pts), k)
    sn = s.cpu().numpy()
    assert ((sn == -1) == (sn.view(np.uint32) == NONE)).all()
    return sn.view(np.uint32), d.cpu().numpy()


def _check(flat, oflat, aabbs, tris, pts, ks=KS, kinds=(0, 1), device=True, label=""):
    """every k and kind, HOST (and DEVICE), against the definition; returns the reference rows {(kind, k): (shape, dist)}"""
    want = {}
    for kind in kinds:
        ref = kr.knearest(oflat, aabbs, pts, ks, tris if kind else None)
        for k in ks:
            ws, wd = ref[k]
            want[(kind, k)] = (ws, wd)
            for mem in (("host", "device") if device else ("host",)):
                gs, gd = flat.knearest_batch(pts, k, triangles=bool(kind)) if mem == "host" else _device_call(flat, pts, k, bool(kind))
                assert gs.dtype == np.uint32 and gs.shape == (len(pts), k)
                bad = np.nonzero((gs != ws).any(axis=1))[0]
                assert len(bad) == 0, (label, kind, k, mem, "shapes differ in rows", bad[:5], gs[bad[:2]], ws[bad[:2]])
                assert kr.same(gd, wd), (label, kind, k, mem, "distances differ")
    return want


def _properties(shape, dist):
    """rows without a NaN are ascending in dist; the non-padding shapes of a row are distinct; padding is NONE / +inf at the row's end"""
    nan_row = np.isnan(dist).any(axis=1)
    d = dist[~nan_row]
    assert (d[:, 1:] >= d[:, :-1]).all()
    pad = shape == NONE
    assert (pad[:, 1:] >= pad[:, :-1]).all() and np.isinf(dist[pad]).all() and (dist[pad] > 0).all()
    srt = np.sort(shape.astype(np.int64), axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != NONE)
    assert not dup.any()


def _query_points(rng, aabbs, tris, dtype, n_uniform, n_surface, n_corner):
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    c, h = (lo + hi) / 2, (hi - lo)
    parts = [rng.uniform(c - h, c + h, size=(n_uniform, 3)).astype(dtype)]                  # twice the scene bounds
    pick = rng.integers(0, len(aabbs), n_surface)
    if tris is not None:
        w = rng.dirichlet([1, 1, 1], size=n_surface)
        parts.append(np.einsum("nk,nkd->nd", w, tris[pick].astype(np.float64)).astype(dtype))  # on the triangles (up to rounding)
    else:
        u = rng.uniform(size=(n_surface, 3))
        p = aabbs[pick, :3] + u * (aabbs[pick, 3:] - aabbs[pick, :3])
        p[:, 0] = aabbs[pick, 0]                                                             # on a face of the box
        parts.append(p.astype(dtype))
    corner = aabbs[rng.integers(0, len(aabbs), n_corner)][:, :3].astype(dtype)
    parts += [corner, corner[: max(1, n_corner // 2)]]                                       # duplicates of shape corners
    parts.append(extreme_points(dtype, c))
    return np.concatenate(parts)


def _build(eng, aabbs, tris=None):
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    if tris is not None:
        flat.set_triangles(tris)
    return flat


# ---------------------------------------------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("dtype", DTYPES)
def test_aligned_boxes_and_known_answers(eng, orc, dtype):
    boxes = orc.aligned_boxes().astype(dtype)
    flat = _build(eng, boxes)
    oflat = orc.flatten(orc.build(boxes).nodes)
    s, d = flat.knearest_batch(np.array([[0.25, 0, 0], [0.75, 0, 0], [0.5, 0, 0]], dtype=dtype), 3)
    assert s.tolist() == [[10, 11, 9], [11, 10, 12], [10, 11, 9]] and d.tolist() == [[0, 0.25, 0.75], [0, 0.25, 0.75], [0, 0, 1]]
    rng = np.random.default_rng(31)
    pts = _query_points(rng, boxes, None, dtype, 200, 60, 21)
    want = _check(flat, oflat, boxes, None, pts, kinds=(0,), label="aligned")
    assert (want[(0, 33)][0][:, 21:] == NONE).all() and (want[(0, 33)][0][:, :21] != NONE).all()   # fewer shapes than k: 12 padded slots


@pytest.mark.parametrize("n_cubes,n_uniform", [(100, 300), (1000, 800)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cube_scenes_both_kinds_host_and_device(eng, orc, dtype, n_cubes, n_uniform):
    """1 200 and 12 000 triangles.  Both triangles of a cube face share one AABB, so with kind 0 ties are everywhere."""
    tris, aabbs = cube_scene(n_cubes, dtype)
    assert (aabbs[0::2] == aabbs[1::2]).all(axis=1).mean() > 0.9                             # the premise: coincident AABBs
    flat = _build(eng, aabbs, tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    rng = np.random.default_rng(32 + n_cubes)
    pts = _query_points(rng, aabbs, tris, dtype, n_uniform, 100, 40)
    want = _check(flat, oflat, aabbs, tris, pts, device=(n_cubes == 100), label=f"cubes{n_cubes}")
    ws, wd = want[(0, 8)]
    fin = ~np.isnan(wd).any(axis=1)
    assert (wd[fin][:, 1:] == wd[fin][:, :-1]).any(axis=1).mean() > 0.5                      # ties within most rows
    for kind in (0, 1):                                                                      # k = 1 is nearest_batch
        s1, d1 = flat.knearest_batch(pts, 1, triangles=bool(kind))
        sn, dn = flat.nearest_batch(pts, triangles=bool(kind))
        assert np.array_equal(s1[:, 0], sn) and kr.same(d1[:, 0], dn)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_point_cloud_ties(eng, orc, dtype):
    """the cloud of tests/test_knn_cpu.py's exactness check ([0, 63]^3, ties at the k-th place are common), as zero-size boxes and as
    point triangles"""
    aabbs, tris = integer_cloud(dtype, 63)
    flat = _build(eng, aabbs, tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    _check(flat, oflat, aabbs, tris, half_grid_queries(dtype, 63, 128), label="cloud")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_trees_and_fewer_shapes_than_k(eng, orc, dtype):
    tris, aabbs = cube_scene(1, dtype)
    rng = np.random.default_rng(34)
    pts = _query_points(rng, aabbs, tris, dtype, 40, 10, 5)
    for n in (1, 2, 5):                                                                      # one shape: a single leaf entry, no navigator
        flat = _build(eng, aabbs[:n], tris[:n])
        oflat = orc.flatten(orc.build(aabbs[:n]).nodes)
        want = _check(flat, oflat, aabbs[:n], tris[:n], pts, label=f"n={n}")
        assert (want[(1, 8)][0][:, n:] == NONE).all() and np.isposinf(want[(1, 8)][1][:, n:]).all()
    empty = eng.Bvh.build([], dtype).flatten()
    for k in KS:
        for s, d in (empty.knearest_batch(pts, k), _device_call(empty, pts, k, False)):
            assert s.shape == d.shape == (len(pts), k) and (s == NONE).all() and np.isposinf(d).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_without_sah_winner(eng, orc, dtype):
    """boxes so far apart that every surface area overflows: no bucket wins, both children get EMPTY bounds (tests/test_gpu_parity.py),
    a child box is not the join of its grandchildren and the engine walks the unfolded array"""
    rng = np.random.default_rng(35)
    big = dtype(1e19 if dtype == np.float32 else 1e154)
    lo = (rng.uniform(-1, 1, size=(500, 3)) * big).astype(dtype)
    far = np.concatenate([lo, lo + big * dtype(0.01)], axis=1)
    pts = np.concatenate([(rng.uniform(-1, 1, size=(300, 3)) * big).astype(dtype), lo[:50], extreme_points(dtype, [0, 0, 0])])
    flat = _build(eng, far)
    oflat = orc.flatten(orc.build(far).nodes)
    _check(flat, oflat, far, None, pts, kinds=(0,), label="no SAH winner")


@pytest.mark.parametrize("dtype", DTYPES)
def test_later_candidates_pass_a_nan_in_the_list(eng, orc, dtype):
    """every 40th triangle blown up until its distance arithmetic overflows to NaN: the NaN enters a list that is not yet full, and finite
    candidates accepted LATER go in front of it (in front of the first element they are smaller than) — the rows the premise counts"""
    tris, _ = cube_scene(100, dtype)
    tris = tris.copy()
    tris[::40] *= dtype(1e30 if dtype == np.float32 else 1e160)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    flat = _build(eng, aabbs, tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    pts = np.random.default_rng(40).uniform(-3000, 3000, size=(200, 3)).astype(dtype)
    want = _check(flat, oflat, aabbs, tris, pts, kinds=(1,), label="NaN in the list")
    order = {s: i for i, s in enumerate(kr.leaf_preorder(oflat))}
    ws, wd = want[(1, 8)]
    passed = 0
    for r in range(len(pts)):
        nan_at = np.nonzero(np.isnan(wd[r]))[0]
        if len(nan_at) and any(order[int(ws[r, i])] > order[int(ws[r, nan_at[0]])] for i in range(nan_at[0])):
            passed += 1
    assert passed > 100, passed


def test_uploaded_flatbvh_and_scene_blob(eng, orc):
    tris, aabbs = cube_scene(100, np.float32)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    moved = aabbs.copy()
    moved[::3, [0, 3]] += np.float32(0.75)                                                   # stale navigator boxes, current shape distances
    rng = np.random.default_rng(36)
    pts = _query_points(rng, aabbs, tris, np.float32, 200, 50, 20)
    up = eng.FlatBvh.from_flat_nodes(oflat, moved)
    _check(up, oflat, moved, None, pts, kinds=(0,), label="uploaded")
    with pytest.raises(eng.BvhGpuError):
        up.knearest_batch(pts[:10], 3, triangles=True)                                       # no triangles were set on this tree
    flat = _build(eng, aabbs)
    blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
    flat.scene_export(blob)
    peer = eng.FlatBvh.scene_import(blob, len(blob))
    _check(peer, oflat, aabbs, None, pts, ks=[1, 8, 64], kinds=(0,), label="scene blob")


# ---------------------------------------------------------------------------------------------------------------- batch sizes
@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_sizes_around_block_boundaries(eng, orc, dtype):
    tris, aabbs = cube_scene(100, dtype)
    flat = _build(eng, aabbs, tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    rng = np.random.default_rng(37)
    pts = _query_points(rng, aabbs, tris, dtype, 257, 0, 1)[:257]
    ks = [1, 8, 33, 64]                                                                      # 256, 256 (f64: 128), 64 and 64 lanes per workgroup
    ref = kr.knearest(oflat, aabbs, pts, ks, tris)
    for n in (0, 1, 63, 64, 65, 255, 257):
        for k in ks:
            s, d = flat.knearest_batch(pts[:n], k, triangles=True)
            assert s.shape == (n, k) and np.array_equal(s, ref[k][0][:n]) and kr.same(d, ref[k][1][:n]), (n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_batch_sample_and_properties(eng, orc, dtype):
    """100 003 points: the definition is too slow for every row, so a seeded sample of 2 000 rows must equal it bit for bit and ALL rows
    must be ascending (where NaN-free) with distinct shapes"""
    tris, aabbs = cube_scene(100, dtype)
    flat = _build(eng, aabbs, tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    rng = np.random.default_rng(38)
    n = 100003
    base = _query_points(rng, aabbs, tris, dtype, n - 3000, 2000, 500)
    pts = np.concatenate([base, base[: n - len(base)]])[:n]
    assert len(pts) == n
    sample = np.sort(np.random.default_rng(39).choice(n, 2000, replace=False))
    for kind in (0, 1):
        ref = kr.knearest(oflat, aabbs, pts[sample], [8, 64], tris if kind else None)
        for k in (8, 64):
            s, d = flat.knearest_batch(pts, k, triangles=bool(kind)) if kind else _device_call(flat, pts, k, False)
            _properties(s, d)
            assert np.array_equal(s[sample], ref[k][0]) and kr.same(d[sample], ref[k][1]), (kind, k)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors(eng, orc):
    from bvh_amd import _lib
    lib = _lib.load()
    tris, aabbs = cube_scene(10, np.float32)
    bvh = eng.Bvh.from_aabbs(aabbs)
    pts = np.zeros((4, 3), dtype=np.float32)
    s = np.zeros((4, 64), dtype=np.uint32)
    d = np.zeros((4, 64), dtype=np.float32)

    def raw(tree, fn="bvhgpu_knearest_f32", k=3, kind=0, out_s=s, out_d=d, n=4, p=pts):
        return getattr(lib, fn)(tree._t, _lib.ptr(p), n, _lib.HOST, kind, k, _lib.ptr(out_s), _lib.ptr(out_d))

    assert raw(bvh) == _lib.NOT_FLATTENED                                                    # a Bvh that was never flattened
    flat = bvh.flatten()
    assert raw(flat) == _lib.OK
    assert raw(flat, k=0) == _lib.INVALID_ARG and raw(flat, k=65) == _lib.INVALID_ARG and raw(flat, k=64) == _lib.OK
    assert raw(flat, kind=2) == _lib.INVALID_ARG
    assert raw(flat, kind=1) == _lib.INVALID_ARG                                             # triangle distance without triangles
    assert raw(flat, fn="bvhgpu_knearest_f64", p=np.zeros((4, 3)), out_d=np.zeros((4, 64))) == _lib.DTYPE_MISMATCH
    assert raw(flat, out_s=None) == _lib.INVALID_ARG and raw(flat, out_d=None) == _lib.INVALID_ARG and raw(flat, p=None) == _lib.INVALID_ARG
    assert raw(flat, n=0, p=None, out_s=None, out_d=None) == _lib.OK                         # n = 0 is fine
    assert raw(flat, n=(1 << 32) // 64, k=64) == _lib.OVERFLOW                               # n x k reaches 2^32 (refused before anything is read)
    for k in (0, 65, -1):
        with pytest.raises(eng.BvhGpuError) as e:
            flat.knearest_batch(pts, k)
        assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(eng.BvhGpuError) as e:
        flat.knearest_batch(pts.astype(np.float64), 3)
    assert e.value.status == _lib.DTYPE_MISMATCH
    import torch
    with pytest.raises(eng.BvhGpuError) as e:
        flat.knearest_batch(torch.zeros((4, 3), dtype=torch.float64, device="cuda"), 3)
    assert e.value.status == _lib.DTYPE_MISMATCH
    with pytest.raises(eng.BvhGpuError) as e:
        flat.knearest_batch(pts, 3, triangles=True)
    assert e.value.status == _lib.INVALID_ARG
    flat.set_triangles(tris)
    assert raw(flat, kind=1) == _lib.OK
