"""bvhgpu_knearest_tree_* on the MI355X against its definition restated on the CPU (tests/knn_tree_ref.py, over the oracle's BvhNode array
and with distances proven equal to the oracle's by tests/test_knn_cpu.py): shapes equal and distance bits equal (two NaNs count as
equal) for every scene, k, kind, dtype, limit and memory space below; k = 1 without a limit against the oracle's Bvh::nearest_to itself."""
import numpy as np
import pytest

import knn_ref as kr
import knn_tree_ref as ktr
from test_gpu_knn import _properties, _query_points
from test_knn_cpu import cube_scene

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
KS = [1, 2, 3, 8, 33, 64]                       # 256 lanes per workgroup up to k = 16 (f32) / 10 (f64), 128 up to 32 / 21, 64 above


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


def _call(tree, pts, k, triangles, max_dist, mem):
    """HOST: numpy in, numpy out.  DEVICE: torch tensors in (a per-point limit too), torch out (shape as int32: NONE reads as -1) → numpy"""
    if mem == "host":
        s, d = tree.knearest_tree_batch(pts, k, triangles=triangles, max_dist=max_dist)
        assert s.dtype == np.uint32 and d.dtype == pts.dtype
        return s, d
    import torch
    tp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    md = torch.from_numpy(np.ascontiguousarray(max_dist)).cuda() if isinstance(max_dist, np.ndarray) else max_dist
    s, d = tree.knearest_tree_batch(tp, k, triangles=triangles, max_dist=md)
    assert s.is_cuda and d.is_cuda and s.dtype == torch.int32 and d.dtype == tp.dtype and tuple(s.shape) == tuple(d.shape) == (len(pts), k)
    sn = s.cpu().numpy()
    assert ((sn == -1) == (sn.view(np.uint32) == NONE)).all()
    return sn.view(np.uint32), d.cpu().numpy()


def _limit_properties(dist, max_dist, dtype):
    """every non-padding dist2 <= r2: sqrt is monotone and correctly rounded, so dist = sqrt(dist2) <= sqrt(r2), r2 = m * m rounded in T"""
    m = np.broadcast_to(np.asarray(max_dist, dtype=dtype), (len(dist),))
    with np.errstate(all="ignore"):
        top = np.sqrt((m * m).astype(dtype))
    ok = np.isposinf(dist) | (dist <= top[:, None])
    ok &= np.isposinf(dist) | (m >= 0)[:, None]
    nan_row = np.isnan(dist).any(axis=1)
    assert ok[~nan_row].all()


def _check(tree, nodes, aabbs, tris, pts, ks=KS, kinds=(0, 1), limits=(None,), mems=("host", "device"), label=""):
    """every k, kind, limit and memory space against the definition; returns the reference rows {(kind, limit index, k): (shape, dist)}"""
    want = {}
    for kind in kinds:
        refs = ktr.knearest_tree_limits(nodes, aabbs, pts, ks, tris if kind else None, limits)
        for li, lim in enumerate(limits):
            for k in ks:
                ws, wd = refs[li][k]
                want[(kind, li, k)] = (ws, wd)
                for mem in mems:
                    gs, gd = _call(tree, pts, k, bool(kind), lim, mem)
                    assert gs.shape == (len(pts), k)
                    bad = np.nonzero((gs != ws).any(axis=1))[0]
                    assert len(bad) == 0, (label, kind, li, k, mem, "shapes differ in rows", bad[:5], gs[bad[:2]], ws[bad[:2]])
                    assert kr.same(gd, wd), (label, kind, li, k, mem, "distances differ")
                    _properties(gs, gd)
                    if lim is not None:
                        _limit_properties(gd, lim, pts.dtype.type)
    return want


def _mixed_limits(rng, typical, n, dtype):
    """per-point limits: ordinary values around `typical`, and 0, a negative value, NaN and +inf"""
    m = (rng.uniform(0.25, 2.0, size=n) * typical).astype(dtype)
    m[1::7] = 0
    m[2::7] = -typical
    m[3::7] = np.nan
    m[4::7] = np.inf
    return m


# ---------------------------------------------------------------------------------------------------------------- scenes
@pytest.mark.parametrize("dtype", DTYPES)
def test_aligned_boxes_and_known_answers(eng, orc, dtype):
    boxes = orc.aligned_boxes().astype(dtype)
    bvh = eng.Bvh.from_aabbs(boxes)
    nodes = orc.build(boxes).nodes
    hand = np.array([[0.25, 0, 0], [0.75, 0, 0], [-3.25, 0.5, -0.5], [20, 0, 0]], dtype=dtype)
    s, d = bvh.knearest_tree_batch(hand, 3)
    assert s.tolist() == [[10, 11, 9], [11, 10, 12], [7, 6, 8], [20, 19, 18]]
    assert d.tolist() == [[0, 0.25, 0.75], [0, 0.25, 0.75], [0, 0.25, 0.75], [9.5, 10.5, 11.5]]
    s, d = bvh.knearest_tree_batch(hand, 3, max_dist=0.25)                                    # the limit itself is inside
    assert s.tolist() == [[10, 11, NONE], [11, 10, NONE], [7, 6, NONE], [NONE] * 3]
    assert d.tolist() == [[0, 0.25, np.inf], [0, 0.25, np.inf], [0, 0.25, np.inf], [np.inf] * 3]
    rng = np.random.default_rng(31)
    pts = _query_points(rng, boxes, None, dtype, 200, 60, 21)
    assert len(pts) % 256 != 0
    want = _check(bvh, nodes, boxes, None, pts, kinds=(0,), limits=(None, 2.0, _mixed_limits(rng, 2.0, len(pts), dtype)), label="aligned")
    assert (want[(0, 0, 33)][0][:, 21:] == NONE).all() and (want[(0, 0, 33)][0][:, :21] != NONE).all()   # fewer shapes than k: 12 padded slots
    filled = (want[(0, 1, 8)][0] != NONE).sum(axis=1)
    assert ((filled > 0) & (filled < 8)).any()                                                # the scalar limit leaves rows partly filled


@pytest.mark.parametrize("n_cubes,n_uniform,n_surface,n_corner", [(100, 300, 100, 40), (1000, 120, 60, 20)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cube_scenes_both_kinds_host_and_device(eng, orc, dtype, n_cubes, n_uniform, n_surface, n_corner):
    """1 200 and 12 000 triangles.  Both triangles of a cube face share one AABB, so with kind 0 ties are everywhere.
    Limits: a scalar of half a typical shape's box diagonal — a point on a cube reaches some of that cube's 12 triangles and not others,
    a point between the cubes reaches nothing — and a per-point mix around it."""
    tris, aabbs = cube_scene(n_cubes, dtype)
    bvh = eng.Bvh.from_aabbs(aabbs)
    bvh.set_triangles(tris)
    nodes = orc.build(aabbs).nodes
    rng = np.random.default_rng(32 + n_cubes)
    pts = _query_points(rng, aabbs, tris, dtype, n_uniform, n_surface, n_corner)
    assert len(pts) % 256 != 0
    diag = np.sqrt(((aabbs[:, 3:] - aabbs[:, :3]).astype(np.float64) ** 2).sum(axis=1))
    typical = dtype(np.median(diag) / 2)
    mems = ("host", "device") if n_cubes == 100 else ("host",)
    want = _check(bvh, nodes, aabbs, tris, pts, limits=(None, typical, _mixed_limits(rng, float(typical), len(pts), dtype)), mems=mems,
                  label=f"cubes{n_cubes}")
    for kind in (0, 1):                                                                       # k = 1: the oracle's Bvh::nearest_to itself
        ws, wd = orc.nearest(nodes, aabbs, pts, tris if kind else None)
        for mem in mems:
            s1, d1 = _call(bvh, pts, 1, bool(kind), None, mem)
            assert np.array_equal(s1[:, 0], ws) and kr.same(d1[:, 0], wd), (kind, mem)
    filled = (want[(1, 1, 8)][0] != NONE).sum(axis=1)
    assert ((filled > 0) & (filled < 8)).any() and (filled == 8).any() and (filled == 0).any()   # partly filled, full and empty rows


# ---------------------------------------------------------------------------------------------------------------- deep trees
@pytest.mark.parametrize("dtype,count,depth", [(np.float64, 300, 150), (np.float32, 40, 30)])
def test_deep_trees_have_no_depth_limit(eng, orc, dtype, count, depth):
    """boxes whose sizes grow eightfold: the SAH peels one box off per level and the tree is a chain"""
    x = 8.0 ** (np.arange(count) - count // 2)
    boxes = np.stack([x, 0 * x, 0 * x, 1.5 * x, 1 + 0 * x, 1 + 0 * x], axis=1).astype(dtype)
    nodes = orc.build(boxes).nodes
    assert orc.tree_stats(nodes, boxes)["max_depth"] >= depth
    bvh = eng.Bvh.from_aabbs(boxes)
    pick = x[:: max(1, count // 40)]
    along = np.stack([1.2 * pick, 0.5 + 0 * pick, 0.5 + 0 * pick], axis=1)                    # inside a box of the chain
    between = np.stack([3.0 * pick, 0.5 + 0 * pick, 0.5 + 0 * pick], axis=1)                  # in the gap behind it
    beside = np.stack([pick, 2.0 + 0 * pick, -3.0 + 0 * pick], axis=1)
    pts = np.concatenate([along, between, beside, -along, [[0, 0, 0], [0.5, 0.5, 0.5]]]).astype(dtype)
    rng = np.random.default_rng(41)
    _check(bvh, nodes, boxes, None, pts, ks=[1, 8, 64], kinds=(0,), limits=(None, _mixed_limits(rng, 1.0, len(pts), dtype)), label="chain")


# ---------------------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_shape_empty_tree_and_no_points(eng, orc, dtype):
    tris, aabbs = cube_scene(1, dtype)
    rng = np.random.default_rng(34)
    pts = _query_points(rng, aabbs, tris, dtype, 40, 10, 5)
    for n in (1, 2, 5):                                                                       # one shape: node 0 is a leaf
        bvh = eng.Bvh.from_aabbs(aabbs[:n])
        bvh.set_triangles(tris[:n])
        nodes = orc.build(aabbs[:n]).nodes
        assert (n > 1) or nodes["shape"][0] == 0
        want = _check(bvh, nodes, aabbs[:n], tris[:n], pts, ks=[1, 8], limits=(None, _mixed_limits(rng, 1.0, len(pts), dtype)), label=f"n={n}")
        assert (want[(1, 0, 8)][0][:, n:] == NONE).all() and np.isposinf(want[(1, 0, 8)][1][:, n:]).all()
    empty = eng.Bvh.build([], dtype)
    for k in KS:
        for mem in ("host", "device"):
            for lim in (None, 1.0):
                s, d = _call(empty, pts, k, False, lim, mem)
                assert s.shape == d.shape == (len(pts), k) and (s == NONE).all() and np.isposinf(d).all()
    bvh = eng.Bvh.from_aabbs(aabbs)
    for mem in ("host", "device"):
        s, d = _call(bvh, pts[:0], 8, False, None, mem)
        assert s.shape == d.shape == (0, 8)


# ---------------------------------------------------------------------------------------------------------------- build states
def test_build_states(eng, orc):
    import torch
    dtype = np.float32
    tris, aabbs = cube_scene(100, dtype)
    nodes = orc.build(aabbs).nodes
    rng = np.random.default_rng(36)
    pts = _query_points(rng, aabbs, tris, dtype, 150, 30, 10)
    ref = ktr.knearest_tree(nodes, aabbs, pts, [8])[8]
    bvh = eng.Bvh.from_aabbs(aabbs)                                                           # never flattened
    s, d = bvh.knearest_tree_batch(pts, 8)
    assert np.array_equal(s, ref[0]) and kr.same(d, ref[1])
    view = bvh.flatten()                                                                      # the view shares the built handle
    s, d = view.knearest_tree_batch(pts, 8)
    assert np.array_equal(s, ref[0]) and kr.same(d, ref[1])
    tris2, aabbs2 = cube_scene(37, dtype)                                                     # another scene into the same handle, no wait
    dev = torch.from_numpy(aabbs2).cuda()
    torch.cuda.synchronize()
    bvh.rebuild_async(dev)
    s, d = bvh.knearest_tree_batch(pts, 8)
    ref2 = ktr.knearest_tree(orc.build(aabbs2).nodes, aabbs2, pts, [8])[8]
    assert np.array_equal(s, ref2[0]) and kr.same(d, ref2[1])
    assert not np.array_equal(ref2[0], ref[0])
    bvh.rebuild(aabbs)                                                                        # and back, synchronously, not flattened
    s, d = bvh.knearest_tree_batch(pts, 8)
    assert np.array_equal(s, ref[0]) and kr.same(d, ref[1])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors(eng, orc):
    import torch
    from bvh_amd import _lib
    lib = _lib.load()
    tris, aabbs = cube_scene(10, np.float32)
    bvh = eng.Bvh.from_aabbs(aabbs)
    pts = np.zeros((4, 3), dtype=np.float32)
    s = np.zeros((4, 64), dtype=np.uint32)
    d = np.zeros((4, 64), dtype=np.float32)
    md = np.ones(4, dtype=np.float32)

    def raw(tree, fn="bvhgpu_knearest_tree_f32", k=3, kind=0, out_s=s, out_d=d, n=4, p=pts, m=None):
        return getattr(lib, fn)(tree._t, _lib.ptr(p), n, _lib.HOST, kind, k, _lib.ptr(m), _lib.ptr(out_s), _lib.ptr(out_d))

    assert raw(bvh) == _lib.OK and raw(bvh, m=md) == _lib.OK                                  # a Bvh that was never flattened is fine
    assert raw(bvh, k=0) == _lib.INVALID_ARG and raw(bvh, k=65) == _lib.INVALID_ARG and raw(bvh, k=64) == _lib.OK
    assert raw(bvh, kind=2) == _lib.INVALID_ARG
    assert raw(bvh, kind=1) == _lib.INVALID_ARG                                               # triangle distance without triangles
    assert raw(bvh, fn="bvhgpu_knearest_tree_f64", p=np.zeros((4, 3)), out_d=np.zeros((4, 64))) == _lib.DTYPE_MISMATCH
    assert raw(bvh, out_s=None) == _lib.INVALID_ARG and raw(bvh, out_d=None) == _lib.INVALID_ARG and raw(bvh, p=None) == _lib.INVALID_ARG
    assert raw(bvh, n=0, p=None, out_s=None, out_d=None) == _lib.OK                           # n = 0 is fine
    assert raw(bvh, n=(1 << 32) // 64, k=64) == _lib.OVERFLOW                                 # n x k reaches 2^32 (refused before anything is read)
    for k in (0, 65, -1):
        with pytest.raises(eng.BvhGpuError) as e:
            bvh.knearest_tree_batch(pts, k)
        assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(eng.BvhGpuError) as e:
        bvh.knearest_tree_batch(pts.astype(np.float64), 3)
    assert e.value.status == _lib.DTYPE_MISMATCH
    with pytest.raises(eng.BvhGpuError) as e:
        bvh.knearest_tree_batch(torch.zeros((4, 3), dtype=torch.float64, device="cuda"), 3)
    assert e.value.status == _lib.DTYPE_MISMATCH
    with pytest.raises(eng.BvhGpuError) as e:
        bvh.knearest_tree_batch(pts, 3, triangles=True)
    assert e.value.status == _lib.INVALID_ARG
    # max_dist in the wrong memory space, of the wrong length
    for p, m in ((pts, torch.ones(4, device="cuda")), (torch.zeros((4, 3), device="cuda"), md), (pts, np.ones(3, dtype=np.float32)),
                 (torch.zeros((4, 3), device="cuda"), torch.ones(5, device="cuda"))):
        with pytest.raises(eng.BvhGpuError) as e:
            bvh.knearest_tree_batch(p, 3, max_dist=m)
        assert e.value.status == _lib.INVALID_ARG
    # trees without a BvhNode array
    flat = bvh.flatten()
    up = eng.FlatBvh.from_flat_nodes(orc.flatten(orc.build(aabbs).nodes), aabbs)
    blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
    flat.scene_export(blob)
    peer = eng.FlatBvh.scene_import(blob, len(blob))
    for tree in (up, peer):
        assert raw(tree) == _lib.INVALID_ARG
        with pytest.raises(eng.BvhGpuError) as e:
            tree.knearest_tree_batch(pts, 3)
        assert e.value.status == _lib.INVALID_ARG and "BvhNode" in str(e.value)
    bvh.set_triangles(tris)
    assert raw(bvh, kind=1) == _lib.OK
