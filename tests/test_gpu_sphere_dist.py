"""bvhgpu_knearest_sphere_* / _knearest_tree_sphere_* / _within_sphere_* on the MI355X against their definitions restated on the CPU
(tests/sphere_dist_ref.py: the existing loops of knn_ref / knn_tree_ref / within_ref over the oracle's arrays, with the sphere distance at
the leaf): shapes equal and distance bits equal (two NaNs count as equal), in f32 and f64, with HOST and HBM points.
tests/test_sphere_dist_cpu.py shows on the reference alone what the scenes below contain."""
import functools

import numpy as np
import pytest

import knn_ref as kr
import sphere_dist_ref as sr
import test_fp_extremes_queries_cpu as q
import within_ref as wr
from test_knn_cpu import extreme_points
from test_sphere_dist_cpu import KS, within_limits
from test_within_cpu import far_scene

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
MEMS = ("host", "device")


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


@functools.lru_cache(maxsize=None)
def _scene(n, dtype):
    """ball_scene(n) with the oracle's arrays and the 300 query points: computed once, shared, never written to"""
    from oracle import orc
    spheres, aabbs = sr.ball_scene(n, dtype)
    nodes = orc.build(aabbs).nodes
    return dict(spheres=spheres, aabbs=aabbs, nodes=nodes, oflat=orc.flatten(nodes), pts=sr.query_points(spheres, dtype))


def _L():
    from bvh_amd import _lib
    return _lib


def _built(eng, aabbs, spheres):
    bvh = eng.Bvh.from_aabbs(aabbs)
    bvh.set_spheres(spheres)
    return bvh


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_out(s, d, n, k, tp=None):
    """torch rows (shape as int32: NONE reads as -1) -> numpy in the HOST call's dtypes"""
    if tp is None:
        assert s.dtype == np.uint32 and s.shape == d.shape == (n, k)
        return s, d
    import torch
    assert s.is_cuda and d.is_cuda and s.dtype == torch.int32 and d.dtype == tp.dtype and tuple(s.shape) == tuple(d.shape) == (n, k)
    return s.cpu().numpy().view(np.uint32), d.cpu().numpy()


def _knn(tree, pts, k, mem="host"):
    if mem == "host":
        return _rows_out(*tree.knearest_sphere_batch(pts, k), len(pts), k)
    tp = _dev(pts)
    return _rows_out(*tree.knearest_sphere_batch(tp, k), len(pts), k, tp)


def _knn_tree(tree, pts, k, m=None, mem="host"):
    if mem == "host":
        return _rows_out(*tree.knearest_tree_sphere_batch(pts, k, m), len(pts), k)
    tp = _dev(pts)
    return _rows_out(*tree.knearest_tree_sphere_batch(tp, k, _dev(m) if isinstance(m, np.ndarray) else m), len(pts), k, tp)


def _within(tree, pts, m, mem="host", sort=True, count_only=False):
    if mem == "host":
        o, s, d = tree.within_sphere_batch(pts, m, sort=sort, count_only=count_only)
        assert o.dtype == np.uint32 and s.dtype == np.uint32 and d.dtype == pts.dtype
        return o, s, d
    import torch
    tp = _dev(pts)
    o, s, d = tree.within_sphere_batch(tp, m if np.ndim(m) == 0 else _dev(m), sort=sort, count_only=count_only)
    assert o.is_cuda and s.is_cuda and d.is_cuda and o.dtype == torch.int64 and s.dtype == torch.int32 and d.dtype == tp.dtype
    return o.cpu().numpy().astype(np.uint32), s.cpu().numpy().view(np.uint32), d.cpu().numpy()


def _same_rows(got, want, label):
    gs, gd = got
    bad = np.nonzero((gs != want[0]).any(axis=1))[0]
    assert len(bad) == 0, (label, "shapes differ in rows", bad[:5], gs[bad[:2]], want[0][bad[:2]])
    assert kr.same(gd, want[1]), (label, "distances differ")


def _same_csr(got, want, label):
    o, s, d = got
    assert o.tobytes() == want[0].tobytes(), (label, "offsets", np.nonzero(o != want[0])[0][:5])
    assert s.shape == want[1].shape and d.dtype == want[2].dtype, label
    bad = np.nonzero(s != want[1])[0]
    assert len(bad) == 0, (label, "shapes differ at", bad[:5])
    assert d.tobytes() == want[2].tobytes(), (label, "distances")


def _check_within(tree, pts, m, rows, label, mems=MEMS):
    dtype = pts.dtype.type
    for sort in (True, False):
        want = wr.csr(rows, dtype, sort)
        for mem in mems:
            _same_csr(_within(tree, pts, m, mem, sort), want, (label, sort, mem))
    for mem in mems:
        o, s, d = _within(tree, pts, m, mem, True, True)
        assert o.tobytes() == want[0].tobytes() and s.shape == (0,) and d.shape == (0,), (label, "count only", mem)


def _mixed_limits(n, dtype, typical):
    """per point: ordinary values around `typical`, and 0, a negative value, NaN and +inf"""
    m = (np.random.default_rng(5).uniform(0.25, 2.0, size=n) * typical).astype(dtype)
    m[1::7], m[2::7], m[3::7], m[4::7] = 0, -typical, np.nan, np.inf
    return m


# ---------------------------------------------------------------------------------------------------------------- trees and k
@pytest.mark.parametrize("n", [1, 2, 12, 700, 2300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_form_on_built_trees(eng, dtype, n):
    """a Bvh (it flattens first) and its flatten(); every k on both sides of every topk_block boundary on the 700-sphere tree"""
    c = _scene(n, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    ks = KS if n == 700 else [1, 11, 64]
    want = sr.knearest(c["oflat"], c["aabbs"], c["spheres"], c["pts"], ks)
    for k in ks:
        for mem in MEMS:
            _same_rows(_knn(bvh, c["pts"], k, mem), want[k], (n, k, mem, "Bvh"))
    flat = bvh.flatten()
    for k in ks[:3]:
        _same_rows(_knn(flat, c["pts"], k), want[k], (n, k, "flatten()"))
    s1, d1 = flat.nearest_sphere_batch(c["pts"])                                       # k = 1 with the last axis dropped
    assert s1.shape == d1.shape == (len(c["pts"]),) and np.array_equal(s1, want[1][0][:, 0]) and kr.same(d1, want[1][1][:, 0])
    t1, e1 = flat.nearest_sphere_batch(_dev(c["pts"]))
    assert tuple(t1.shape) == (len(c["pts"]),) and np.array_equal(t1.cpu().numpy().view(np.uint32), s1) and kr.same(e1.cpu().numpy(), d1)


@pytest.mark.parametrize("n", [1, 2, 12, 700, 2300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tree_form_on_built_trees(eng, dtype, n):
    """max_dist None, a scalar and per point (with 0, negative, NaN and +inf); the tree need not be flattened"""
    c = _scene(n, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    ks = KS if n == 700 else [1, 11, 64]
    limits = (None, dtype(2.5), _mixed_limits(len(c["pts"]), dtype, 2.5))
    refs = sr.knearest_tree_limits(c["nodes"], c["aabbs"], c["spheres"], c["pts"], ks, limits)
    for li, lim in enumerate(limits):
        for k in ks:
            for mem in (MEMS if k in (1, 11, 64) else ("host",)):
                _same_rows(_knn_tree(bvh, c["pts"], k, lim, mem), refs[li][k], (n, k, li, mem))
    if n >= 12:
        filled = (refs[1][11][0] != NONE).sum(axis=1)
        assert (filled == 0).any() and ((filled > 0) & (filled < 11)).any()            # the scalar limit leaves rows empty and partly filled
    flat = sr.knearest(c["oflat"], c["aabbs"], c["spheres"], c["pts"], [11])[11]
    assert kr.same(refs[0][11][1], flat[1])                                            # the two forms agree in distances


@pytest.mark.parametrize("n", [1, 2, 12, 700])
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_on_built_trees(eng, dtype, n):
    c = _scene(n, dtype)
    flat = _built(eng, c["aabbs"], c["spheres"]).flatten()
    limits = (dtype(3), _mixed_limits(len(c["pts"]), dtype, 3.0))
    rows = sr.within_rows_multi(c["oflat"], c["aabbs"], c["spheres"], c["pts"], limits)
    for li, m in enumerate(limits):
        _check_within(flat, c["pts"], m, rows[li], (n, li))
    bvh = _built(eng, c["aabbs"], c["spheres"])                                        # a Bvh flattens first
    _same_csr(_within(bvh, c["pts"], limits[0]), wr.csr(rows[0], dtype), (n, "Bvh"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_every_tier_and_the_rows_beyond_lds(eng, dtype):
    """2 300 spheres: rows of length 0, up to 32 (lane tier), up to 2 048 (LDS tier) and, for the four points with max_dist = +inf,
    2 300 (sorted in global memory); the walk kernel is the sphere kernel"""
    c = _scene(2300, dtype)
    flat = _built(eng, c["aabbs"], c["spheres"]).flatten()
    m = within_limits(len(c["pts"]), dtype)
    rows = sr.within_rows(c["oflat"], c["aabbs"], c["spheres"], c["pts"], m)
    lens = np.array([len(ls) for _, ls in rows])
    assert (lens[:4] == 2300).all() and (lens == 0).any() and ((lens > 32) & (lens <= 2048)).any()
    _check_within(flat, c["pts"], m, rows, "tiers")
    t = "float" if dtype == np.float32 else "double"
    assert flat.query_kernel() == f"bvhgpu::k_within_count_sphere<{t}, false>"
    _within(flat, c["pts"][:4], np.inf)
    assert flat.query_kernel() == f"bvhgpu::k_within_fill_sphere<{t}, false, true>"
    _within(flat, c["pts"][:4], np.inf, sort=False)
    assert flat.query_kernel() == f"bvhgpu::k_within_fill_sphere<{t}, false, false>"


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_tree_and_no_points(eng, dtype):
    pts = _scene(12, dtype)["pts"][:65]
    empty = eng.Bvh.build([], dtype)
    empty.set_spheres(np.zeros((0, 4), dtype=dtype))
    for k in (1, 33):
        for mem in MEMS:
            for s, d in (_knn(empty, pts, k, mem), _knn_tree(empty, pts, k, None, mem), _knn_tree(empty, pts, k, dtype(1), mem)):
                assert (s == NONE).all() and np.isposinf(d).all()
    for mem in MEMS:
        o, s, d = _within(empty, pts, np.inf, mem)
        assert o.tolist() == [0] * 66 and s.shape == d.shape == (0,)
    c = _scene(12, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    for mem in MEMS:                                                                   # n == 0 points
        assert _knn(bvh, pts[:0], 3, mem)[0].shape == (0, 3) and _knn_tree(bvh, pts[:0], 3, None, mem)[1].shape == (0, 3)
        o, s, d = _within(bvh, pts[:0], dtype(1), mem)
        assert o.tolist() == [0] and s.shape == d.shape == (0,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_uploaded_flatbvh(eng, dtype):
    """FlatBvh.from_flat_nodes + set_spheres: the flat forms answer (over the unfolded array), the tree form has no BvhNode array"""
    c = _scene(700, dtype)
    up = eng.FlatBvh.from_flat_nodes(c["oflat"], c["aabbs"])
    up.set_spheres(c["spheres"])
    want = sr.knearest(c["oflat"], c["aabbs"], c["spheres"], c["pts"], [1, 17, 64])
    for k in want:
        for mem in MEMS:
            _same_rows(_knn(up, c["pts"], k, mem), want[k], ("uploaded", k, mem))
    m = _mixed_limits(len(c["pts"]), dtype, 3.0)
    _check_within(up, c["pts"], m, sr.within_rows(c["oflat"], c["aabbs"], c["spheres"], c["pts"], m), "uploaded")
    t = "float" if dtype == np.float32 else "double"
    assert up.query_kernel() == f"bvhgpu::k_within_count_sphere<{t}, true>"
    for mem in MEMS:
        with pytest.raises(eng.BvhGpuError) as e:
            _knn_tree(up, c["pts"], 3, None, mem)
        assert e.value.status == _L().INVALID_ARG


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_without_sah_winner_and_overflowing_s2(eng, orc, dtype):
    """boxes so far apart that no bucket wins a split: both children get EMPTY bounds and every family walks the unfolded arrays (within:
    the mirror).  Centres near 1e19 (f32) / 1e154 (f64): s2 overflows for most pairs, d = +inf"""
    far, _tris, pts, m = far_scene(dtype)
    pts, m = pts[::2], m[::2]
    spheres = sr.inscribed(far)
    nodes = orc.build(far).nodes
    oflat = orc.flatten(nodes)
    assert q.has_empty_child_bounds(oflat)
    with np.errstate(all="ignore"):
        assert np.isposinf(sr.sphere_dist2_v(spheres, pts[0])).any()
    bvh = _built(eng, far, spheres)
    ks = [1, 17, 64]
    want = sr.knearest(oflat, far, spheres, pts, ks)
    tree = sr.knearest_tree_limits(nodes, far, spheres, pts, ks, (None, m))
    for k in ks:
        _same_rows(_knn_tree(bvh, pts, k), tree[0][k], ("far tree", k))
        _same_rows(_knn_tree(bvh, pts, k, m, "device"), tree[1][k], ("far tree limit", k))
        for mem in MEMS:
            _same_rows(_knn(bvh, pts, k, mem), want[k], ("far flat", k, mem))
    _check_within(bvh, pts, m, sr.within_rows(oflat, far, spheres, pts, m), "far")
    t = "float" if dtype == np.float32 else "double"
    assert bvh.query_kernel() == f"bvhgpu::k_within_count_sphere<{t}, true>"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refitted_tree(eng, orc, dtype):
    """shapes move, the topology stays: the refitted boxes prune, the spheres set afterwards are read"""
    c = _scene(700, dtype)
    rng = np.random.default_rng(8)
    moved = c["aabbs"].copy()
    shift = rng.uniform(-1.5, 1.5, size=(len(moved), 3)).astype(dtype)
    moved[:, :3] += shift
    moved[:, 3:] += shift
    spheres = sr.inscribed(moved)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    bvh.flatten_in_place()
    bvh.refit(moved)
    bvh.set_spheres(spheres)
    nodes = orc.refit(c["nodes"], moved)
    oflat = orc.flatten(nodes)
    want = sr.knearest(oflat, moved, spheres, c["pts"], [1, 22])
    tree = sr.knearest_tree(nodes, moved, spheres, c["pts"], [1, 22], dtype(3))
    for k in (1, 22):
        _same_rows(_knn(bvh, c["pts"], k), want[k], ("refit flat", k))
        _same_rows(_knn_tree(bvh, c["pts"], k, dtype(3)), tree[k], ("refit tree", k))
    _check_within(bvh, c["pts"], dtype(3), sr.within_rows(oflat, moved, spheres, c["pts"], dtype(3)), "refit", mems=("host",))


# ---------------------------------------------------------------------------------------------------------------- k and batch sizes
@pytest.mark.parametrize("dtype", DTYPES)
def test_k_out_of_range_is_refused_with_outputs_untouched(eng, dtype):
    c = _scene(12, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    bvh.flatten_in_place()                                                             # (the raw flat entry is called below: NOT_FLATTENED comes before the k rule)
    lib = _L().load()
    sfx = "f32" if dtype == np.float32 else "f64"
    pts = np.ascontiguousarray(c["pts"][:5])
    for k in (0, 65):
        for entry, extra in (("knearest_sphere", ()), ("knearest_tree_sphere", (None,))):
            shape = np.full(5 * 65, 0xABABABAB, dtype=np.uint32)
            dist = np.full(5 * 65, -7, dtype=dtype)
            rc = getattr(lib, f"bvhgpu_{entry}_{sfx}")(bvh._t, _L().ptr(pts), 5, _L().HOST, k, *extra, _L().ptr(shape), _L().ptr(dist))
            assert rc == _L().INVALID_ARG and (shape == 0xABABABAB).all() and (dist == -7).all(), (k, entry)
        with pytest.raises(eng.BvhGpuError):
            bvh.knearest_sphere_batch(pts, k)
        with pytest.raises(eng.BvhGpuError):
            bvh.knearest_tree_sphere_batch(_dev(pts), k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_sizes_around_block_boundaries(eng, dtype):
    c = _scene(700, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    pts = c["pts"][:257]
    ks = [1, 17, 33]                                                                   # 256, 128 and 64 lanes per workgroup
    want = sr.knearest(c["oflat"], c["aabbs"], c["spheres"], pts, ks)
    tree = sr.knearest_tree(c["nodes"], c["aabbs"], c["spheres"], pts, ks, dtype(2.5))
    rows = sr.within_rows(c["oflat"], c["aabbs"], c["spheres"], pts, dtype(3))
    for n in (1, 63, 64, 65, 257):
        for k in ks:
            _same_rows(_knn(bvh, pts[:n], k, "device"), (want[k][0][:n], want[k][1][:n]), (n, k))
            _same_rows(_knn_tree(bvh, pts[:n], k, dtype(2.5)), (tree[k][0][:n], tree[k][1][:n]), (n, k, "tree"))
        _same_csr(_within(bvh, pts[:n], dtype(3), "device"), wr.csr(rows[:n], dtype), (n, "within"))


# ---------------------------------------------------------------------------------------------------------------- FP extremes
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp_extremes(eng, orc, dtype):
    """NaN / +-inf / max-finite / subnormal point components; r in {0, subnormal, negative, +inf, NaN} and a NaN centre on every 9th
    sphere over unchanged boxes; per-point limits with 0, negative, NaN and +inf"""
    c = _scene(700, dtype)
    fi = np.finfo(dtype)
    spheres = c["spheres"].copy()
    odd = np.array([0, float(fi.smallest_subnormal), -0.25, np.inf, np.nan], dtype=dtype)
    idx = np.arange(0, 700, 9)
    spheres[idx, 3] = np.resize(odd, len(idx))
    spheres[4::63, 0] = np.nan
    pts = np.concatenate([c["pts"][:120], extreme_points(dtype, [0, 0, 0])])
    bvh = _built(eng, c["aabbs"], spheres)
    ks = [1, 10, 64]
    want = sr.knearest(c["oflat"], c["aabbs"], spheres, pts, ks)
    m = _mixed_limits(len(pts), dtype, 3.0)
    tree = sr.knearest_tree_limits(c["nodes"], c["aabbs"], spheres, pts, ks, (None, m))
    assert np.isnan(want[64][1]).any()                                                 # NaN distances entered lists that were not full
    for k in ks:
        for mem in MEMS:
            _same_rows(_knn(bvh, pts, k, mem), want[k], ("extremes flat", k, mem))
        _same_rows(_knn_tree(bvh, pts, k), tree[0][k], ("extremes tree", k))
        _same_rows(_knn_tree(bvh, pts, k, m, "device"), tree[1][k], ("extremes tree limit", k))
    for lim in (m, np.inf):
        _check_within(bvh, pts, lim, sr.within_rows(c["oflat"], c["aabbs"], spheres, pts, lim), "extremes", mems=("host",))


@pytest.mark.parametrize("dtype", DTYPES)
def test_enlarged_spheres_follow_the_walk_not_brute_force(eng, dtype):
    """the CPU test's enlarged scene: spheres reach outside their boxes, some are pruned, and the engine gives the walk's rows"""
    c = _scene(700, dtype)
    big = sr.enlarged(c["spheres"])
    bvh = _built(eng, c["aabbs"], big)
    want = sr.knearest(c["oflat"], c["aabbs"], big, c["pts"], [10])[10]
    got = _knn(bvh, c["pts"], 10)
    _same_rows(got, want, "enlarged")
    brute = sr.brute_rows(c["oflat"], big, c["pts"], 10)
    assert any(not np.array_equal(got[0][r], kr.row(*b, 10, dtype)[0]) for r, b in enumerate(brute))
    _same_rows(_knn_tree(bvh, c["pts"], 10), sr.knearest_tree(c["nodes"], c["aabbs"], big, c["pts"], [10])[10], "enlarged tree")
    _same_csr(_within(bvh, c["pts"], dtype(1)), wr.csr(sr.within_rows(c["oflat"], c["aabbs"], big, c["pts"], dtype(1)), dtype), "enlarged within")


# ---------------------------------------------------------------------------------------------------------------- lifecycle
@pytest.mark.parametrize("dtype", DTYPES)
def test_lifecycle(eng, orc, dtype):
    a, b = _scene(700, dtype), _scene(12, dtype)
    pts = a["pts"][:65]
    bvh = eng.Bvh.from_aabbs(a["aabbs"])
    lib = _L().load()
    sfx = "f32" if dtype == np.float32 else "f64"

    def refused():
        """every method raises INVALID_ARG, and the raw entries leave sentinel-filled outputs untouched"""
        for fn in (lambda: bvh.knearest_sphere_batch(pts, 3), lambda: bvh.nearest_sphere_batch(pts), lambda: bvh.knearest_tree_sphere_batch(pts, 3),
                   lambda: bvh.within_sphere_batch(pts, 1.0), lambda: bvh.knearest_sphere_batch(_dev(pts), 3)):
            with pytest.raises(eng.BvhGpuError) as e:
                fn()
            assert e.value.status == _L().INVALID_ARG and "sphere distance needs bvhgpu_tree_set_spheres first" in str(e.value)
        p = np.ascontiguousarray(pts)
        shape, dist = np.full(65 * 3, 0xABABABAB, dtype=np.uint32), np.full(65 * 3, -7, dtype=dtype)
        for entry, extra in (("knearest_sphere", ()), ("knearest_tree_sphere", (None,))):
            rc = getattr(lib, f"bvhgpu_{entry}_{sfx}")(bvh._t, _L().ptr(p), 65, _L().HOST, 3, *extra, _L().ptr(shape), _L().ptr(dist))
            assert rc == _L().INVALID_ARG and (shape == 0xABABABAB).all() and (dist == -7).all()

    bvh.flatten_in_place()
    refused()                                                                          # before set_spheres
    bvh.set_spheres(a["spheres"])
    want_a = sr.knearest(a["oflat"], a["aabbs"], a["spheres"], pts, [3])[3]
    _same_rows(_knn(bvh, pts, 3), want_a, "first generation")
    bvh.rebuild(b["aabbs"], flatten=True)                                              # another shape count: the spheres are gone
    refused()
    bvh.set_spheres(b["spheres"])
    _same_rows(_knn(bvh, pts, 3), sr.knearest(b["oflat"], b["aabbs"], b["spheres"], pts, [3])[3], "12 spheres")
    # a rebuild with the same count keeps the spheres; the first call of each family reads the NEW tree: the boxes are mirrored in x, so
    # the walk order — and with it the order of ties and what is pruned — is the new tree's (the spheres are set to match)
    for first in ("knearest", "knearest_tree", "within"):
        bvh.rebuild(a["aabbs"], flatten=True)
        bvh.set_spheres(a["spheres"])
        _knn(bvh, pts, 3)
        mirrored = a["aabbs"].copy()
        mirrored[:, 0], mirrored[:, 3] = -a["aabbs"][:, 3], -a["aabbs"][:, 0]
        msph = sr.inscribed(mirrored)
        bvh.rebuild(mirrored, flatten=True)
        nodes = orc.build(mirrored).nodes
        oflat = orc.flatten(nodes)
        if first == "knearest":
            stale = _knn(bvh, pts, 3)                                                  # the old spheres over the new tree: still answered
            _same_rows(stale, sr.knearest(oflat, mirrored, a["spheres"], pts, [3])[3], "new tree, old spheres")
            assert not np.array_equal(stale[0], want_a[0])
            bvh.set_spheres(msph)
            _same_rows(_knn(bvh, pts, 3), sr.knearest(oflat, mirrored, msph, pts, [3])[3], "rebuilt, knearest first")
        elif first == "knearest_tree":
            bvh.set_spheres(msph)
            _same_rows(_knn_tree(bvh, pts, 3, dtype(2.5)), sr.knearest_tree(nodes, mirrored, msph, pts, [3], dtype(2.5))[3], "rebuilt, tree first")
        else:
            bvh.set_spheres(msph)
            _same_csr(_within(bvh, pts, dtype(3)), wr.csr(sr.within_rows(oflat, mirrored, msph, pts, dtype(3)), dtype), "rebuilt, within first")
    # a refit: same topology, moved boxes; the first call reads the refitted tree
    moved = mirrored.copy()
    moved[:, [0, 3]] += dtype(2)
    bvh.refit(moved)
    bvh.set_spheres(sr.inscribed(moved))
    rnodes = orc.refit(nodes, moved)
    got = _knn(bvh, pts, 3)
    _same_rows(got, sr.knearest(orc.flatten(rnodes), moved, sr.inscribed(moved), pts, [3])[3], "refitted")
    assert not kr.same(got[1], sr.knearest(oflat, mirrored, msph, pts, [3])[3][1])     # the two generations differ


# ---------------------------------------------------------------------------------------------------------------- cross-checks
@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_checks(eng, dtype):
    c = _scene(700, dtype)
    bvh = _built(eng, c["aabbs"], c["spheres"])
    tris = np.repeat(c["spheres"][:, None, :3], 3, axis=1).copy()
    bvh.set_triangles(tris)
    pts = c["pts"]
    before = [bvh.knearest_batch(pts, 8), bvh.knearest_batch(pts, 8, triangles=True), bvh.knearest_tree_batch(pts, 8, max_dist=2.5),
              bvh.within_batch(pts, 3.0), bvh.within_batch(pts, 3.0, triangles=True), bvh.nearest_batch(pts)]
    s1, d1 = _knn(bvh, pts, 1)
    sn, dn = bvh.nearest_sphere_batch(pts)
    assert np.array_equal(s1[:, 0], sn) and kr.same(d1[:, 0], dn)                      # k = 1 equals nearest_sphere_batch
    # a within row no longer than k holds the same pairs as the tree form with that limit
    m = _mixed_limits(len(pts), dtype, 2.0)
    o, s, d = _within(bvh, pts, m)
    ts, td = _knn_tree(bvh, pts, 64, m)
    short = 0
    for i in range(len(pts)):
        b, e = int(o[i]), int(o[i + 1])
        if e - b <= 64:
            short += 1
            assert sorted(s[b:e].tolist()) == sorted(ts[i, :e - b].tolist()) and (ts[i, e - b:] == NONE).all()
            assert kr.same(d[b:e], td[i, :e - b])
    assert short > 100
    bvh.set_spheres(sr.enlarged(c["spheres"]))                                       # ... whatever the spheres are
    _knn(bvh, pts, 8)
    after = [bvh.knearest_batch(pts, 8), bvh.knearest_batch(pts, 8, triangles=True), bvh.knearest_tree_batch(pts, 8, max_dist=2.5),
             bvh.within_batch(pts, 3.0), bvh.within_batch(pts, 3.0, triangles=True), bvh.nearest_batch(pts)]
    for x, y in zip(before, after):                                                    # kinds 0 and 1 are what they were
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and u.shape == v.shape and kr.same(u, v)
