"""Nearest-first k-nearest over instanced scenes on the GPU (bvhgpu_instances_knearest_tree_*): every row byte for byte against
tests/instances_knn_tree_ref.py `rows` on the scenes tests/test_instances_knn_tree_cpu.py examines — the cluster scenes at every block
size of the block rule, HOST and HBM, without a limit, with a scalar, with one limit per point and with the special limits; point counts;
the ties of the line of instances; single leaves on both levels; padding and empty sets; splits without SAH winner on both levels; an
identity instance against the member's own knearest_tree_batch and the distances against the flat form's, GPU against GPU; the member
kinds the descent refuses; tree generations and the refusals of the raw C ABI.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import numpy as np
import pytest

import instances_knn_tree_ref as iktr
import instances_ref as ir
import instances_within_ref as iwr
import knn_ref as kr
from test_instances_cpu import SIZES, member_trees, transforms
from test_instances_knn_cpu import LINE_KS, N_POINTS, cluster
from test_instances_knn_tree_cpu import cluster_rows, limits_of, line_case

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KS = (1, 2, 5, 16, 64)        # blocks of 256, 256, 256, 128 and 64 lanes in both dtypes
NONE = iktr.NONE
NOT_BUILT = "the nearest-first descent needs the BvhNode array of every member tree"


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


def _gpu_trees(eng, ctx, trees):
    out = []
    for aabbs, tris in trees:
        flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris)
        out.append(flat)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_limit(m):
    """a limit for points in HBM: None and scalars as they are, n values as a GPU tensor"""
    return _dev(m) if isinstance(m, np.ndarray) else m


def _host(got):
    """(instance, shape, dist) as numpy, indices as uint32 (points in HBM come back as torch tensors)"""
    inst, shape, dist = got
    if not isinstance(inst, np.ndarray):
        import torch
        assert inst.dtype == torch.int32 and shape.dtype == torch.int32 and inst.is_cuda and shape.is_cuda and dist.is_cuda
        inst, shape, dist = inst.cpu().numpy().view(np.uint32), shape.cpu().numpy().view(np.uint32), dist.cpu().numpy()
    return inst, shape, dist


def _agree(got, rows, k, dtype, label):
    inst, shape, dist = _host(got)
    want = iktr.padded(rows, k, dtype)
    assert inst.dtype == np.uint32 and shape.dtype == np.uint32 and dist.dtype == dtype, label
    assert inst.shape == shape.shape == dist.shape == (len(rows), k), (label, inst.shape)
    assert inst.tobytes() == want[0].tobytes(), label
    assert shape.tobytes() == want[1].tobytes(), label
    assert kr.same(dist, want[2]), label                      # bytes; two NaNs are equal whatever their payload


def _block_lds(k, dtype):
    """the block rule of bvh_amd/csrc/instances_knn_tree.hip (instances_knn.hip's) → (lanes, bytes of LDS): the largest of 256 / 128 / 64
    lanes whose lists, k x (sizeof(T) + 8) bytes a lane, fit 32 KB; 64 lanes above that"""
    per_lane = k * (np.dtype(dtype).itemsize + 8)
    lanes = 256 if 256 * per_lane <= 32 * 1024 else 128 if 128 * per_lane <= 32 * 1024 else 64
    return lanes, lanes * per_lane


# ---- 1. the cluster scenes -----------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_block_size():
    for dt in DTYPES:
        assert {_block_lds(k, dt)[0] for k in KS} == {256, 128, 64}
        assert _block_lds(16, dt)[0] == 128 and _block_lds(5, dt)[0] == 256
    assert _block_lds(64, np.float64) == (64, 65536) and _block_lds(64, np.float32) == (64, 49152)      # the 65 536-byte launch


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene(eng, orc, ctx, dtype, n, k):
    """n = 1: the top level is one leaf record; n = 2, 37: member C is one leaf record; all 600 points, HOST and HBM; no limit, a scalar
    (as every point's limit), one limit per point and the special limits"""
    c, pts, _ = cluster(orc, dtype, n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    dpts = _dev(pts)
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for kind in ("none", "drawn", "special"):
            rows, _ = cluster_rows(orc, dtype, n, k, kind)
            m = limits_of(kind, dtype, n)
            _agree(inst.knearest_tree_batch(pts, k, m), rows, k, dtype, (n, k, kind, "host"))
            _agree(inst.knearest_tree_batch(dpts, k, _dev_limit(m)), rows, k, dtype, (n, k, kind, "device"))
        rows = iktr.rows(c["scene"], pts, k, 2.0, None, cluster(orc, dtype, n)[2])
        _agree(inst.knearest_tree_batch(pts, k, 2.0), rows, k, dtype, (n, k, "scalar", "host"))
        _agree(inst.knearest_tree_batch(dpts, k, max_dist=2.0), rows, k, dtype, (n, k, "scalar", "device"))
        _agree(inst.knearest_tree_batch(pts, k, np.full(N_POINTS, 2.0, dtype)), rows, k, dtype, (n, k, "scalar as an array"))
        if k == 1:
            for kind in ("none", "drawn"):
                want = iktr.padded(cluster_rows(orc, dtype, n, 1, kind)[0], 1, dtype)
                i1, s1, d1 = inst.nearest_tree_batch(pts, limits_of(kind, dtype, n))
                assert i1.shape == s1.shape == d1.shape == (N_POINTS,)
                assert i1.tobytes() == want[0].tobytes() and s1.tobytes() == want[1].tobytes() and d1.tobytes() == want[2].tobytes()


# ---- 2. point counts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_point_counts(eng, orc, ctx, dtype):
    c, pts, _ = cluster(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (5, 64):                                     # blocks of 256 and of 64 lanes
            for kind in ("none", "drawn"):
                rows, _ = cluster_rows(orc, dtype, 37, k, kind)
                lim = limits_of(kind, dtype, 37)
                for m in (0, 1, 63, 64, 65, 257):
                    cut = None if lim is None else np.ascontiguousarray(lim[:m])
                    _agree(inst.knearest_tree_batch(np.ascontiguousarray(pts[:m]), k, cut), rows[:m], k, dtype, (k, kind, m))
                cut = None if lim is None else _dev(lim[:65])
                _agree(inst.knearest_tree_batch(_dev(pts[:65]), k, cut), rows[:65], k, dtype, (k, kind, 65, "device"))
        gi, gs, gd = inst.knearest_tree_batch(pts[:0], 3)
        assert gi.shape == gs.shape == gd.shape == (0, 3) and gd.dtype == dtype
        gi, gs, gd = inst.knearest_tree_batch(_dev(pts[:0]), 3, 1.0)
        assert tuple(gi.shape) == tuple(gd.shape) == (0, 3)
        assert tuple(inst.nearest_tree_batch(pts[:0])[2].shape) == (0,)


# ---- 3. the line of instances: ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene(eng, orc, ctx, dtype):
    s = line_case(orc, dtype)
    trees = _gpu_trees(eng, ctx, s["trees"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        for k in LINE_KS:
            _agree(inst.knearest_tree_batch(s["points"], k), s["rows"][k], k, dtype, ("line", k))
            _agree(inst.knearest_tree_batch(_dev(s["points"]), k), s["rows"][k], k, dtype, ("line, device", k))
            _agree(inst.knearest_tree_batch(s["points"], k, 0.5), iktr.rows(s["scene"], s["points"], k, 0.5), k, dtype, ("line, limit", k))
        i2, s2, d2 = inst.knearest_tree_batch(s["points"][:2], 2)
        assert d2.tolist() == [[0.5, 0.5], [0.0, 0.0]] and sorted(i2[1].tolist()) == [0, 64]
        _, _, d64 = inst.knearest_tree_batch(s["points"], 64, 0.5)
        assert np.isfinite(d64).sum(axis=1).tolist() == [2, 2, 0, 4]           # ties at the limit are inside (<=)


# ---- 4. single leaves on both levels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_leaves(eng, orc, ctx, dtype):
    """record 0 is a leaf: the one-triangle member (member level), a one-instance set (top level), and both at once"""
    members = member_trees(orc, dtype)
    tri, cubes = members[2], members[1]
    pts = np.array([[0, 0, 0], [7, -3, 2], [-9, 1, 1], [2, 0.5, 0.1]], dtype=dtype)
    x1 = np.eye(3, 4, dtype=dtype)[None].copy()
    x1[0, 0, 3] = 2
    x2 = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x2[0, 0, 3], x2[1, 0, 3] = 2, -4
    for name, member, of, x in (("both", tri, [0], x1), ("member", tri, [0, 0], x2), ("top", cubes, [0], x1)):
        sc = ir.Scene([member], of, x, dtype)
        trees = _gpu_trees(eng, ctx, [member])
        with eng.Instances(trees, of, x, ctx) as inst:
            for k in (1, 2, 5, 64):
                for m in (None, 3.0, iktr.special_limits(len(pts), dtype)):
                    rows = iktr.rows(sc, pts, k, m)
                    _agree(inst.knearest_tree_batch(pts, k, m), rows, k, dtype, (name, k, "host"))
                    _agree(inst.knearest_tree_batch(_dev(pts), k, _dev_limit(m)), rows, k, dtype, (name, k, "device"))


# ---- 5. padding, empty sets --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_and_the_empty_set(eng, orc, ctx, dtype):
    """two instances of the one-triangle member: two entries and k - 2 padded slots; a limit that admits nothing: all padding; a set
    without instances: all padding, with and without limits"""
    tri = member_trees(orc, dtype)[2]
    x = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x[0, 0, 3], x[1, 0, 3] = 2, -4
    sc = ir.Scene([tri], [0, 0], x, dtype)
    pts = np.array([[0, 0, 0], [7, -3, 2], [-9, 1, 1]], dtype=dtype)
    trees = _gpu_trees(eng, ctx, [tri])
    with eng.Instances(trees, [0, 0], x, ctx) as inst:
        for k in (1, 2, 5, 64):
            rows = iktr.rows(sc, pts, k)
            assert all(len(r) == min(k, 2) for r in rows)
            _agree(inst.knearest_tree_batch(pts, k), rows, k, dtype, ("padding", k))
        gi, gs, gd = _host(inst.knearest_tree_batch(_dev(pts), 5))
        assert (gi[:, 2:] == NONE).all() and (gs[:, 2:] == NONE).all() and np.isposinf(gd[:, 2:]).all() and np.isfinite(gd[:, :2]).all()
        ti, _, _ = inst.knearest_tree_batch(_dev(pts), 5)
        assert (ti[:, 2:] == -1).all()                        # NONE reads -1 in torch.int32
        for m in (-1.0, np.nan, np.array([-0.5, np.nan, -np.inf], dtype=dtype)):
            gi, gs, gd = inst.knearest_tree_batch(pts, 5, m)
            assert (gi == NONE).all() and (gs == NONE).all() and np.isposinf(gd).all()
        gi, gs, gd = inst.nearest_tree_batch(pts, 1e-3)
        assert gi.tolist() == [NONE] * 3 and gs.tolist() == [NONE] * 3 and np.isposinf(gd).all()
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for k in (1, 5, 64):
            for p, m in ((pts, None), (_dev(pts), None), (pts, 2.0), (_dev(pts), _dev(np.ones(3, dtype)))):
                gi, gs, gd = _host(empty.knearest_tree_batch(p, k, m))
                assert gi.shape == (3, k) and (gi == NONE).all() and (gs == NONE).all() and np.isposinf(gd).all() and gd.dtype == dtype
        gi, gs, gd = empty.nearest_tree_batch(pts)
        assert gi.tolist() == [NONE] * 3 and np.isposinf(gd).all()


# ---- 6. splits without SAH winner --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("member", "top"))
def test_empty_child_bounds(eng, orc, ctx, dtype, which):
    """a built member whose root split has no SAH winner (both child boxes Aabb::empty(): cmd = 0, nothing is pruned there), and a top
    level with coincident world boxes whose split has none either; with ties between the coincident instances"""
    sc, (far, tris), x, pts = iktr.far_member_scene(dtype) if which == "member" else iktr.coincident_scene(dtype)
    top, members = iktr.node_arrays(sc)
    assert iktr.has_empty_child(members[0]) and (which == "member" or iktr.has_empty_child(top))
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    limit = dtype(0.3 * float(np.abs(pts[:150]).max()))
    cache = {}
    with eng.Instances([member], [0] * len(x), x, ctx) as inst:
        for k in ((1, 5, 64) if which == "member" else (1, 2, 7, 64)):
            for m in (None, limit, iktr.special_limits(len(pts), dtype)):
                rows = iktr.rows(sc, pts, k, m, None, cache)
                if which == "top" and k == 2 and m is None:
                    assert sum(1 for r in rows if len(r) == 2 and r[0][0] == r[1][0] and r[0][1] != r[1][1]) >= 50      # ties across instances
                _agree(inst.knearest_tree_batch(pts, k, m), rows, k, dtype, (which, k))


# ---- 7. anchors that do not pass through the new reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_members_own_knearest_tree(eng, orc, ctx, dtype):
    """GPU against GPU, bit for bit: the distances of every row, and the shapes of every row without a repeated distance (F = 3 widens the
    member's prune, which may change the order ties are met in, but never the row's distances)"""
    aabbs, tris = member_trees(orc, dtype)[1]
    assert not iktr.has_empty_child(orc.build(aabbs).nodes)
    B = _gpu_trees(eng, ctx, [(aabbs, tris)])[0]
    rng = np.random.default_rng(77)
    pts = rng.uniform(-5, 5, size=(400, 3)).astype(dtype)
    per_point = rng.uniform(0.1, 4.0, size=400).astype(dtype)
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        for k in (1, 5, 64):
            for m in (None, 1.5, per_point, iktr.special_limits(400, dtype)):
                shape, dist = B.knearest_tree_batch(pts, k, triangles=True, max_dist=m)
                gi, gs, gd = inst.knearest_tree_batch(pts, k, m)
                assert kr.same(gd, dist), k
                filled = gs != NONE
                assert np.array_equal(filled, shape != NONE) and (gi[filled] == 0).all() and (gi[~filled] == NONE).all()
                distinct = np.array([len(set(r[f].tolist())) == int(f.sum()) for r, f in zip(dist, filled)])
                assert distinct.all() or k > 1               # (the cubes' triangles share edges: longer rows often repeat a distance)
                assert gs[distinct].tobytes() == shape[distinct].tobytes(), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_distances_are_the_flat_forms(eng, orc, ctx, dtype):
    """GPU against GPU, without a limit: bit-equal distances to Instances.knearest_batch on the 37-instance scene"""
    c, pts, _ = cluster(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (1, 5, 64):
            fi, fs, fd = inst.knearest_batch(pts, k)
            ti, ts, td = inst.knearest_tree_batch(pts, k)
            assert td.tobytes() == fd.tobytes(), k
            assert (ti != NONE).all() and (ts != NONE).all()
        _, _, td = inst.knearest_tree_batch(pts, 5, np.inf)
        assert td.tobytes() == inst.knearest_batch(pts, 5)[2].tobytes()


# ---- 8. member kinds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_members_without_a_node_array_are_refused(eng, orc, ctx, dtype):
    """an uploaded FlatBvh and an imported scene carry no BvhNode array: INVALID_ARG with the message that names the flat form, which
    answers on the same sets"""
    c, pts, _ = cluster(orc, dtype, 37)
    sc = c["scene"]
    built = _gpu_trees(eng, ctx, c["trees"])
    up = eng.FlatBvh.from_flat_nodes(sc.flats[1], c["trees"][1][0], ctx)
    up.set_triangles(c["trees"][1][1])
    blob = np.zeros(built[1].scene_nbytes(), np.uint8)
    built[1].scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(c["trees"][1][1])
    for other in (up, imp):
        with eng.Instances([built[0], other, built[2]], c["tree_of"], c["x"], ctx) as inst:
            for call in (lambda: inst.knearest_tree_batch(pts, 3), lambda: inst.nearest_tree_batch(_dev(pts), 1.0)):
                with pytest.raises(eng.BvhGpuError) as e:
                    call()
                assert e.value.status == 1 and NOT_BUILT in str(e.value) and "bvhgpu_instances_knearest_*" in str(e.value)
            gi, _, _ = inst.knearest_batch(pts[:10], 3)
            assert gi.shape == (10, 3)


# ---- 9. tree generations -------------------------------------------------------------------------------------------------------------------
def test_tree_generations(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    dtype = np.float32
    trees = member_trees(orc, dtype)
    (a_aabbs, a_tris), (b_aabbs, b_tris) = trees[0], trees[1]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    x = transforms(5, dtype, 31)
    pts, lim = iwr.cluster_points(5, dtype, 300)

    def ref(tr, xf, k, m=None):
        return iktr.rows(ir.Scene([tr], [0] * 5, xf, dtype), pts, k, m)

    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.knearest_tree_batch(pts, 5), ref(trees[0], x, 5), 5, dtype, "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        for k in (1, 5):
            with pytest.raises(BvhGpuError) as e:
                inst.knearest_tree_batch(pts, k, lim)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        with pytest.raises(BvhGpuError) as e:
            inst.nearest_tree_batch(pts)
        assert "instances are stale" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x)
        new = (b_aabbs[:100], b_tris[:100])
        got = inst.knearest_tree_batch(pts, 5)                           # the first reader of the new generation is this entry
        _agree(got, ref(new, x, 5), 5, dtype, "after")
        _agree(inst.knearest_tree_batch(pts, 5, lim), ref(new, x, 5, lim), 5, dtype, "after, limited")
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        with pytest.raises(BvhGpuError) as e:
            inst.knearest_tree_batch(pts, 5)
        assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        # a re-pose: the rows follow the new pose
        x2 = transforms(5, dtype, 999)
        inst.update(x2)
        want2 = ref(new, x2, 5)
        got2 = inst.knearest_tree_batch(pts, 5)
        _agree(got2, want2, 5, dtype, "re-posed")
        assert got2[0].tobytes() != got[0].tobytes() or got2[2].tobytes() != got[2].tobytes()
        fresh_member = _gpu_trees(eng, ctx, [new])[0]
        with eng.Instances([fresh_member], [0] * 5, x2, ctx) as fresh:
            _agree(fresh.knearest_tree_batch(pts, 5), want2, 5, dtype, "re-posed against a fresh set")


# ---- 10. the refusals of the raw C ABI, in the header's order --------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype = np.float32
    k = 5
    c, pts_all, _ = cluster(orc, dtype, 37)
    rows = cluster_rows(orc, dtype, 37, k, "drawn")[0][:64]
    trees = _gpu_trees(eng, ctx, c["trees"])
    pts = np.ascontiguousarray(pts_all[:64])
    lim = np.ascontiguousarray(limits_of("drawn", dtype, 37)[:64])
    pts64, lim64 = pts.astype(np.float64), lim.astype(np.float64)
    f32, f64 = lib.bvhgpu_instances_knearest_tree_f32, lib.bvhgpu_instances_knearest_tree_f64
    STALE, UNCOMMITTED = "instances are stale: call bvhgpu_instances_update", "instances are not committed"
    oi, os_, od = np.full((64, 64), 0xABABABAB, np.uint32), np.full((64, 64), 0xABABABAB, np.uint32), np.full((64, 64), 7.0, dtype)
    od64 = np.full((64, 64), 7.0, np.float64)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text):
        assert rc == status and text in err(), (rc, err())
        assert (oi == 0xABABABAB).all() and (os_ == 0xABABABAB).all() and (od == 7.0).all() and (od64 == 7.0).all()

    member = eng.Bvh.from_aabbs(c["trees"][0][0], ctx)
    member.flatten_in_place()
    member.set_triangles(c["trees"][0][1])
    blob = np.zeros(trees[1].scene_nbytes(), np.uint8)
    trees[1].scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(c["trees"][1][1])
    eye = np.eye(3, 4, dtype=dtype)[None]
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances([member], [0] * 37, c["x"], ctx) as stale, \
            eng.Instances(trees, c["tree_of"], c["x"], ctx) as broken, eng.Instances([imp], [0], eye, ctx) as unbuilt:
        member.rebuild(c["trees"][1][0][:100], flatten=True)             # a member without triangles, of another generation
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        s = inst._s
        P, M, I, S, D = ptr(pts), ptr(lim), ptr(oi), ptr(os_), ptr(od)
        # each rule alone
        assert f32(None, P, 64, HOST, k, M, I, S, D) == INVALID_ARG
        refused(INVALID_ARG, INVALID_ARG, "")
        for bad_k in (0, _lib.INSTANCES_KNN_MAX_K + 1, 0xFFFFFFFF):
            refused(f32(s, P, 64, HOST, bad_k, M, I, S, D), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KNN_MAX_K")
        refused(f32(s, None, 64, HOST, k, M, I, S, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, M, None, S, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, None, I, None, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, M, I, S, None), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, 7, k, M, I, S, D), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE")
        refused(f64(s, ptr(pts64), 64, HOST, k, ptr(lim64), I, S, ptr(od64)), DTYPE_MISMATCH, "instance set dtype differs from point dtype")
        refused(f32(broken._s, P, 64, HOST, k, M, I, S, D), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, P, 64, HOST, k, M, I, S, D), INVALID_ARG, STALE)
        refused(f32(unbuilt._s, P, 64, HOST, k, M, I, S, D), INVALID_ARG, NOT_BUILT)
        refused(f32(unbuilt._s, P, 64, HOST, k, None, I, S, D), INVALID_ARG, "bvhgpu_instances_knearest_*")
        refused(f32(s, P, 1 << 26, HOST, 64, M, I, S, D), OVERFLOW, "too many results (points x k)")           # n * k = 2^32
        refused(f32(s, P, 0xFFFFFFFF, HOST, 1, M, I, S, D), OVERFLOW, "too many results (points x k)")
        # the order: an earlier rule wins over a later one
        refused(f64(stale._s, None, 0xFFFFFFFF, 7, 0, M, I, S, D), INVALID_ARG, "k must be")
        refused(f64(stale._s, None, 0xFFFFFFFF, 7, k, M, I, S, D), INVALID_ARG, "NULL argument")
        refused(f64(stale._s, P, 0xFFFFFFFF, 7, k, M, I, S, D), INVALID_ARG, "mem must be")
        refused(f64(stale._s, P, 0xFFFFFFFF, HOST, k, M, I, S, D), DTYPE_MISMATCH, "dtype")
        refused(f32(broken._s, P, 0xFFFFFFFF, HOST, k, M, I, S, D), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, P, 0xFFFFFFFF, HOST, k, M, I, S, D), INVALID_ARG, STALE)
        refused(f32(unbuilt._s, P, 0xFFFFFFFF, HOST, k, M, I, S, D), INVALID_ARG, NOT_BUILT)
        # the stale check is the flat form's: the same words from both
        assert lib.bvhgpu_instances_knearest_f32(stale._s, P, 64, HOST, k, I, S, D) == INVALID_ARG
        flat_words = err()
        assert f32(stale._s, P, 64, HOST, k, M, I, S, D) == INVALID_ARG and err() == flat_words
        # NULL buffers are fine where there is nothing to read or write
        assert f32(s, None, 0, HOST, k, None, None, None, None) == OK
        refused(OK, OK, "")
        # a later valid call still answers, on the set that refused and into the buffers that stayed untouched
        gi, gs, gd = np.zeros((64, k), np.uint32), np.zeros((64, k), np.uint32), np.zeros((64, k), dtype)
        assert f32(s, P, 64, HOST, k, M, ptr(gi), ptr(gs), ptr(gd)) == OK
        _agree((gi, gs, gd), rows, k, dtype, "after the refusals")
        _agree(inst.knearest_tree_batch(pts, k, lim), rows, k, dtype, "after the refusals, through the binding")
        # the binding refuses a k out of range by the engine's status, and a limit that does not fit the points before the engine is asked
        for bad_k in (0, 65, -1):
            with pytest.raises(_lib.BvhGpuError) as e:
                inst.knearest_tree_batch(pts, bad_k)
            assert e.value.status == INVALID_ARG and "k must be" in str(e.value)
        with pytest.raises(_lib.BvhGpuError) as e:
            inst.knearest_tree_batch(pts, k, lim[:63])
        assert e.value.status == INVALID_ARG and "max_dist has 63 values for 64 points" in str(e.value)
        with pytest.raises(_lib.BvhGpuError) as e:
            inst.knearest_tree_batch(pts, k, lim64)
        assert e.value.status == DTYPE_MISMATCH
