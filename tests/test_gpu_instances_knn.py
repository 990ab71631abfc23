"""k-nearest over instanced scenes on the GPU (bvhgpu_instances_knearest_*): every row byte for byte against tests/instances_knn_ref.py on
the scenes tests/test_instances_knn_cpu.py shows to equal a brute force over all pairs — the cluster scenes at every block size of the
block rule, HOST and HBM; the ties of the line of instances; members and top levels of every served kind; an identity instance against
the member's own knearest_batch and k = 1 against the head of a radius search, GPU against GPU; point counts, padding and empty sets;
tree generations and the refusals of the raw C ABI.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as fz
import instances_knn_ref as ikr
import instances_ref as ir
import instances_within_ref as iwr
import knn_ref as kr
from test_instances_cpu import SIZES, member_trees, transforms
from test_instances_knn_cpu import LINE_KS, N_POINTS, cluster, cluster_rows, line_case
from test_within_cpu import far_scene

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KS = (1, 2, 5, 64)            # f32: blocks of 256, 256, 256 and 64 lanes; f64 the same
NONE = ikr.NONE


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
    want = ikr.padded(rows, k, dtype)
    assert inst.dtype == np.uint32 and shape.dtype == np.uint32 and dist.dtype == dtype, label
    assert inst.shape == shape.shape == dist.shape == (len(rows), k), (label, inst.shape)
    assert inst.tobytes() == want[0].tobytes(), label
    assert shape.tobytes() == want[1].tobytes(), label
    assert kr.same(dist, want[2]), label                      # bytes; two NaNs are equal whatever their payload


def _block_lds(k, dtype):
    """the block rule of bvh_amd/csrc/instances_knn.hip → (lanes, bytes of LDS)"""
    per_lane = k * (np.dtype(dtype).itemsize + 8)
    lanes = 256 if 256 * per_lane <= 32 * 1024 else 128 if 128 * per_lane <= 32 * 1024 else 64
    return lanes, lanes * per_lane


# ---- 1. the cluster scenes -----------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_block_size():
    lanes = {_block_lds(k, dt)[0] for k in KS + (16,) for dt in DTYPES}
    assert lanes == {256, 128, 64}
    assert _block_lds(64, np.float64) == (64, 65536) and _block_lds(64, np.float32) == (64, 49152)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene(eng, orc, ctx, dtype, n, k):
    """n = 1: the top level is one leaf entry; n = 2, 37: member C has one triangle; all 600 points, HOST and HBM"""
    c, pts, _ = cluster(orc, dtype, n)
    rows, _ = cluster_rows(orc, dtype, n, k)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        _agree(inst.knearest_batch(pts, k), rows, k, dtype, (n, k, "host"))
        _agree(inst.knearest_batch(_dev(pts), k), rows, k, dtype, (n, k, "device"))
        if k == 1:
            i1, s1, d1 = inst.nearest_batch(pts)
            want = ikr.padded(rows, 1, dtype)
            assert i1.shape == s1.shape == d1.shape == (N_POINTS,)
            assert i1.tobytes() == want[0].tobytes() and s1.tobytes() == want[1].tobytes() and d1.tobytes() == want[2].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_128_lane_block(eng, orc, ctx, dtype):
    """k = 16: the one block size the issue's k leave out"""
    assert _block_lds(16, dtype)[0] == 128
    c, pts, _ = cluster(orc, dtype, 37)
    rows, _ = cluster_rows(orc, dtype, 37, 16)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        _agree(inst.knearest_batch(pts, 16), rows, 16, dtype, "k = 16")


# ---- 2. the line of instances: ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene(eng, orc, ctx, dtype):
    s = line_case(orc, dtype)
    trees = _gpu_trees(eng, ctx, s["trees"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        for k in LINE_KS:
            _agree(inst.knearest_batch(s["points"], k), s["rows"][k], k, dtype, ("line", k))
            _agree(inst.knearest_batch(_dev(s["points"]), k), s["rows"][k], k, dtype, ("line, device", k))
        i2, s2, d2 = inst.knearest_batch(s["points"][:2], 2)
        assert d2.tolist() == [[0.5, 0.5], [0.0, 0.0]] and sorted(i2[1].tolist()) == [0, 64]


# ---- 3. members and top levels of every served kind ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_uploaded_flat_bvh_as_a_member(eng, orc, ctx, dtype):
    """member B as the oracle's FlatNode array uploaded (the UNFOLDED rule) beside the built A and C (folded), in one launch"""
    c, pts, _ = cluster(orc, dtype, 37)
    sc = c["scene"]
    built = _gpu_trees(eng, ctx, c["trees"])
    up = eng.FlatBvh.from_flat_nodes(sc.flats[1], c["trees"][1][0], ctx)
    up.set_triangles(c["trees"][1][1])
    with eng.Instances([built[0], up, built[2]], c["tree_of"], c["x"], ctx) as inst:
        for k in (1, 5, 64):
            _agree(inst.knearest_batch(pts, k), cluster_rows(orc, dtype, 37, k)[0], k, dtype, ("uploaded", k))


def _far_points(dtype, wt_a, wt_b):
    far, tris, pts, _ = far_scene(dtype)
    return np.ascontiguousarray(np.concatenate([pts[:150], wt_a[:50, 0], wt_b[100:150, 1]]))      # random points and points on world vertices


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_world_boxes_give_a_mirrored_top_level(eng, orc, ctx, dtype):
    """three instances of the far scene, two of whose world boxes coincide (a translation of 1 vanishes at 1e19): the top level's split has
    no SAH winner, its child bounds are empty and it is walked over its unfolded mirror, and so is the member; ties between the
    coincident instances"""
    far, tris, _, _ = far_scene(dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (3, 1, 1))
    x[1, :, 3] = [1, 2, 3]
    x[2, 0, 0] = 0.5
    sc = ir.Scene([(far, tris)], [0, 0, 0], x, dtype)
    assert fz.has_empty_child_bounds(sc.top) and sc.w[0].tobytes() == sc.w[1].tobytes() != sc.w[2].tobytes()
    wt = iwr.world_triangles(sc)
    pts = _far_points(dtype, wt[0], wt[2])
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    cache = {}
    with eng.Instances([member], [0, 0, 0], x, ctx) as inst:
        for k in (1, 2, 7, 64):
            rows = ikr.rows(sc, pts, k, None, cache)
            if k == 2:
                assert sum(1 for r in rows if len(r) == 2 and r[0][0] == r[1][0] and r[0][1] != r[1][1]) >= 50      # ties across instances
            _agree(inst.knearest_batch(pts, k), rows, k, dtype, ("coincident world boxes", k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_member_with_empty_child_bounds_built_and_imported(eng, orc, ctx, dtype):
    """boxes so far apart that no bucket wins a split: the built member is walked over its unfolded mirror; the same member after scene
    export / import carries the folded array only and is refused, outputs untouched"""
    far, tris, _, _ = far_scene(dtype)
    x = np.eye(3, 4, dtype=dtype)[None].copy()
    x[0, 0, 0], x[0, 1, 1] = 0.5, -2.0
    sc = ir.Scene([(far, tris)], [0], x, dtype)
    assert fz.has_empty_child_bounds(sc.flats[0])
    wt = iwr.world_triangles(sc)[0]
    pts = _far_points(dtype, wt, wt)
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    cache = {}
    with eng.Instances([member], [0], x, ctx) as inst:
        for k in (1, 5, 64):
            _agree(inst.knearest_batch(pts, k), ikr.rows(sc, pts, k, None, cache), k, dtype, ("empty child bounds", k))
    blob = np.zeros(member.scene_nbytes(), np.uint8)
    member.scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(tris)
    with eng.Instances([imp], [0], x, ctx) as inst:
        with pytest.raises(eng.BvhGpuError) as e:
            inst.knearest_batch(pts, 3)
        assert e.value.status == 1 and "split without SAH winner" in str(e.value)


# ---- 4. anchors that do not pass through the new reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_members_own_knearest(eng, orc, ctx, dtype):
    B = _gpu_trees(eng, ctx, [member_trees(orc, dtype)[1]])[0]
    rng = np.random.default_rng(77)
    pts = rng.uniform(-5, 5, size=(400, 3)).astype(dtype)
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        for k in (1, 5, 64):
            shape, dist = B.knearest_batch(pts, k, triangles=True)
            gi, gs, gd = inst.knearest_batch(pts, k)
            assert gs.tobytes() == shape.tobytes() and gd.tobytes() == dist.tobytes(), k
            assert (gi == 0).all() and gi.shape == (400, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nearest_is_the_head_of_the_radius_search(eng, orc, ctx, dtype):
    """for every point the k = 1 distance is bit-equal to the head of the sorted within_batch row at max_dist = +inf — and so is the pair"""
    c, pts, _ = cluster(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        gi, gs, gd = inst.nearest_batch(pts)
        w = inst.within_batch(pts, np.inf)
        heads = w["offsets"][:-1].astype(np.int64)
        assert (np.diff(w["offsets"].astype(np.int64)) == 3743).all()
        assert gd.tobytes() == w["dist"][heads].tobytes()
        assert gi.tobytes() == w["instance"][heads].tobytes() and gs.tobytes() == w["shape"][heads].tobytes()


# ---- 5. point counts, padding, empty sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_point_counts(eng, orc, ctx, dtype):
    c, pts, _ = cluster(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (5, 64):                                     # blocks of 256 and of 64 lanes
            rows, _ = cluster_rows(orc, dtype, 37, k)
            for m in (0, 1, 63, 64, 65, 257):
                _agree(inst.knearest_batch(np.ascontiguousarray(pts[:m]), k), rows[:m], k, dtype, (k, m))
            _agree(inst.knearest_batch(_dev(pts[:65]), k), rows[:65], k, dtype, (k, 65, "device"))
        gi, gs, gd = inst.knearest_batch(pts[:0], 3)
        assert gi.shape == gs.shape == gd.shape == (0, 3) and gd.dtype == dtype
        gi, gs, gd = inst.knearest_batch(_dev(pts[:0]), 3)
        assert tuple(gi.shape) == tuple(gd.shape) == (0, 3)
        assert tuple(inst.nearest_batch(pts[:0])[2].shape) == (0,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding(eng, orc, ctx, dtype):
    """two instances of the one-triangle member: two entries and k - 2 padded slots; a set without instances: all padding"""
    tri = member_trees(orc, dtype)[2]
    x = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x[0, 0, 3], x[1, 0, 3] = 2, -4
    sc = ir.Scene([tri], [0, 0], x, dtype)
    pts = np.array([[0, 0, 0], [7, -3, 2], [-9, 1, 1]], dtype=dtype)
    trees = _gpu_trees(eng, ctx, [tri])
    with eng.Instances(trees, [0, 0], x, ctx) as inst:
        for k in (1, 2, 5, 64):
            rows = ikr.rows(sc, pts, k)
            assert all(len(r) == min(k, 2) for r in rows)
            _agree(inst.knearest_batch(pts, k), rows, k, dtype, ("padding", k))
        gi, gs, gd = _host(inst.knearest_batch(_dev(pts), 5))
        assert (gi[:, 2:] == NONE).all() and (gs[:, 2:] == NONE).all() and np.isposinf(gd[:, 2:]).all() and np.isfinite(gd[:, :2]).all()
        ti, _, _ = inst.knearest_batch(_dev(pts), 5)
        assert (ti[:, 2:] == -1).all()                        # NONE reads -1 in torch.int32
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for k in (1, 5, 64):
            for p in (pts, _dev(pts)):
                gi, gs, gd = _host(empty.knearest_batch(p, k))
                assert gi.shape == (3, k) and (gi == NONE).all() and (gs == NONE).all() and np.isposinf(gd).all() and gd.dtype == dtype
        gi, gs, gd = empty.nearest_batch(pts)
        assert gi.tolist() == [NONE] * 3 and np.isposinf(gd).all()


# ---- 6. tree generations -------------------------------------------------------------------------------------------------------------------
def test_tree_generations(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    dtype = np.float32
    trees = member_trees(orc, dtype)
    (a_aabbs, a_tris), (b_aabbs, b_tris) = trees[0], trees[1]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    x = transforms(5, dtype, 31)
    pts, _ = iwr.cluster_points(5, dtype, 300)

    def ref(tr, xf, k):
        return ikr.rows(ir.Scene([tr], [0] * 5, xf, dtype), pts, k)

    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.knearest_batch(pts, 5), ref(trees[0], x, 5), 5, dtype, "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        for k in (1, 5):
            with pytest.raises(BvhGpuError) as e:
                inst.knearest_batch(pts, k)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        with pytest.raises(BvhGpuError) as e:
            inst.nearest_batch(pts)
        assert "instances are stale" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x)
        new = (b_aabbs[:100], b_tris[:100])
        got = inst.knearest_batch(pts, 5)                                # the first reader of the new generation is this entry
        _agree(got, ref(new, x, 5), 5, dtype, "after")
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        with pytest.raises(BvhGpuError) as e:
            inst.knearest_batch(pts, 5)
        assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        # a re-pose: the rows follow the new pose
        x2 = transforms(5, dtype, 999)
        inst.update(x2)
        want2 = ref(new, x2, 5)
        got2 = inst.knearest_batch(pts, 5)
        _agree(got2, want2, 5, dtype, "re-posed")
        assert got2[0].tobytes() != got[0].tobytes() or got2[2].tobytes() != got[2].tobytes()
        fresh_member = _gpu_trees(eng, ctx, [new])[0]
        with eng.Instances([fresh_member], [0] * 5, x2, ctx) as fresh:
            _agree(fresh.knearest_batch(pts, 5), want2, 5, dtype, "re-posed against a fresh set")


# ---- 7. the refusals of the raw C ABI, in the header's order ---------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype = np.float32
    k = 5
    c, pts_all, _ = cluster(orc, dtype, 37)
    rows = cluster_rows(orc, dtype, 37, k)[0][:64]
    trees = _gpu_trees(eng, ctx, c["trees"])
    pts = np.ascontiguousarray(pts_all[:64])
    pts64 = pts.astype(np.float64)
    f32, f64 = lib.bvhgpu_instances_knearest_f32, lib.bvhgpu_instances_knearest_f64
    STALE, UNCOMMITTED, FOLDED = "instances are stale: call bvhgpu_instances_update", "instances are not committed", "split without SAH winner"
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
    far, far_tris = far_scene(dtype)[:2]
    far_member = eng.Bvh.from_aabbs(far, ctx).flatten()
    far_member.set_triangles(far_tris)
    blob = np.zeros(far_member.scene_nbytes(), np.uint8)
    far_member.scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(far_tris)
    eye = np.eye(3, 4, dtype=dtype)[None]
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances([member], [0] * 37, c["x"], ctx) as stale, \
            eng.Instances(trees, c["tree_of"], c["x"], ctx) as broken, eng.Instances([imp], [0], eye, ctx) as folded:
        member.rebuild(c["trees"][1][0][:100], flatten=True)             # a member without triangles, of another generation
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        s = inst._s
        P, I, S, D = ptr(pts), ptr(oi), ptr(os_), ptr(od)
        # each rule alone
        assert f32(None, P, 64, HOST, k, I, S, D) == INVALID_ARG
        refused(INVALID_ARG, INVALID_ARG, "")
        for bad_k in (0, _lib.INSTANCES_KNN_MAX_K + 1, 0xFFFFFFFF):
            refused(f32(s, P, 64, HOST, bad_k, I, S, D), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KNN_MAX_K")
        refused(f32(s, None, 64, HOST, k, I, S, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, None, S, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, I, None, D), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, HOST, k, I, S, None), INVALID_ARG, "NULL argument")
        refused(f32(s, P, 64, 7, k, I, S, D), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE")
        refused(f64(s, ptr(pts64), 64, HOST, k, I, S, ptr(od64)), DTYPE_MISMATCH, "instance set dtype differs from point dtype")
        refused(f32(broken._s, P, 64, HOST, k, I, S, D), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, P, 64, HOST, k, I, S, D), INVALID_ARG, STALE)
        refused(f32(folded._s, P, 64, HOST, k, I, S, D), INVALID_ARG, FOLDED)
        refused(f32(s, P, 1 << 26, HOST, 64, I, S, D), OVERFLOW, "too many results (points x k)")           # n * k = 2^32
        refused(f32(s, P, 0xFFFFFFFF, HOST, 1, I, S, D), OVERFLOW, "too many results (points x k)")
        # the order: an earlier rule wins over a later one
        refused(f64(stale._s, None, 0xFFFFFFFF, 7, 0, I, S, D), INVALID_ARG, "k must be")
        refused(f64(stale._s, None, 0xFFFFFFFF, 7, k, I, S, D), INVALID_ARG, "NULL argument")
        refused(f64(stale._s, P, 0xFFFFFFFF, 7, k, I, S, D), INVALID_ARG, "mem must be")
        refused(f64(stale._s, P, 0xFFFFFFFF, HOST, k, I, S, D), DTYPE_MISMATCH, "dtype")
        refused(f32(broken._s, P, 0xFFFFFFFF, HOST, k, I, S, D), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, P, 0xFFFFFFFF, HOST, k, I, S, D), INVALID_ARG, STALE)
        refused(f32(folded._s, P, 0xFFFFFFFF, HOST, k, I, S, D), INVALID_ARG, FOLDED)
        # the stale check is bvhgpu_instances_trace_*'s: the same words from both
        rays = np.ascontiguousarray(c["rays"][:64])
        v, ti, tsh = np.zeros((64, 3), dtype), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
        assert lib.bvhgpu_instances_trace_f32(stale._s, ptr(rays), None, 64, HOST, 0, ptr(v), ptr(ti), ptr(tsh)) == INVALID_ARG
        trace_words = err()
        assert f32(stale._s, P, 64, HOST, k, I, S, D) == INVALID_ARG and err() == trace_words
        # NULL buffers are fine where there is nothing to read or write
        assert f32(s, None, 0, HOST, k, None, None, None) == OK
        refused(OK, OK, "")
        # a later valid call still answers, on the set that refused and into the buffers that stayed untouched
        gi, gs, gd = np.zeros((64, k), np.uint32), np.zeros((64, k), np.uint32), np.zeros((64, k), dtype)
        assert f32(s, P, 64, HOST, k, ptr(gi), ptr(gs), ptr(gd)) == OK
        _agree((gi, gs, gd), rows, k, dtype, "after the refusals")
        _agree(inst.knearest_batch(pts, k), rows, k, dtype, "after the refusals, through the binding")
        # the binding refuses a k out of range by the engine's status
        for bad_k in (0, 65, -1):
            with pytest.raises(_lib.BvhGpuError) as e:
                inst.knearest_batch(pts, bad_k)
            assert e.value.status == INVALID_ARG and "k must be" in str(e.value)
