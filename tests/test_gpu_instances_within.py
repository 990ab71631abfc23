"""Radius search over instanced scenes on the GPU (bvhgpu_instances_within_*): every row byte for byte against
tests/instances_within_ref.py on the scenes tests/test_instances_within_cpu.py shows to equal a brute force and to be worth running — the
cluster scenes sorted, in list order and count-only, with a scalar and with per-point limits, HOST and HBM; the line of instances, whose
rows reach the lane, LDS and global-memory tiers of the sort; an identity instance against the member's own within_batch, GPU against GPU;
edge limits and point counts; members and top levels of every served kind; tree generations, the result object's kinds and the refusals
of the raw C ABI.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as fz
import instances_ref as ir
import instances_within_ref as iwr
from test_gpu_any_hit import _rb
from test_instances_cpu import SIZES, member_trees, transforms
from test_instances_within_cpu import N_POINTS, cluster_rows, line_case
from test_within_cpu import far_scene

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


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
    """(offsets, instance, shape, dist) as numpy, offsets and indices as uint32 (points in HBM come back as torch tensors)"""
    off, inst, shape, dist = got["offsets"], got["instance"], got["shape"], got["dist"]
    if not isinstance(off, np.ndarray):
        import torch
        assert off.dtype == torch.int64 and inst.dtype == torch.int32 and shape.dtype == torch.int32 and dist.is_cuda and off.is_cuda
        off = off.cpu().numpy().astype(np.uint32)
        inst, shape, dist = inst.cpu().numpy().view(np.uint32), shape.cpu().numpy().view(np.uint32), dist.cpu().numpy()
    return off, inst, shape, dist


def _agree(got, want, label):
    off, inst, shape, dist = _host(got)
    assert off.dtype == np.uint32 and inst.dtype == np.uint32 and shape.dtype == np.uint32 and dist.dtype == want[3].dtype, label
    assert dist.shape == want[3].shape, (label, dist.shape, want[3].shape)
    assert off.tobytes() == want[0].tobytes(), label
    assert inst.tobytes() == want[1].tobytes(), label
    assert shape.tobytes() == want[2].tobytes(), label
    assert dist.tobytes() == want[3].tobytes(), label


def _counts_agree(got, want_off, label):
    assert set(got) == {"offsets"}, label
    off = got["offsets"]
    off = off if isinstance(off, np.ndarray) else off.cpu().numpy().astype(np.uint32)
    assert off.tobytes() == want_off.tobytes(), label


def _both_orders(inst, pts, lim, rows, dtype, label, device=True):
    """sorted, list order and count-only from HOST input (and from HBM) against the reference rows"""
    for sort in (True, False):
        want = iwr.csr(rows, dtype, sort)
        _agree(inst.within_batch(pts, lim, sort=sort), want, (label, sort, "host"))
        if device:
            _agree(inst.within_batch(_dev(pts), lim if np.ndim(lim) == 0 else _dev(lim), sort=sort), want, (label, sort, "device"))
    _counts_agree(inst.within_batch(pts, lim, count_only=True), want[0], (label, "count"))


# ---- 1. the cluster scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene(eng, orc, ctx, dtype, n):
    """n = 1: the top level is one leaf entry; n = 2, 37: member C has one triangle"""
    c, pts, m, rows, _ = cluster_rows(orc, dtype, n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        _both_orders(inst, pts, m, rows, dtype, n)
        total = sum(len(r) for r in rows)
        assert total >= 1000
        _counts_agree(inst.within_batch(_dev(pts), _dev(m), sort=False, count_only=True), iwr.csr(rows, dtype)[0], (n, "count, device"))
        assert inst._hits.walk_kernel().startswith("bvhgpu::k_instances_within_count<")
        assert inst._hits.info()["total"] == inst._hits.info()["hits"] == total
        inst.within_batch(pts, m)
        assert inst._hits.walk_kernel().startswith("bvhgpu::k_instances_within_fill<") and inst._hits.wait()["total"] == total
        # a scalar limit is the same limit for every point
        sub = np.ascontiguousarray(pts[:150])
        _both_orders(inst, sub, 2.5, iwr.rows(c["scene"], sub, 2.5), dtype, (n, "scalar"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_uploaded_flat_bvh_as_a_member(eng, orc, ctx, dtype):
    """member B as the oracle's FlatNode array uploaded (the UNFOLDED rule) beside the built A and C (folded), in one launch"""
    c, pts, m, rows, _ = cluster_rows(orc, dtype, 37)
    sc = c["scene"]
    built = _gpu_trees(eng, ctx, c["trees"])
    up = eng.FlatBvh.from_flat_nodes(sc.flats[1], c["trees"][1][0], ctx)
    up.set_triangles(c["trees"][1][1])
    with eng.Instances([built[0], up, built[2]], c["tree_of"], c["x"], ctx) as inst:
        _both_orders(inst, pts, m, rows, dtype, "uploaded", device=False)


# ---- 2. the line of instances: every tier --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene_reaches_every_tier(eng, orc, ctx, dtype):
    s = line_case(orc, dtype)
    lane_max, lds_max = s["lane_max"], s["lds_max"]
    trees = _gpu_trees(eng, ctx, s["trees"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        got = inst.within_batch(s["points"], s["limits"])
        lens = np.diff(got["offsets"].astype(np.int64))
        assert ((lens >= 2) & (lens <= lane_max)).any() and ((lens > lane_max) & (lens <= lds_max)).any() and (lens > lds_max).any()
        for L in (0, 1, lane_max - 1, lane_max, lane_max + 1, lds_max - 1, lds_max, lds_max + 1, 4224):
            assert (lens == L).any(), L
        _agree(got, iwr.csr(s["rows"], dtype, True), "sorted")
        for j in range(len(lens)):
            assert (np.diff(got["dist"][got["offsets"][j]:got["offsets"][j + 1]]) >= 0).all()
        _both_orders(inst, s["points"], s["limits"], s["rows"], dtype, "line")


# ---- 3. an anchor that does not pass through the new reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_members_own_within(eng, orc, ctx, dtype):
    B = _gpu_trees(eng, ctx, [member_trees(orc, dtype)[1]])[0]
    rng = np.random.default_rng(77)
    pts = rng.uniform(-5, 5, size=(400, 3)).astype(dtype)
    m = rng.uniform(0.1, 4.0, size=400).astype(dtype)
    off, shape, dist = B.within_batch(pts, m, triangles=True, sort=False)
    assert (np.diff(off.astype(np.int64)) > 0).sum() >= 200
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        got = inst.within_batch(pts, m, sort=False)
        assert got["offsets"].tobytes() == off.tobytes() and got["shape"].tobytes() == shape.tobytes() and got["dist"].tobytes() == dist.tobytes()
        assert (got["instance"] == 0).all() and len(got["instance"]) == len(shape)
        off, shape, dist = B.within_batch(pts, m, triangles=True)
        got = inst.within_batch(pts, m)
        assert got["offsets"].tobytes() == off.tobytes() and got["shape"].tobytes() == shape.tobytes() and got["dist"].tobytes() == dist.tobytes()


# ---- 4. limits, point counts, empty sets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_limits(eng, orc, ctx, dtype):
    """0 and -0.0 keep what is at distance 0 (the point x = 5 lies on a shape of instance 0 and of its coincident copy), a negative and a NaN
    limit keep nothing, +inf keeps every pair; NaN and infinite points"""
    s = line_case(orc, dtype)
    lim = np.array([0.0, -0.0, -1.0, np.nan, np.inf, 0.5, -np.inf, 1.0, 1.0, np.inf, np.inf], dtype=dtype)
    pts = np.zeros((len(lim), 3), dtype=dtype)
    pts[:, 0] = 5
    pts[7] = [np.nan, 0, 0]
    pts[8] = [np.inf, 0, 0]
    pts[9] = [np.nan, np.nan, np.nan]
    pts[10] = [-np.inf, 0, 0]
    rows = iwr.rows(s["scene"], pts, lim)
    assert [len(r) for r in rows][:7] == [2, 2, 0, 0, 4224, 2, 0]
    trees = _gpu_trees(eng, ctx, s["trees"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        _both_orders(inst, pts, lim, rows, dtype, "edge limits")
        got = inst.within_batch(pts[:2], lim[:2])
        assert got["dist"].tolist() == [0.0] * 4 and sorted(got["instance"].tolist()) == [0, 0, 64, 64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_point_counts(eng, orc, ctx, dtype):
    c, pts, m, rows, _ = cluster_rows(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (0, 1, 255, 256, 257, 1025):
            idx = np.arange(k) % N_POINTS
            sub_rows = [rows[j] for j in idx]
            for sort in (True, False):
                _agree(inst.within_batch(np.ascontiguousarray(pts[idx]), np.ascontiguousarray(m[idx]), sort=sort), iwr.csr(sub_rows, dtype, sort), (k, sort))
        got = inst.within_batch(pts[:0], m[:0])
        assert got["offsets"].tolist() == [0] and got["dist"].shape == (0,) and got["instance"].shape == (0,) and got["shape"].shape == (0,)
        assert got["dist"].dtype == dtype
        got = inst.within_batch(_dev(pts[:0]), 1.0, sort=False)
        assert got["offsets"].cpu().tolist() == [0] and tuple(got["dist"].shape) == (0,)
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for kw in (dict(), dict(sort=False), dict(count_only=True)):
            got = empty.within_batch(pts, m, **kw)
            assert got["offsets"].shape == (N_POINTS + 1,) and not got["offsets"].any()
            assert kw.get("count_only") or (len(got["instance"]) == 0 and got["dist"].shape == (0,))


# ---- 5. arrays with empty child bounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_world_boxes_give_a_mirrored_top_level(eng, orc, ctx, dtype):
    """tests/test_gpu_instances_region.py's set of three instances of the far scene, two of whose world boxes coincide (a translation of 1
    vanishes at 1e19): the top level's split has no SAH winner, its child bounds are empty (distance 0 to every point) and it is walked
    over its unfolded mirror, and so is the member; rows up to 1 500 entries, ties between the coincident instances"""
    far, tris, pts, m = far_scene(dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (3, 1, 1))
    x[1, :, 3] = [1, 2, 3]
    x[2, 0, 0] = 0.5
    sc = ir.Scene([(far, tris)], [0, 0, 0], x, dtype)
    assert fz.has_empty_child_bounds(sc.top) and sc.w[0].tobytes() == sc.w[1].tobytes() != sc.w[2].tobytes()
    wt = iwr.world_triangles(sc)
    pts = np.ascontiguousarray(np.concatenate([pts[:300], wt[0][:100, 0], wt[2][100:200, 1]]))       # random points and points on world vertices
    m = np.ascontiguousarray(m[:len(pts)])
    rows = iwr.rows(sc, pts, m)
    lens = np.array([len(r) for r in rows])
    assert (lens > 0).sum() >= 100 and (lens == 0).sum() >= 100 and lens.max() == 1500
    assert sum(1 for r in rows if len(set(i for _, i, _ in r)) >= 2) >= 100
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    with eng.Instances([member], [0, 0, 0], x, ctx) as inst:
        _both_orders(inst, pts, m, rows, dtype, "coincident world boxes")


@pytest.mark.parametrize("dtype", DTYPES)
def test_member_with_empty_child_bounds_built_and_imported(eng, orc, ctx, dtype):
    """boxes so far apart that no bucket wins a split: the built member is walked over its unfolded mirror, whose empty navigator boxes
    are entered whatever the point; the same member after scene export / import carries the folded array only and is refused"""
    far, tris, pts, m = far_scene(dtype)
    x = np.eye(3, 4, dtype=dtype)[None].copy()
    x[0, 0, 0], x[0, 1, 1] = 0.5, -2.0
    sc = ir.Scene([(far, tris)], [0], x, dtype)
    assert fz.has_empty_child_bounds(sc.flats[0])
    wt = iwr.world_triangles(sc)[0]
    pts = np.ascontiguousarray(np.concatenate([pts[:300], wt[:100, 0], wt[100:200, 1]]))       # random points and points on world vertices
    m = np.ascontiguousarray(m[:len(pts)])
    rows = iwr.rows(sc, pts, m)
    lens = np.array([len(r) for r in rows])
    assert (lens > 0).sum() >= 100 and (lens == 0).sum() >= 100
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    with eng.Instances([member], [0], x, ctx) as inst:
        _both_orders(inst, pts, m, rows, dtype, "empty child bounds", device=False)
    blob = np.zeros(member.scene_nbytes(), np.uint8)
    member.scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(tris)
    with eng.Instances([imp], [0], x, ctx) as inst:
        for kw in (dict(), dict(sort=False), dict(count_only=True)):
            with pytest.raises(eng.BvhGpuError) as e:
                inst.within_batch(pts, m, **kw)
            assert e.value.status == 1 and "split without SAH winner" in str(e.value)


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
    pts, m = iwr.cluster_points(5, dtype, 300)

    def ref(tr, xf, sort=True):
        return iwr.within(ir.Scene([tr], [0] * 5, xf, dtype), pts, m, sort)

    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.within_batch(pts, m), ref(trees[0], x), "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        for kw in (dict(), dict(sort=False), dict(count_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.within_batch(pts, m, **kw)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x)
        # the first reader of the new generation is this entry
        got = inst.within_batch(pts, m)
        want = ref((b_aabbs[:100], b_tris[:100]), x)
        assert int(want[0][-1]) >= 100
        _agree(got, want, "after")
        fresh_member = _gpu_trees(eng, ctx, [(b_aabbs[:100], b_tris[:100])])[0]
        with eng.Instances([fresh_member], [0] * 5, x, ctx) as fresh:
            _agree(fresh.within_batch(pts, m), _host(got), "a fresh set")
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        for kw in (dict(), dict(count_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.within_batch(pts, m, **kw)
            assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        # a re-pose, against the reference and against a fresh set
        x2 = transforms(5, dtype, 999)
        inst.update(x2)
        want2 = ref((b_aabbs[:100], b_tris[:100]), x2)
        assert want2[1].tobytes() != want[1].tobytes()
        got2 = inst.within_batch(pts, m)
        _agree(got2, want2, "re-posed")
        _agree(inst.within_batch(pts, m, sort=False), ref((b_aabbs[:100], b_tris[:100]), x2, False), "re-posed, list order")
        with eng.Instances([fresh_member], [0] * 5, x2, ctx) as fresh:
            _agree(fresh.within_batch(pts, m), _host(got2), "re-posed against a fresh set")


# ---- 7. the result object ------------------------------------------------------------------------------------------------------------------
def test_one_result_object_through_every_rows_family(eng, orc, ctx):
    """one bvhgpu_hits used in turn by bvhgpu_within_*, bvhgpu_instances_allhits_*, this entry and back: each result is right and every wrong
    fetch is refused, by status and by message"""
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    c, pts_all, m_all, rows, _ = cluster_rows(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    tree = trees[1]
    aabbs, tris = c["trees"][1]
    pts, lim = np.ascontiguousarray(pts_all[:300]), np.ascontiguousarray(m_all[:300])
    want = iwr.csr(rows[:300], dtype)
    total = int(want[0][-1])
    assert total >= 50
    big = 200000
    so, si, ss, sv = (np.full(600, 0xABABABAB, np.uint32), np.full(big, 0xABABABAB, np.uint32), np.full(big, 0xABABABAB, np.uint32),
                      np.full((big, 3), 7.0, dtype))
    mine = lib.bvhgpu_hits_fetch_instances_within
    RIGHT = "use bvhgpu_hits_fetch_instances_within"

    def untouched():
        return (so == 0xABABABAB).all() and (si == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (sv == 7.0).all()

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def this_entry(h, flags=0):
        assert lib.bvhgpu_instances_within_f32(inst._s, ptr(pts), ptr(lim), 300, HOST, flags, C.byref(h)) == OK
        nr, tot, st = C.c_size_t(), C.c_uint64(), _lib.TraverseStats()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), C.byref(st)) == OK and (nr.value, tot.value, st.hits) == (300, total, total)
        assert lib.bvhgpu_hits_wait(h) == OK
        wrong = {
            "fetch": lambda: lib.bvhgpu_hits_fetch(h, ptr(so), ptr(ss), None, HOST),
            "triangles": lambda: lib.bvhgpu_hits_fetch_triangles(h, ptr(sv), HOST),
            "closest": lambda: lib.bvhgpu_hits_fetch_closest(h, ptr(sv), ptr(ss), HOST),
            "any": lambda: lib.bvhgpu_hits_fetch_any(h, ptr(sv), ptr(ss), HOST),
            "box": lambda: lib.bvhgpu_hits_fetch_box(h, ptr(sv), ptr(ss), HOST),
            "sphere": lambda: lib.bvhgpu_hits_fetch_sphere(h, ptr(sv), ptr(ss), HOST),
            "allhits": lambda: lib.bvhgpu_hits_fetch_allhits(h, ptr(so), ptr(ss), ptr(sv), HOST),
            "within": lambda: lib.bvhgpu_hits_fetch_within(h, ptr(so), ptr(ss), ptr(sv), HOST),
            "region": lambda: lib.bvhgpu_hits_fetch_region(h, ptr(so), ptr(ss), None, HOST),
            "instances_region": lambda: lib.bvhgpu_hits_fetch_instances_region(h, ptr(so), ptr(si), ptr(ss), None, HOST),
            "instances_allhits": lambda: lib.bvhgpu_hits_fetch_instances_allhits(h, ptr(so), ptr(si), ptr(ss), ptr(sv), HOST),
            "device": lambda: lib.bvhgpu_hits_device(h, None, None, None),
        }
        for name, f in wrong.items():
            assert f() == INVALID_ARG and RIGHT in err(), (name, err())
            assert untouched(), name
        if flags & 2:
            assert mine(h, ptr(so), ptr(si), None, None, HOST) == INVALID_ARG and "COUNT_ONLY" in err()
            assert mine(h, ptr(so), None, ptr(ss), None, HOST) == INVALID_ARG and "COUNT_ONLY" in err()
            assert mine(h, ptr(so), None, None, ptr(sv), HOST) == INVALID_ARG and "COUNT_ONLY" in err()
            assert untouched()
            off = np.zeros(301, np.uint32)
            assert mine(h, ptr(off), None, None, None, HOST) == OK and off.tobytes() == want[0].tobytes()
            return
        assert mine(h, ptr(so), ptr(si), ptr(ss), ptr(sv), 9) == INVALID_ARG and "mem must be" in err() and untouched()
        off, gi, gs, gd = np.zeros(301, np.uint32), np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(total, dtype)
        assert mine(h, ptr(off), ptr(gi), ptr(gs), ptr(gd), HOST) == OK
        assert off.tobytes() == want[0].tobytes() and gi.tobytes() == want[1].tobytes() and gs.tobytes() == want[2].tobytes()
        assert gd.tobytes() == want[3].tobytes()
        assert mine(h, None, None, None, None, HOST) == OK                     # each pointer may be NULL

    def other_kind(h, text):
        assert mine(h, ptr(so), ptr(si), ptr(ss), ptr(sv), HOST) == INVALID_ARG and text in err(), err()
        assert untouched()

    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        h = C.c_void_p()
        # bvhgpu_within_*
        wp = np.ascontiguousarray(((aabbs[:50, :3] + aabbs[:50, 3:]) / 2).astype(dtype))
        wl = np.full(50, 0.75, dtype)
        assert lib.bvhgpu_within_f32(tree._t, ptr(wp), ptr(wl), 50, HOST, 1, 0, C.byref(h)) == OK
        keep = h.value
        other_kind(h, "no bvhgpu_instances_within_")
        w_got = tree.within_batch(wp, wl, triangles=True)       # (the tree's own result object; tests/test_gpu_within.py holds it to the oracle)
        off, gs, gv = np.zeros(51, np.uint32), np.zeros(len(w_got[1]), np.uint32), np.zeros(len(w_got[1]), dtype)
        assert lib.bvhgpu_hits_fetch_within(h, ptr(off), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == w_got[0].tobytes() and gs.tobytes() == w_got[1].tobytes() and gv.tobytes() == w_got[2].tobytes()
        assert int(off[-1]) >= 50
        # bvhgpu_instances_allhits_*
        rays = np.ascontiguousarray(c["rays"][150:450])
        assert lib.bvhgpu_instances_allhits_f32(inst._s, ptr(rays), None, 300, HOST, 0, C.byref(h)) == OK and h.value == keep
        other_kind(h, "no bvhgpu_instances_within_")
        a_got = inst.allhits_batch(_rb(eng, rays))               # (the set's own result object; tests/test_gpu_instances_allhits.py holds it to the reference)
        n_a = len(a_got["shape"])
        assert n_a >= 50
        off, gi, gs, gv = np.zeros(301, np.uint32), np.zeros(n_a, np.uint32), np.zeros(n_a, np.uint32), np.zeros((n_a, 3), dtype)
        assert lib.bvhgpu_hits_fetch_instances_allhits(h, ptr(off), ptr(gi), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == a_got["offsets"].tobytes() and gi.tobytes() == a_got["instance"].tobytes() and gv.tobytes() == a_got["vals"].tobytes()
        # this entry
        this_entry(h)
        assert h.value == keep
        # and back: bvhgpu_within_* once more, then this entry count-only and full
        assert lib.bvhgpu_within_f32(tree._t, ptr(wp), ptr(wl), 50, HOST, 1, 0, C.byref(h)) == OK and h.value == keep
        other_kind(h, "no bvhgpu_instances_within_")
        off, gs, gv = np.zeros(51, np.uint32), np.zeros(len(w_got[1]), np.uint32), np.zeros(len(w_got[1]), dtype)
        assert lib.bvhgpu_hits_fetch_within(h, ptr(off), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == w_got[0].tobytes() and gs.tobytes() == w_got[1].tobytes() and gv.tobytes() == w_got[2].tobytes()
        this_entry(h, 2)
        this_entry(h, 0)
        # a closest-hit batch refuses this fetch too
        assert lib.bvhgpu_traverse_f32(tree._t, ptr(rays), 300, HOST, _lib.TRAVERSE_CLOSEST, C.byref(h)) == OK
        other_kind(h, "no bvhgpu_instances_within_")
        lib.bvhgpu_hits_destroy(h)


# ---- 8. the refusals of the raw C ABI, in the header's order ---------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    import torch
    from bvh_amd import _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype = np.float32
    c, pts_all, m_all, rows, _ = cluster_rows(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    pts, lim = np.ascontiguousarray(pts_all[:64]), np.ascontiguousarray(m_all[:64])
    pts64, lim64 = pts.astype(np.float64), lim.astype(np.float64)
    want = iwr.csr(rows[:64], dtype)
    total = int(want[0][-1])
    assert total >= 50
    f32, f64 = lib.bvhgpu_instances_within_f32, lib.bvhgpu_instances_within_f64
    STALE, UNCOMMITTED, FOLDED = "instances are stale: call bvhgpu_instances_update", "instances are not committed", "split without SAH winner"

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text, h, keep=None):
        assert rc == status and text in err(), (rc, err())
        assert h.value == keep                                # *hits stays as it was

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
        member.rebuild(c["trees"][1][0][:100], flatten=True)
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        s = inst._s
        h = C.c_void_p()
        # 1. a NULL set or a NULL hits
        assert f32(None, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        assert f32(s, ptr(pts), ptr(lim), 64, HOST, 0, None) == INVALID_ARG and "hits is NULL" in err()
        # 2. a result object that still holds an asynchronous batch: it wins over everything behind it
        rays = np.ascontiguousarray(c["rays"][150:214])
        rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        ha = C.c_void_p()
        assert lib.bvhgpu_traverse_async_f32(trees[1]._t, ptr(rays_dev.data_ptr()), 64, DEVICE, 0, C.byref(ha)) == OK
        held = ha.value
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, 8, C.byref(ha)), INVALID_ARG, "still holds an asynchronous batch", ha, held)
        assert lib.bvhgpu_hits_wait(ha) == OK
        lib.bvhgpu_hits_destroy(ha)
        # 3. .. 11., each alone
        refused(f32(s, None, ptr(lim), 64, HOST, 0, C.byref(h)), INVALID_ARG, "points is NULL", h)
        refused(f32(s, ptr(pts), None, 64, HOST, 0, C.byref(h)), INVALID_ARG, "max_dist is NULL", h)
        refused(f32(s, ptr(pts), ptr(lim), 64, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE", h)
        refused(f64(s, ptr(pts64), ptr(lim64), 64, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "instance set dtype differs from point dtype", h)
        for flags in (4, 8, 1 << 10, 1 << 24, 1 << 31, 3 | 16):
            refused(f32(s, ptr(pts), ptr(lim), 64, HOST, flags, C.byref(h)), INVALID_ARG, "instance within flags", h)
        refused(f32(broken._s, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)), INVALID_ARG, UNCOMMITTED, h)
        refused(f32(stale._s, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)), INVALID_ARG, STALE, h)
        for flags in (0, 1, 2):
            refused(f32(folded._s, ptr(pts), ptr(lim), 64, HOST, flags, C.byref(h)), INVALID_ARG, FOLDED, h)
        refused(f32(s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 0, C.byref(h)), OVERFLOW, "2^32-2 points", h)
        # the order: an earlier rule wins over a later one
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "points is NULL", h)
        refused(f64(stale._s, ptr(pts), None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "max_dist is NULL", h)
        refused(f64(stale._s, ptr(pts), ptr(lim), 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "mem must be", h)
        refused(f64(stale._s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 8, C.byref(h)), DTYPE_MISMATCH, "dtype", h)
        refused(f32(stale._s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 8, C.byref(h)), INVALID_ARG, "instance within flags", h)
        refused(f32(broken._s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, UNCOMMITTED, h)
        refused(f32(stale._s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, STALE, h)
        refused(f32(folded._s, ptr(pts), ptr(lim), 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, FOLDED, h)
        # the stale check is bvhgpu_instances_trace_*'s: the same words from both
        v, i, sh = np.zeros((64, 3), dtype), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
        assert lib.bvhgpu_instances_trace_f32(stale._s, ptr(rays), None, 64, HOST, 0, ptr(v), ptr(i), ptr(sh)) == INVALID_ARG
        trace_words = err()
        assert f32(stale._s, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)) == INVALID_ARG and err() == trace_words
        # NULL points and limits are fine where there is nothing to read
        assert f32(s, None, None, 0, HOST, 0, C.byref(h)) == OK and h.value
        keep = h.value
        so = np.full(65, 0xABABABAB, np.uint32)
        assert lib.bvhgpu_hits_fetch_instances_within(h, ptr(so), None, None, None, HOST) == OK and so[0] == 0 and (so[1:] == 0xABABABAB).all()
        # a refused batch leaves the result object as it was
        assert f32(s, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)) == OK and h.value == keep
        refused(f32(s, ptr(pts), ptr(lim), 64, 7, 0, C.byref(h)), INVALID_ARG, "mem must be", h, keep)
        refused(f32(stale._s, ptr(pts), ptr(lim), 64, HOST, 0, C.byref(h)), INVALID_ARG, STALE, h, keep)
        refused(f32(s, ptr(pts), ptr(lim), 64, HOST, 4, C.byref(h)), INVALID_ARG, "instance within flags", h, keep)
        nr, tot = C.c_size_t(), C.c_uint64()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (64, total)
        off, gi, gs, gd = np.zeros(65, np.uint32), np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(total, dtype)
        assert lib.bvhgpu_hits_fetch_instances_within(h, ptr(off), ptr(gi), ptr(gs), ptr(gd), HOST) == OK
        assert off.tobytes() == want[0].tobytes() and gi.tobytes() == want[1].tobytes() and gs.tobytes() == want[2].tobytes()
        assert gd.tobytes() == want[3].tobytes()
        assert lib.bvhgpu_hits_fetch_instances_within(None, ptr(off), None, None, None, HOST) == INVALID_ARG
        lib.bvhgpu_hits_destroy(h)
