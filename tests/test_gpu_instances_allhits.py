"""All-hits over instanced scenes on the GPU (bvhgpu_instances_allhits_*): every row byte for byte against tests/instances_allhits_ref.py on
the scenes tests/test_instances_allhits_cpu.py shows to be worth running — the cluster scene in both orders, free and cut, HOST and HBM; the
stack scene, whose rows reach the lane, LDS and global-memory tiers of the sort; anchors that do not pass through the new reference (the
row heads against closest_hits / any_hits / occluded, an identity instance against the single-tree all-hits); edge sizes, tree
generations, the result object's kinds and the refusals of the raw C ABI.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_ref as ir
from test_gpu_any_hit import _rb
from test_instances_allhits_cpu import N_STACK_RAYS, _heads, cluster_rows, stack_case
from test_instances_cpu import N_RAYS, SIZES, case, cluster_rays, member_trees, transforms

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
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


def _dev_rays(eng, rays):
    import torch
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    return eng.RayBatch.from_device(dev, len(rays), dt)


def _gpu_trees(eng, ctx, trees):
    out = []
    for aabbs, tris in trees:
        flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris)
        out.append(flat)
    return out


def _host(got):
    """(offsets, instance, shape, vals) as numpy, offsets and indices as uint32 (rays in HBM come back as torch tensors)"""
    off, inst, shape, vals = got["offsets"], got["instance"], got["shape"], got["vals"]
    if not isinstance(off, np.ndarray):
        import torch
        assert off.dtype == torch.int64 and inst.dtype == torch.int32 and shape.dtype == torch.int32 and vals.is_cuda and off.is_cuda
        off = off.cpu().numpy().astype(np.uint32)
        inst, shape, vals = inst.cpu().numpy().view(np.uint32), shape.cpu().numpy().view(np.uint32), vals.cpu().numpy()
    return off, inst, shape, vals


def _agree(got, want, label):
    off, inst, shape, vals = _host(got)
    assert off.dtype == np.uint32 and inst.dtype == np.uint32 and shape.dtype == np.uint32 and vals.dtype == want[3].dtype, label
    assert vals.shape == want[3].shape, label
    assert off.tobytes() == want[0].tobytes(), label
    assert inst.tobytes() == want[1].tobytes(), label
    assert shape.tobytes() == want[2].tobytes(), label
    assert vals.tobytes() == want[3].tobytes(), label


def _counts_agree(got, want_off, label):
    assert set(got) == {"offsets"}, label
    off = got["offsets"]
    off = off if isinstance(off, np.ndarray) else off.cpu().numpy().astype(np.uint32)
    assert off.tobytes() == want_off.tobytes(), label


# ---- 1. the cluster scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene(eng, orc, ctx, dtype, n):
    import torch
    c, rows = cluster_rows(orc, dtype, n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        rb, rd = _rb(eng, c["rays"]), _dev_rays(eng, c["rays"])
        for cut in (False, True):
            tm = c["tmax"] if cut else None
            td = torch.from_numpy(c["tmax"]).cuda() if cut else None
            for sort in (True, False):
                want = rows[(cut, sort)]
                _agree(inst.allhits_batch(rb, tm, sort=sort), want, (n, cut, sort, "host"))
                _agree(inst.allhits_batch(rd, td, sort=sort), want, (n, cut, sort, "device"))
                _counts_agree(inst.allhits_batch(rb, tm, sort=sort, count_only=True), want[0], (n, cut, sort, "count, host"))
            _counts_agree(inst.allhits_batch(rd, td, count_only=True), rows[(cut, True)][0], (n, cut, "count, device"))
            assert inst._hits.walk_kernel().startswith("bvhgpu::k_instances_allhits_count<")
            assert inst._hits.info()["total"] == inst._hits.info()["hits"] == int(rows[(cut, True)][0][-1])
        inst.allhits_batch(rb)
        assert inst._hits.walk_kernel().startswith("bvhgpu::k_instances_allhits_fill<") and inst._hits.wait()["total"] == int(rows[(False, True)][0][-1])


# ---- 2. the stack scene: every tier --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stack_scene_reaches_every_tier(eng, orc, ctx, dtype):
    s = stack_case(orc, dtype)
    lane_max, lds_max = s["lane_max"], s["lds_max"]
    trees = _gpu_trees(eng, ctx, s["trees"])
    rb = _rb(eng, s["rays"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        got = inst.allhits_batch(rb, s["tmax"])
        lens = np.diff(got["offsets"].astype(np.int64))
        assert ((lens >= 2) & (lens <= lane_max)).any() and ((lens > lane_max) & (lens <= lds_max)).any() and (lens > lds_max).any()
        for L in (0, 1, lane_max - 1, lane_max, lane_max + 1, lds_max - 1, lds_max, lds_max + 1):
            assert (lens == L).any(), L
        _agree(got, s["cut"], "cut, sorted")
        _agree(inst.allhits_batch(rb, s["tmax"], sort=False), s["cut_list"], "cut, list order")
        got = inst.allhits_batch(rb)
        assert (np.diff(got["offsets"].astype(np.int64))[:N_STACK_RAYS] > lds_max).sum() >= 57
        _agree(got, s["uncut"], "uncut, sorted")
        _agree(inst.allhits_batch(rb, sort=False), s["uncut_list"], "uncut, list order")
        _counts_agree(inst.allhits_batch(rb, s["tmax"], count_only=True), s["cut"][0], "count")


# ---- 3. anchors that do not pass through the new reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_heads_are_the_trace_entries_answers(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for tm in (None, c["tmax"]):
            for sort, call in ((True, inst.closest_hits), (False, inst.any_hits)):
                got = _host(inst.allhits_batch(rb, tm, sort=sort))
                heads, full = _heads(got, N_RAYS, dtype), np.diff(got[0].astype(np.int64)) > 0
                vals, ii, ss = call(rb, tm)
                assert heads[0].tobytes() == vals.tobytes() and heads[1].tobytes() == ii.tobytes() and heads[2].tobytes() == ss.tobytes(), sort
                assert np.array_equal(full, inst.occluded(rb, tm))
            assert 20 <= full.sum() <= N_RAYS - 20


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree_allhits(eng, orc, ctx, dtype):
    trees = member_trees(orc, dtype)
    B = _gpu_trees(eng, ctx, [trees[1]])[0]
    rays = cluster_rays(orc, 1500, dtype, 21)
    rays["o"] *= dtype(0.2)
    rb = _rb(eng, rays)
    isect, shape = B.closest_hits(rb)[:2]
    assert (shape != NONE).sum() >= 100
    tmax = (np.where(np.isfinite(isect[:, 0]), isect[:, 0], 50) * np.random.default_rng(5).uniform(0.3, 1.7, len(rays))).astype(dtype)
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        for tm in (None, tmax):
            for sort in (True, False):
                off, sh, vals = B.allhits_batch(rb, "triangle", tm, sort)
                got = inst.allhits_batch(rb, tm, sort=sort)
                assert got["offsets"].tobytes() == off.tobytes() and got["shape"].tobytes() == sh.tobytes(), (sort,)
                assert got["vals"].tobytes() == vals.tobytes() and (got["instance"] == 0).all() and len(got["instance"]) == len(sh)
                assert (np.diff(off.astype(np.int64)) >= 2).sum() >= 50


# ---- 4. ray counts and empty sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_counts(eng, orc, ctx, dtype):
    c, rows = cluster_rows(orc, dtype, 37)
    table = c["free"]["table"]
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for m in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
            sub = dict(table, cand_off=table["cand_off"][:m + 1])
            for sort in (True, False):
                _agree(inst.allhits_batch(_rb(eng, c["rays"][:m]), c["tmax"][:m], sort=sort), iar.rows(sub, m, c["tmax"][:m], dtype, sort), (m, sort))
        got = inst.allhits_batch(_rb(eng, c["rays"][:0]))
        assert got["offsets"].tolist() == [0] and got["vals"].shape == (0, 3) and got["instance"].shape == (0,) and got["shape"].shape == (0,)
        assert got["vals"].dtype == dtype
        got = inst.allhits_batch(_dev_rays(eng, c["rays"][:0]), sort=False)
        assert got["offsets"].cpu().tolist() == [0] and tuple(got["vals"].shape) == (0, 3)
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for kw in (dict(), dict(sort=False), dict(count_only=True)):
            got = empty.allhits_batch(_rb(eng, c["rays"]), c["tmax"], **kw)
            assert got["offsets"].shape == (N_RAYS + 1,) and not got["offsets"].any()
            assert kw.get("count_only") or (len(got["instance"]) == 0 and got["vals"].shape == (0, 3))


# ---- 5. tree generations -------------------------------------------------------------------------------------------------------------------
def test_tree_generations(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    dtype = np.float32
    trees = member_trees(orc, dtype)
    (a_aabbs, a_tris), (b_aabbs, b_tris) = trees[0], trees[1]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    x = transforms(5, dtype, 31)
    rays = cluster_rays(orc, 600, dtype, 32)
    rb = _rb(eng, rays)

    def ref(tr, xf, sort=True):
        return iar.rows(ir.Scene([tr], [0] * 5, xf, dtype).trace(rays)["table"], len(rays), None, dtype, sort)

    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.allhits_batch(rb), ref(trees[0], x), "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        for kw in (dict(), dict(sort=False), dict(count_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.allhits_batch(rb, **kw)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x)
        # the first reader of the new generation is this entry
        got = inst.allhits_batch(rb)
        want = ref((b_aabbs[:100], b_tris[:100]), x)
        assert int(want[0][-1]) >= 100
        _agree(got, want, "after")
        fresh_member = _gpu_trees(eng, ctx, [(b_aabbs[:100], b_tris[:100])])[0]
        with eng.Instances([fresh_member], [0] * 5, x, ctx) as fresh:
            _agree(fresh.allhits_batch(rb), _host(got), "a fresh set")
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        for kw in (dict(), dict(count_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.allhits_batch(rb, **kw)
            assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        # a re-pose
        x2 = transforms(5, dtype, 999)
        inst.update(x2)
        want2 = ref((b_aabbs[:100], b_tris[:100]), x2)
        assert want2[1].tobytes() != want[1].tobytes()
        _agree(inst.allhits_batch(rb), want2, "re-posed")
        _agree(inst.allhits_batch(rb, sort=False), ref((b_aabbs[:100], b_tris[:100]), x2, False), "re-posed, list order")


# ---- 6. the result object ------------------------------------------------------------------------------------------------------------------
def test_one_result_object_through_every_rows_family(eng, orc, ctx):
    """one bvhgpu_hits used in turn by bvhgpu_traverse_allhits_*, bvhgpu_instances_region_*, this entry, bvhgpu_within_* and this entry again:
    each result is right and every wrong fetch is refused, by status and by message"""
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    c, rows = cluster_rows(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    tree = trees[1]
    aabbs, tris = c["trees"][1]
    rays = np.ascontiguousarray(c["rays"][150:450])              # (the batch's first 150 rays are the unaimed ones)
    table = c["free"]["table"]
    want = iar.rows(dict(table, cand_off=table["cand_off"][150:451]), 300, None, dtype)
    total = int(want[0][-1])
    assert total >= 50
    big = 200000
    so, si, ss, sv = (np.full(600, 0xABABABAB, np.uint32), np.full(big, 0xABABABAB, np.uint32), np.full(big, 0xABABABAB, np.uint32),
                      np.full((big, 3), 7.0, dtype))
    sb = np.full(big, 0xAB, np.uint8)
    mine = lib.bvhgpu_hits_fetch_instances_allhits
    RIGHT = "use bvhgpu_hits_fetch_instances_allhits"

    def untouched():
        return (so == 0xABABABAB).all() and (si == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (sv == 7.0).all() and (sb == 0xAB).all()

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def this_entry(h, flags=0):
        assert lib.bvhgpu_instances_allhits_f32(inst._s, ptr(rays), None, 300, HOST, flags, C.byref(h)) == OK
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
        off, gi, gs, gv = np.zeros(301, np.uint32), np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros((total, 3), dtype)
        assert mine(h, ptr(off), ptr(gi), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == want[0].tobytes() and gi.tobytes() == want[1].tobytes() and gs.tobytes() == want[2].tobytes()
        assert gv.tobytes() == want[3].tobytes()
        assert mine(h, None, None, None, None, HOST) == OK                     # each pointer may be NULL

    def other_kind(h, text):
        assert mine(h, ptr(so), ptr(si), ptr(ss), ptr(sv), HOST) == INVALID_ARG and text in err(), err()
        assert untouched()

    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        h = C.c_void_p()
        # bvhgpu_traverse_allhits_*
        assert lib.bvhgpu_traverse_allhits_f32(tree._t, ptr(rays), None, 300, HOST, _lib.LEAF_KINDS["triangle"], 0, C.byref(h)) == OK
        keep = h.value
        other_kind(h, "no bvhgpu_instances_allhits_")
        a_want = tree.allhits_batch(_rb(eng, rays), "triangle")     # (the tree's own result object; tests/test_gpu_allhits.py holds it to the oracle)
        assert int(a_want[0][-1]) >= 50
        off, gs, gv = np.zeros(301, np.uint32), np.zeros(len(a_want[1]), np.uint32), np.zeros((len(a_want[1]), 3), dtype)
        assert lib.bvhgpu_hits_fetch_allhits(h, ptr(off), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == a_want[0].tobytes() and gs.tobytes() == a_want[1].tobytes() and gv.tobytes() == a_want[2].tobytes()
        # bvhgpu_instances_region_*: every instance, every shape
        assert lib.bvhgpu_instances_region_f32(inst._s, None, 3, 0, HOST, 0, C.byref(h)) == OK and h.value == keep
        other_kind(h, "no bvhgpu_instances_allhits_")
        per = sum(len(c["trees"][t][0]) for t in c["tree_of"])
        off = np.zeros(4, np.uint32)
        assert lib.bvhgpu_hits_fetch_instances_region(h, ptr(off), None, None, None, HOST) == OK and off.tolist() == [0, per, 2 * per, 3 * per]
        # this entry
        this_entry(h)
        assert h.value == keep
        # bvhgpu_within_*
        pts = np.ascontiguousarray(((aabbs[:50, :3] + aabbs[:50, 3:]) / 2).astype(dtype))
        lim = np.full(50, 0.75, dtype)
        assert lib.bvhgpu_within_f32(tree._t, ptr(pts), ptr(lim), 50, HOST, 0, 0, C.byref(h)) == OK and h.value == keep
        other_kind(h, "no bvhgpu_instances_allhits_")
        w_got = tree.within_batch(pts, lim)
        off, gs, gv = np.zeros(51, np.uint32), np.zeros(len(w_got[1]), np.uint32), np.zeros(len(w_got[1]), dtype)
        assert lib.bvhgpu_hits_fetch_within(h, ptr(off), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == w_got[0].tobytes() and gs.tobytes() == w_got[1].tobytes() and gv.tobytes() == w_got[2].tobytes()
        assert int(off[-1]) >= 50
        # and this entry again, count-only and full
        this_entry(h, 2)
        this_entry(h, 0)
        # a closest-hit batch refuses this fetch too
        assert lib.bvhgpu_traverse_f32(tree._t, ptr(rays), 300, HOST, _lib.TRAVERSE_CLOSEST, C.byref(h)) == OK
        other_kind(h, "no bvhgpu_instances_allhits_")
        lib.bvhgpu_hits_destroy(h)


# ---- 7. the refusals of the raw C ABI, in the header's order ---------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    import torch
    from bvh_amd import _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype = np.float32
    c, rows = cluster_rows(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rays = np.ascontiguousarray(c["rays"][150:214])               # (the batch's first 150 rays are the unaimed ones)
    rays64 = np.ascontiguousarray(case(orc, np.float64, 37)["rays"][150:214])
    table = c["free"]["table"]
    want = iar.rows(dict(table, cand_off=table["cand_off"][150:215]), 64, None, dtype)
    total = int(want[0][-1])
    assert total >= 50
    f32, f64 = lib.bvhgpu_instances_allhits_f32, lib.bvhgpu_instances_allhits_f64
    STALE, UNCOMMITTED = "instances are stale: call bvhgpu_instances_update", "instances are not committed"

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text, h, keep=None):
        assert rc == status and text in err(), (rc, err())
        assert h.value == keep                                # *hits stays as it was

    member = eng.Bvh.from_aabbs(c["trees"][0][0], ctx)
    member.flatten_in_place()
    member.set_triangles(c["trees"][0][1])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances([member], [0] * 37, c["x"], ctx) as stale, \
            eng.Instances(trees, c["tree_of"], c["x"], ctx) as broken:
        member.rebuild(c["trees"][1][0][:100], flatten=True)
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        s = inst._s
        h = C.c_void_p()
        # 1. a NULL set or a NULL hits
        assert f32(None, ptr(rays), None, 64, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        assert f32(s, ptr(rays), None, 64, HOST, 0, None) == INVALID_ARG and "hits is NULL" in err()
        # 2. a result object that still holds an asynchronous batch: it wins over everything behind it
        rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        ha = C.c_void_p()
        assert lib.bvhgpu_traverse_async_f32(trees[1]._t, ptr(rays_dev.data_ptr()), 64, DEVICE, 0, C.byref(ha)) == OK
        held = ha.value
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, 8, C.byref(ha)), INVALID_ARG, "still holds an asynchronous batch", ha, held)
        assert lib.bvhgpu_hits_wait(ha) == OK
        lib.bvhgpu_hits_destroy(ha)
        # 3. .. 9., each alone
        refused(f32(s, None, None, 64, HOST, 0, C.byref(h)), INVALID_ARG, "rays is NULL", h)
        refused(f32(s, ptr(rays), None, 64, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE", h)
        refused(f64(s, ptr(rays64), None, 64, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "instance set dtype differs from ray dtype", h)
        for flags in (4, 8, 1 << 10, 1 << 25, 1 << 31, 3 | 16):
            refused(f32(s, ptr(rays), None, 64, HOST, flags, C.byref(h)), INVALID_ARG, "instance all-hits flags", h)
        refused(f32(broken._s, ptr(rays), None, 64, HOST, 0, C.byref(h)), INVALID_ARG, UNCOMMITTED, h)
        refused(f32(stale._s, ptr(rays), None, 64, HOST, 0, C.byref(h)), INVALID_ARG, STALE, h)
        refused(f32(s, ptr(rays), None, 0xFFFFFFFF, HOST, 0, C.byref(h)), OVERFLOW, "2^32-2 rays", h)
        # the order: an earlier rule wins over a later one
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "rays is NULL", h)
        refused(f64(stale._s, ptr(rays), None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "mem must be", h)
        refused(f64(stale._s, ptr(rays), None, 0xFFFFFFFF, HOST, 8, C.byref(h)), DTYPE_MISMATCH, "dtype", h)
        refused(f32(stale._s, ptr(rays), None, 0xFFFFFFFF, HOST, 8, C.byref(h)), INVALID_ARG, "instance all-hits flags", h)
        refused(f32(broken._s, ptr(rays), None, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, UNCOMMITTED, h)
        refused(f32(stale._s, ptr(rays), None, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, STALE, h)
        # the stale check is bvhgpu_instances_trace_*'s: the same words from both
        v, i, sh = np.zeros((64, 3), dtype), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
        assert lib.bvhgpu_instances_trace_f32(stale._s, ptr(rays), None, 64, HOST, 0, ptr(v), ptr(i), ptr(sh)) == INVALID_ARG
        trace_words = err()
        assert f32(stale._s, ptr(rays), None, 64, HOST, 0, C.byref(h)) == INVALID_ARG and err() == trace_words
        # NULL rays are fine where there is nothing to read
        assert f32(s, None, None, 0, HOST, 0, C.byref(h)) == OK and h.value
        keep = h.value
        so = np.full(65, 0xABABABAB, np.uint32)
        assert lib.bvhgpu_hits_fetch_instances_allhits(h, ptr(so), None, None, None, HOST) == OK and so[0] == 0 and (so[1:] == 0xABABABAB).all()
        # a refused batch leaves the result object as it was
        assert f32(s, ptr(rays), None, 64, HOST, 0, C.byref(h)) == OK and h.value == keep
        refused(f32(s, ptr(rays), None, 64, 7, 0, C.byref(h)), INVALID_ARG, "mem must be", h, keep)
        refused(f32(stale._s, ptr(rays), None, 64, HOST, 0, C.byref(h)), INVALID_ARG, STALE, h, keep)
        refused(f32(s, ptr(rays), None, 64, HOST, 4, C.byref(h)), INVALID_ARG, "instance all-hits flags", h, keep)
        nr, tot = C.c_size_t(), C.c_uint64()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (64, total)
        off, gi, gs, gv = np.zeros(65, np.uint32), np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros((total, 3), dtype)
        assert lib.bvhgpu_hits_fetch_instances_allhits(h, ptr(off), ptr(gi), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == want[0].tobytes() and gi.tobytes() == want[1].tobytes() and gs.tobytes() == want[2].tobytes()
        assert gv.tobytes() == want[3].tobytes()
        assert lib.bvhgpu_hits_fetch_instances_allhits(None, ptr(off), None, None, None, HOST) == INVALID_ARG
        lib.bvhgpu_hits_destroy(h)
