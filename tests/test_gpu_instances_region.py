"""Convex regions over instanced scenes on the GPU (bvhgpu_instances_region_*): every flag combination byte for byte against
tests/instances_region_ref.py (the definition over the oracle) on the scenes tests/test_instances_region_cpu.py shows to be non-trivial, in
f32 and f64, planes in HOST and in HBM; two anchors against bvh_amd.region_batch that do not pass through that reference; members of every
served kind; re-posing, staleness, refit and a failed update; the refusals of the raw C ABI in the header's order; the result kinds.
Nothing here provokes a fault: every refusal happens on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as fz
import instances_ref as ir
import instances_region_ref as irr
import region_ref as rr
from test_gpu_any_hit import _rb
from test_instances_region_cpu import exact_scene
from test_within_cpu import far_scene

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
COMBOS = ("plain", "classify", "count_only", "instances_only", "instances_only_classify")


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


def _call(inst, planes, combo="classify", device=False):
    """Instances.region_batch → (offsets u32, instance u32, shape u32 | None, inside u8 | None) as numpy, whichever memory the planes are in"""
    kw = dict(classify="classify" in combo, count_only=combo == "count_only", instances_only=combo.startswith("instances_only"))
    if not device:
        r = inst.region_batch(planes, **kw)
        assert r["offsets"].dtype == np.uint32 and r["instance"].dtype == np.uint32
        assert all(v.dtype == (np.uint8 if k == "inside" else np.uint32) for k, v in r.items())
        return r["offsets"], r["instance"], r.get("shape"), r.get("inside")
    import torch
    r = inst.region_batch(torch.from_numpy(np.ascontiguousarray(planes)).cuda(), **kw)
    assert all(v.is_cuda for v in r.values()) and r["offsets"].dtype == torch.int64 and r["instance"].dtype == torch.int32
    assert "shape" not in r or r["shape"].dtype == torch.int32
    assert "inside" not in r or r["inside"].dtype == torch.uint8
    on = r["offsets"].cpu().numpy()
    assert on.min(initial=0) >= 0
    u32 = lambda k: r[k].cpu().numpy().view(np.uint32) if k in r else None   # noqa: E731
    return on.astype(np.uint32), u32("instance"), u32("shape"), r["inside"].cpu().numpy() if "inside" in r else None


def _same(got, want, label):
    """got: _call's tuple; want: the same four (None where the combination has no such array)"""
    for name, g, w in zip(("offsets", "instance", "shape", "inside"), got, want):
        assert (g is None) == (w is None), (label, name)
        if g is not None:
            assert g.shape == w.shape, (label, name, g.shape, w.shape)
            bad = np.nonzero(g != w)[0]
            assert len(bad) == 0, (label, name, "differs at", bad[:5], g[bad[:5]], w[bad[:5]])


def _wanted(ref, combo):
    off, inst, shape, ins = ref["full"]
    toff, tidx, tins = ref["top"]
    none = np.zeros(0, dtype=np.uint32)
    return dict(plain=(off, inst, shape, None), classify=(off, inst, shape, ins), count_only=(off, none, none, None),
                instances_only=(toff, tidx, None, None), instances_only_classify=(toff, tidx, None, tins))[combo]


def _check(inst, planes, ref, label, mems=(False, True), combos=COMBOS):
    for device in mems:
        for combo in combos:
            _same(_call(inst, planes, combo, device), _wanted(ref, combo), (label, combo, "device" if device else "host"))


# ---- 1. the rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_main_scene_under_every_flag_combination(eng, orc, ctx, dtype):
    """4 members (1, 12, 240 and 8 400 shapes: 1 and 9 chunks in one launch), 37 instances, 52 regions"""
    m = irr.main_scene(dtype)
    trees = _gpu_trees(eng, ctx, m["trees"])
    with eng.Instances(trees, m["tree_of"], m["x"], ctx) as inst:
        assert inst.world_boxes.tobytes() == m["scene"].w.tobytes()
        _check(inst, m["planes"], m["ref"], "main")
        t = "float" if dtype == np.float32 else "double"
        inst.region_batch(m["planes"], classify=True)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_region_walk<{t}, true, true>"
        inst.region_batch(m["planes"], count_only=True)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_region_walk<{t}, false, false>"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", irr.CASES)
def test_batch_and_set_sizes_and_plane_counts(eng, orc, ctx, dtype, name):
    """irr.case: sets of 1 and 2 instances, only the one-triangle member, 2 500 regions (two chunks per pair of the large member), m in
    {0, 1, 32}, one region (the largest stride), no pair at all"""
    c = irr.case(dtype, name)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        _check(inst, c["planes"], c["ref"], name, mems=(False, True) if name != "many" else (True,))
        if name == "none":
            assert inst.region_batch(c["planes"])["offsets"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_regions_and_no_instances(eng, orc, ctx, dtype):
    m = irr.main_scene(dtype)
    trees = _gpu_trees(eng, ctx, m["trees"])
    with eng.Instances(trees, m["tree_of"], m["x"], ctx) as inst:
        for combo in COMBOS:
            for device in (False, True):
                got = _call(inst, np.zeros((0, 6, 4), dtype=dtype), combo, device)
                assert got[0].tolist() == [0] and len(got[1]) == 0 and (got[2] is None or len(got[2]) == 0), combo
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for combo in COMBOS:
            got = _call(empty, m["planes"], combo)
            assert got[0].tolist() == [0] * (len(m["planes"]) + 1) and len(got[1]) == 0, combo
        got = _call(empty, np.zeros((3, 0, 4), dtype=dtype), "plain")
        assert got[0].tolist() == [0, 0, 0, 0]


# ---- 2. anchors: not through the new reference's stage 2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_region_batch_over_the_member(eng, orc, ctx, dtype):
    aabbs, tris = irr.main_members(dtype)[3]
    member = _gpu_trees(eng, ctx, [(aabbs, tris)])[0]
    planes = rr.random_regions(aabbs, 30, 17)
    want = eng.region_batch(member, planes, classify=True)
    assert want["chunks"] > 1 and len(want["indices"]) > 1000
    with eng.Instances([member], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        got = inst.region_batch(planes, classify=True)
        assert got["offsets"].tobytes() == want["offsets"].tobytes() and got["shape"].tobytes() == want["indices"].tobytes()
        assert got["inside"].tobytes() == want["inside"].tobytes() and (got["instance"] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_translated_instances_equal_region_batch_over_the_flattened_scene(eng, orc, ctx, dtype):
    """X = [I | t] with every sum exact: the set of world-space boxes of a row is the flattened tree's row, as a set"""
    trees, of, x, planes = exact_scene(dtype)
    base = np.concatenate([[0], np.cumsum([len(trees[t][0]) for t in of])])
    world = np.ascontiguousarray(np.concatenate([trees[t][0] + np.tile(x[i, :, 3], 2) for i, t in enumerate(of)]))
    flat = eng.Bvh.from_aabbs(world, ctx).flatten()
    want = eng.region_batch(flat, planes)
    members = _gpu_trees(eng, ctx, trees)
    with eng.Instances(members, of, x, ctx) as inst:
        got = inst.region_batch(planes)
    assert got["offsets"].tobytes() == want["offsets"].tobytes() and want["offsets"][-1] > 100
    off = got["offsets"]
    for q in range(len(planes)):
        mine = base[got["instance"][off[q]:off[q + 1]]] + got["shape"][off[q]:off[q + 1]]
        assert sorted(mine.tolist()) == sorted(want["indices"][off[q]:off[q + 1]].tolist()), q


# ---- 3. members of every served kind -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_uploaded_flat_bvh_as_a_member(eng, orc, ctx, dtype):
    """the oracle's FlatNode array uploaded (the UNFOLDED rule, 3 chunks at one region) beside a built member (folded) in one launch"""
    from test_instances_cpu import transforms
    big, cube = irr.main_members(dtype)[2], irr.main_members(dtype)[1]
    a = np.ascontiguousarray(np.concatenate([big[0]] * 4) + np.repeat(np.arange(4, dtype=dtype), len(big[0]))[:, None] * dtype(0.25))
    tris = np.ascontiguousarray(np.concatenate([big[1]] * 4))
    sc = ir.Scene([(a, tris), cube], [0, 1, 0], transforms(3, dtype, 61), dtype)
    assert len(sc.flats[0]) == 3 * 960 - 2
    up = eng.FlatBvh.from_flat_nodes(sc.flats[0], a, ctx)
    up.set_triangles(tris)
    built = _gpu_trees(eng, ctx, [cube])[0]
    for planes in (rr.random_regions(sc.w, 20, 62), rr.random_regions(sc.w, 1, 63, max_planes=1)):
        ref = irr.reference(sc, planes)
        assert ref["full"][0][-1] > 50
        with eng.Instances([up, built], [0, 1, 0], sc.x, ctx) as inst:
            _check(inst, planes, ref, "uploaded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_member_with_empty_child_bounds_built_and_imported(eng, orc, ctx, dtype):
    """boxes so far apart that no bucket wins a split: the built member is walked through the unfolded mirror, whose empty navigator boxes
    are never entered (m = 0 enters everything); one instance, so the top level is one leaf.  A second set of three instances, two of whose
    world boxes coincide (a translation of 1 vanishes at 1e19), has a top level with empty child bounds as well: by the definition no
    region with a plane reaches an instance there.  The same member after scene export / import carries the folded array only: the query
    refuses it, create does not, and INSTANCES_ONLY reads no member"""
    far, tris = far_scene(dtype)[:2]
    x = np.eye(3, 4, dtype=dtype)[None].copy()                 # (a scene of this extent overflows the SAH of any top level with two boxes:
    x[0, 0, 0], x[0, 1, 1] = 0.5, -2.0                          #  one instance, scaled and mirrored)
    sc = ir.Scene([(far, tris)], [0], x, dtype)
    assert fz.has_empty_child_bounds(sc.flats[0])
    planes = rr.random_regions(sc.w, 30, 9)
    ref = irr.reference(sc, planes)
    assert len(ref["top"][1]) >= 20 and ref["full"][0][-1] == 0   # the root's children are empty: pairs that pass the top and report nothing
    member = eng.Bvh.from_aabbs(far, ctx).flatten()
    member.set_triangles(tris)
    zero = np.zeros((2, 0, 4), dtype)
    with eng.Instances([member], [0], x, ctx) as inst:
        _check(inst, planes, ref, "empty child bounds")
        _check(inst, zero, irr.reference(sc, zero), "empty child bounds, m = 0", mems=(False,))
    x3 = np.tile(np.eye(3, 4, dtype=dtype), (3, 1, 1))
    x3[1, :, 3] = [1, 2, 3]
    x3[2, 0, 0] = 0.5
    sc3 = ir.Scene([(far, tris)], [0, 0, 0], x3, dtype)
    assert fz.has_empty_child_bounds(sc3.top) and sc3.w[0].tobytes() == sc3.w[1].tobytes() != sc3.w[2].tobytes()
    ref3, ref30 = irr.reference(sc3, planes), irr.reference(sc3, zero)
    assert len(ref3["top"][1]) == 0 and ref30["full"][0].tolist() == [0, 3 * len(far), 6 * len(far)]
    with eng.Instances([member], [0, 0, 0], x3, ctx) as inst:
        _check(inst, planes, ref3, "coincident world boxes", mems=(False,))
        _check(inst, zero, ref30, "coincident world boxes, m = 0", mems=(False,))
    blob = np.zeros(member.scene_nbytes(), np.uint8)
    member.scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    imp.set_triangles(tris)
    with eng.Instances([imp], [0], x, ctx) as inst:
        for kw in (dict(), dict(classify=True), dict(count_only=True)):
            with pytest.raises(eng.BvhGpuError) as e:
                inst.region_batch(planes, **kw)
            assert e.value.status == 1 and "split without SAH winner" in str(e.value)
        _same(_call(inst, planes, "instances_only_classify"), _wanted(ref, "instances_only_classify"), "imported, instances only")


# ---- 4. re-pose, staleness, refit, a failed update --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_is_a_fresh_set(eng, orc, ctx, dtype):
    m = irr.main_scene(dtype)
    trees = _gpu_trees(eng, ctx, m["trees"])
    ref2 = irr.reference(ir.Scene(m["trees"], m["tree_of"], m["x2"], dtype), m["planes"])
    with eng.Instances(trees, m["tree_of"], m["x"], ctx) as inst, eng.Instances(trees, m["tree_of"], m["x2"], ctx) as fresh:
        before = _call(inst, m["planes"])
        inst.update(m["x2"])
        got = _call(inst, m["planes"])
        _same(got, _wanted(ref2, "classify"), "second pose")
        _same(got, _call(fresh, m["planes"]), "fresh set")
        assert before[0].tobytes() != got[0].tobytes()


def test_stale_refitted_and_uncommitted_sets(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    from test_instances_cpu import transforms
    dtype = np.float32
    members = irr.main_members(dtype)
    (a, a_tris), (b, b_tris) = members[2], members[3]
    member = eng.Bvh.from_aabbs(a, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    x = transforms(5, dtype, 31)
    sc = ir.Scene([(a, a_tris)], [0] * 5, x, dtype)
    planes = rr.random_regions(sc.w, 20, 32)
    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _check(inst, planes, irr.reference(sc, planes), "before", mems=(False,))
        # a refit keeps the arrays and the generation: the new boxes are committed by update, and the rows are the oracle's refit's
        moved = np.ascontiguousarray(a + np.tile(np.random.default_rng(33).uniform(-0.5, 0.5, size=(len(a), 3)).astype(dtype), 2))
        member.refit(moved)
        inst.update(x)
        sc2 = ir.Scene([(moved, a_tris)], [0] * 5, x, dtype)
        sc2.flats[0] = orc.flatten(orc.refit(orc.build(a).nodes, moved))
        ref2 = irr.reference(sc2, planes)
        assert ref2["full"][2].tobytes() != irr.reference(sc, planes)["full"][2].tobytes()
        _check(inst, planes, ref2, "refit", mems=(False,))
        # a rebuild with another shape count: new arrays, a new generation, no triangles
        member.rebuild(b[:1200], flatten=True)
        for kw in (dict(), dict(instances_only=True), dict(count_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.region_batch(planes, **kw)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        member.set_triangles(b_tris[:1200])
        inst.update(x)
        sc3 = ir.Scene([(b[:1200], b_tris[:1200])], [0] * 5, x, dtype)
        _check(inst, planes, irr.reference(sc3, planes), "after", mems=(False,))
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        for kw in (dict(), dict(instances_only=True)):
            with pytest.raises(BvhGpuError) as e:
                inst.region_batch(planes, **kw)
            assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        inst.update(x)
        _check(inst, planes, irr.reference(sc3, planes), "after a good update", mems=(False,), combos=("classify",))


# ---- 5. the refusals of the raw C ABI, in the header's order ----------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    m = irr.main_scene(np.float32)
    trees = _gpu_trees(eng, ctx, m["trees"])
    planes = np.ascontiguousarray(m["planes"][:4])
    want = irr.reference(m["scene"], planes)["full"]
    f32, f64 = lib.bvhgpu_instances_region_f32, lib.bvhgpu_instances_region_f64

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text, h, keep=None):
        assert rc == status and text in err(), (rc, err())
        assert h.value == keep                                # *hits stays as it was

    with eng.Instances(trees, m["tree_of"], m["x"], ctx) as inst:
        s = inst._s
        h = C.c_void_p()
        assert f32(None, ptr(planes), 4, 6, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        assert f32(s, ptr(planes), 4, 6, HOST, 0, None) == INVALID_ARG and "hits is NULL" in err()
        refused(f32(s, ptr(planes), 1, 33, HOST, 0, C.byref(h)), INVALID_ARG, "BVHGPU_REGION_MAX_PLANES", h)
        refused(f32(s, None, 4, 6, HOST, 0, C.byref(h)), INVALID_ARG, "planes is NULL", h)
        refused(f32(s, ptr(planes), 4, 6, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE", h)
        refused(f64(s, ptr(planes.astype(np.float64)), 4, 6, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "instance set dtype differs from plane dtype", h)
        for flags in (8, 16, 1 << 10, 1 << 31):
            refused(f32(s, ptr(planes), 4, 6, HOST, flags, C.byref(h)), INVALID_ARG, "instance region flags", h)
        refused(f32(s, None, 0xFFFFFFFF, 0, HOST, 0, C.byref(h)), OVERFLOW, "2^32-2 regions", h)
        # the order: an earlier rule wins over a later one
        refused(f32(s, None, 4, 33, 7, 8, C.byref(h)), INVALID_ARG, "BVHGPU_REGION_MAX_PLANES", h)
        refused(f64(s, None, 4, 6, 7, 8, C.byref(h)), INVALID_ARG, "planes is NULL", h)
        refused(f64(s, ptr(planes), 4, 6, 7, 8, C.byref(h)), INVALID_ARG, "mem must be", h)
        refused(f64(s, ptr(planes), 0xFFFFFFFF, 6, HOST, 8, C.byref(h)), DTYPE_MISMATCH, "dtype", h)
        refused(f32(s, ptr(planes), 0xFFFFFFFF, 6, HOST, 8, C.byref(h)), INVALID_ARG, "instance region flags", h)
        # bvhgpu_region_* keeps refusing bit 4
        refused(lib.bvhgpu_region_f32(trees[3]._t, ptr(planes), 4, 6, HOST, 4, C.byref(h)), INVALID_ARG, "region flags", h)
        # NULL planes are fine where there is nothing to read
        assert f32(s, None, 3, 0, HOST, 0, C.byref(h)) == OK and h.value
        keep = h.value
        # a result without CLASSIFY has no inside bytes, an INSTANCES_ONLY one no shapes: refused, outputs untouched
        assert f32(s, ptr(planes), 4, 6, HOST, 0, C.byref(h)) == OK and h.value == keep
        total = int(want[0][-1])
        so, si, ss = np.full(5, 0xABABABAB, np.uint32), np.full(total, 0xABABABAB, np.uint32), np.full(total, 0xABABABAB, np.uint32)
        sb = np.full(total, 0xAB, np.uint8)
        fetch = lib.bvhgpu_hits_fetch_instances_region
        assert fetch(h, ptr(so), ptr(si), ptr(ss), ptr(sb), HOST) == INVALID_ARG and "without BVHGPU_REGION_CLASSIFY" in err()
        assert fetch(h, ptr(so), ptr(si), ptr(ss), None, 9) == INVALID_ARG and "mem must be" in err()
        assert fetch(None, ptr(so), ptr(si), ptr(ss), None, HOST) == INVALID_ARG
        assert (so == 0xABABABAB).all() and (si == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (sb == 0xAB).all()
        # a refused batch leaves the result object as it was
        refused(f32(s, ptr(planes), 4, 33, HOST, 0, C.byref(h)), INVALID_ARG, "BVHGPU_REGION_MAX_PLANES", h, keep)
        refused(f32(s, ptr(planes), 4, 6, DEVICE + 5, 0, C.byref(h)), INVALID_ARG, "mem must be", h, keep)
        nr, tot = C.c_size_t(), C.c_uint64()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (4, total)
        assert fetch(h, ptr(so), ptr(si), ptr(ss), None, HOST) == OK
        assert so.tobytes() == want[0].tobytes() and si.tobytes() == want[1].tobytes() and ss.tobytes() == want[2].tobytes()
        assert f32(s, ptr(planes), 4, 6, HOST, 4, C.byref(h)) == OK
        ss[:] = 0xABABABAB
        assert fetch(h, ptr(so), ptr(si), ptr(ss), None, HOST) == INVALID_ARG and "BVHGPU_REGION_INSTANCES_ONLY" in err()
        assert (ss == 0xABABABAB).all()
        # more than 2^32 - 1 reported shapes: 64 000 regions without planes report every shape of every instance.  The total is checked
        # before anything is sized by it; the result object is then an empty result of this kind
        per_region = sum(len(m["trees"][t][0]) for t in m["tree_of"])
        assert 64000 * per_region > 0xFFFFFFFF > 64000 * 37
        refused(f32(s, None, 64000, 0, HOST, 0, C.byref(h)), OVERFLOW, "2^32-1", h, keep)
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (0, 0)
        so[:] = 0xABABABAB
        assert fetch(h, ptr(so), None, None, None, HOST) == OK and so[0] == 0 and (so[1:] == 0xABABABAB).all()
        assert f32(s, ptr(planes), 4, 6, HOST, 0, C.byref(h)) == OK and fetch(h, ptr(so), None, None, None, HOST) == OK
        assert so.tobytes() == want[0].tobytes()
        lib.bvhgpu_hits_destroy(h)


# ---- 6. the result kinds -----------------------------------------------------------------------------------------------------------------
def test_the_result_is_a_kind_of_its_own(eng, orc, ctx):
    """both directions between the two region kinds, every existing fetch on this result, this fetch on every ray result, and a result
    object of another kind reused by this entry and handed on"""
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    c = irr.case(dtype, "two")
    trees = _gpu_trees(eng, ctx, c["trees"])
    tree = trees[1]
    a = c["trees"][1][0]
    cen = (a[:, :3] + a[:, 3:]) / 2
    tree.set_spheres(np.ascontiguousarray(np.concatenate([cen, np.full((len(a), 1), 0.5, dtype)], axis=1)))
    rays = _rb(eng, np.ascontiguousarray(orc.create_rays(0, 500)))
    so, ss, sv = np.full(600, 0xABABABAB, np.uint32), np.full(200000, 0xABABABAB, np.uint32), np.full((200000, 3), 7.0, dtype)
    h = tree._hits
    fetch = lib.bvhgpu_hits_fetch_instances_region

    def untouched():
        return (so == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (sv == 7.0).all()

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    others = {
        "traverse": (lambda: tree.traverse_batch(rays), "no bvhgpu_instances_region_"),
        "query": (lambda: tree.query_batch("aabb", a[:50]), "no bvhgpu_instances_region_"),
        "closest": (lambda: tree.closest_hits(rays), "bvhgpu_hits_fetch_closest"),
        "any": (lambda: tree.any_hits(rays), "bvhgpu_hits_fetch_any"),
        "box": (lambda: tree.closest_box_hits(rays), "bvhgpu_hits_fetch_box"),
        "sphere": (lambda: tree.closest_sphere_hits(rays), "bvhgpu_hits_fetch_sphere"),
        "allhits": (lambda: tree.allhits_batch(rays), "bvhgpu_hits_fetch_allhits"),
        "within": (lambda: tree.within_batch(np.ascontiguousarray(cen[:50]), 100.0), "bvhgpu_hits_fetch_within"),
        "region": (lambda: eng.region_batch(tree, c["planes"]), "bvhgpu_hits_fetch_region"),
    }
    for kind, (run, text) in others.items():
        run()
        assert fetch(h.h, ptr(so), ptr(ss), ptr(ss), None, HOST) == INVALID_ARG, kind
        assert text in err(), (kind, err())
        assert untouched(), kind
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for flags in (0, 2, 4):
            # the tree's result object, which holds a plain region result, is reused by this entry
            assert getattr(lib, "bvhgpu_instances_region_f32")(inst._s, ptr(c["planes"]), len(c["planes"]), 6, HOST, flags, C.byref(h.h)) == OK
            fetches = {
                "region": lambda: lib.bvhgpu_hits_fetch_region(h.h, ptr(so), ptr(ss), None, HOST),
                "fetch": lambda: lib.bvhgpu_hits_fetch(h.h, ptr(so), ptr(ss), None, HOST),
                "triangles": lambda: lib.bvhgpu_hits_fetch_triangles(h.h, ptr(sv), HOST),
                "closest": lambda: lib.bvhgpu_hits_fetch_closest(h.h, ptr(sv), ptr(ss), HOST),
                "any": lambda: lib.bvhgpu_hits_fetch_any(h.h, ptr(sv), ptr(ss), HOST),
                "box": lambda: lib.bvhgpu_hits_fetch_box(h.h, ptr(sv), ptr(ss), HOST),
                "sphere": lambda: lib.bvhgpu_hits_fetch_sphere(h.h, ptr(sv), ptr(ss), HOST),
                "allhits": lambda: lib.bvhgpu_hits_fetch_allhits(h.h, ptr(so), ptr(ss), ptr(sv), HOST),
                "within": lambda: lib.bvhgpu_hits_fetch_within(h.h, ptr(so), ptr(ss), ptr(sv), HOST),
                "device": lambda: lib.bvhgpu_hits_device(h.h, None, None, None),
            }
            for name, f in fetches.items():
                assert f() == INVALID_ARG, (flags, name)
                assert ("bvhgpu_hits_fetch_instances_region" if name == "region" else "bvhgpu_hits_fetch_region") in err(), (flags, name, err())
                assert untouched(), (flags, name)
        off, inst_, shape = np.zeros(len(c["planes"]) + 1, np.uint32), np.zeros(int(c["ref"]["full"][0][-1]), np.uint32), None
        assert lib.bvhgpu_instances_region_f32(inst._s, ptr(c["planes"]), len(c["planes"]), 6, HOST, 0, C.byref(h.h)) == OK
        shape = np.zeros_like(inst_)
        assert fetch(h.h, ptr(off), ptr(inst_), ptr(shape), None, HOST) == OK
        assert off.tobytes() == c["ref"]["full"][0].tobytes() and inst_.tobytes() == c["ref"]["full"][1].tobytes()
        assert shape.tobytes() == c["ref"]["full"][2].tobytes()
    # and the result object goes on to the next kinds of batch: a plain region result is plain again
    want = rr.walk(rr.oracle_tree(a), a, c["planes"])
    got = eng.region_batch(tree, c["planes"], classify=True)
    assert got["offsets"].tobytes() == want[0].tobytes() and got["indices"].tobytes() == want[1].tobytes() and got["inside"].tobytes() == want[2].tobytes()
    off, idx, _, _ = tree.traverse_batch(rays)
    ooff, oidx, _, _ = orc.traverse_flat(rr.oracle_tree(a), a, np.ascontiguousarray(orc.create_rays(0, 500)))
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
