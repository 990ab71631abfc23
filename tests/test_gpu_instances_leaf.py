"""Instance sets of BOX and SPHERE leaves on the GPU (bvhgpu_instances_create_leaf_*): every ray family byte for byte against
tests/instances_leaf_ref.py (the definition over the oracle) on the scenes tests/test_instances_leaf_cpu.py shows to be non-trivial, f32 and
f64, rays in host memory and in HBM; an identity anchor against the single-tree sphere and box queries that does not pass through that
reference; region queries; staleness by the set's own array; edge sizes and the refusals of the raw C ABI.
Nothing here provokes a fault: every refusal is decided on the host before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_khits_ref as ikr
import instances_leaf_ref as ilr
import instances_masks_ref as imr
from test_gpu_any_hit import _rb
from test_gpu_instances import _dev_rays
from test_instances_cpu import cluster_rays, transforms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
KS = (1, 3, 64)


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


def _gpu_trees(eng, ctx, trees, spheres=True):
    out = []
    for aabbs, sph in trees:
        flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        if spheres:
            flat.set_spheres(sph)
        out.append(flat)
    return out


def _np(a):
    """numpy as it is; a torch tensor on the GPU as numpy, int32 indices as uint32 (NONE reads as -1 there), int64 offsets as uint32"""
    if isinstance(a, np.ndarray):
        return a
    import torch
    assert a.is_cuda
    a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else (a.astype(np.uint32) if a.dtype == np.int64 else a)


def _same(got, want, label):
    """byte for byte, column by column (want: a reference result already cut to two scalars by ilr.two)"""
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (label, k)


def _csr(d):
    return d["offsets"], d["instance"], d["shape"], d["vals"]


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ilr.SIZES)
@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_with_the_reference(eng, orc, ctx, dtype, leaf, n):
    import torch
    c = ilr.case(dtype, n, leaf)
    nr = ilr.N_RAYS
    table = c["free"]["table"]
    trees = _gpu_trees(eng, ctx, c["trees"], spheres=leaf == "sphere")       # (a box set's members carry neither triangles nor spheres)
    M, R = c["inst_mask"], c["ray_mask"]
    with eng.Instances(trees, c["tree_of"], c["x"], ctx, leaf=leaf) as inst:
        assert inst.leaf == leaf and inst.info() == (3, n)
        assert inst.world_boxes.tobytes() == c["scene"].w.tobytes()
        inst.set_masks(M)
        for where in ("host", "device"):
            rb = _rb(eng, c["rays"]) if where == "host" else _dev_rays(eng, c["rays"])
            up = (lambda a: a) if where == "host" else (lambda a: None if a is None else torch.from_numpy(a).cuda())
            rm = R if where == "host" else torch.from_numpy(R.view(np.int32)).cuda()
            for tm, want in ((None, c["free"]), (c["tmax"], c["cut"])):
                tag = (n, leaf, where, tm is None)
                closest = inst.closest_hits(rb, up(tm))
                _same(closest, ilr.two(want["closest"]), tag + ("closest",))
                _same(inst.any_hits(rb, up(tm)), ilr.two(want["first"]), tag + ("first",))
                assert np.array_equal(_np(inst.occluded(rb, up(tm))), want["first"][1] != NONE)
                for k in KS if where == "host" else (3,):
                    got = inst.khits_batch(rb, k, up(tm))
                    _same(got, ilr.two(ikr.definition(table, nr, tm, k, dtype)), tag + ("khits", k))
                    if k == 1:       # k = 1 is closest_hits
                        _same((got[2][:, 0], got[0][:, 0], got[1][:, 0]), tuple(_np(a) for a in closest), tag + ("k = 1",))
                srt = inst.allhits_batch(rb, up(tm))
                _same(_csr(srt), ilr.two(iar.rows(table, nr, tm, dtype, sort=True)), tag + ("allhits sorted",))
                if where == "host":
                    lst = inst.allhits_batch(rb, tm, sort=False)
                    _same(_csr(lst), ilr.two(iar.rows(table, nr, tm, dtype, sort=False)), tag + ("allhits list order",))
                    cnt = inst.allhits_batch(rb, tm, count_only=True)
                    assert set(cnt) == {"offsets"} and cnt["offsets"].tobytes() == srt["offsets"].tobytes() == lst["offsets"].tobytes()
                    # the head of a sorted row is the closest hit, of a list-order row the first
                    for rows, ref in ((srt, want["closest"]), (lst, want["first"])):
                        off = rows["offsets"].astype(np.int64)
                        full = np.nonzero(np.diff(off))[0]
                        assert np.array_equal(full, np.nonzero(ref[1] != NONE)[0])
                        assert rows["vals"][off[full]].tobytes() == np.ascontiguousarray(ref[0][full, :2]).tobytes()
                        assert np.array_equal(rows["instance"][off[full]], ref[1][full]) and np.array_equal(rows["shape"][off[full]], ref[2][full])
                # the masked forms: one mask per ray against the set's, over the visible instances
                _same(inst.closest_hits_masked(rb, rm, up(tm)), ilr.two(imr.closest(table, M, R, nr, tm, dtype)), tag + ("masked closest",))
                _same(inst.any_hits_masked(rb, rm, up(tm)), ilr.two(imr.first(table, M, R, nr, tm, dtype)), tag + ("masked first",))
                if where == "host":
                    assert np.array_equal(inst.occluded_masked(rb, rm, tm), imr.first(table, M, R, nr, tm, dtype)[1] != NONE)
                    _same(inst.khits_masked_batch(rb, 3, rm, tm), ilr.two(imr.khits(table, M, R, nr, tm, 3, dtype)), tag + ("masked khits",))
                    for so in (True, False):
                        _same(_csr(inst.allhits_masked_batch(rb, rm, tm, sort=so)), ilr.two(imr.allhits(table, M, R, nr, tm, dtype, sort=so)),
                              tag + ("masked allhits", so))


# ---- 2. identity anchor: not through the new reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree_query(eng, orc, ctx, dtype, leaf):
    aabbs, sph = ilr.member_trees(dtype)[2]
    B = _gpu_trees(eng, ctx, [(aabbs, sph)])[0]
    rays = cluster_rays(orc, 1500, dtype, 21)
    rays["o"] *= dtype(0.2)
    rb = _rb(eng, rays)
    one_closest, one_first = (B.closest_sphere_hits, B.first_sphere_hits) if leaf == "sphere" else (B.closest_box_hits, B.first_box_hits)
    hit, shape = one_closest(rb)
    assert (shape != NONE).sum() >= 100
    tmax = (np.where(np.isfinite(hit[:, 0]), hit[:, 0], 50) * np.random.default_rng(5).uniform(0.3, 1.7, len(rays))).astype(dtype)
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx, leaf=leaf) as inst:
        for tm in (None, tmax):
            for mine, theirs in ((inst.closest_hits, one_closest), (inst.any_hits, one_first)):
                hit, shape = theirs(rb, tm)
                vals, ii, ss = mine(rb, tm)
                assert vals.tobytes() == hit.tobytes() and ss.tobytes() == shape.tobytes()
                assert (ii[shape != NONE] == 0).all() and (ii[shape == NONE] == NONE).all()
            for k in KS:
                v1, s1 = B.khits_batch(rb, k, leaf, tm)
                ii, ss, vals = inst.khits_batch(rb, k, tm)
                assert vals.tobytes() == v1.tobytes() and ss.tobytes() == s1.tobytes() and np.array_equal(ii == NONE, s1 == NONE)
            for so in (True, False):
                off, s1, v1 = B.allhits_batch(rb, leaf, tm, sort=so)
                rows = inst.allhits_batch(rb, tm, sort=so)
                assert rows["offsets"].tobytes() == off.tobytes() and rows["shape"].tobytes() == s1.tobytes() and rows["vals"].tobytes() == v1.tobytes()
                assert not rows["instance"].any() and len(s1) >= 100
        cut = one_first(rb, tmax)[1] != NONE
        assert 20 <= cut.sum() < (one_closest(rb)[1] != NONE).sum()


# ---- 2b. a row beyond the all-hits tier that sorts in LDS -------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_sorted_in_global_memory(eng, orc, ctx, dtype, leaf):
    """12 instances of 240 nested spheres around the origin, each instance a little off the last: a ray through the middle has 2 880
    candidates, more than INST_ALLHITS_LDS_ROW_MAX, so its row is sorted in place in global memory with records 2 scalars apart"""
    r = np.linspace(1.0, 3.0, 240).reshape(-1, 1)
    sph = np.ascontiguousarray(np.concatenate([np.zeros((240, 3)), r], axis=1).astype(dtype))
    aabbs = np.ascontiguousarray(np.concatenate([sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]], axis=1))
    x = np.tile(np.eye(3, 4, dtype=dtype)[None], (12, 1, 1))
    x[:, :, 3] = np.random.default_rng(9).uniform(-0.2, 0.2, size=(12, 3))
    o = np.random.default_rng(10).uniform(-0.3, 0.3, size=(8, 3)) + [-20, 0, 0]
    rays = orc.make_rays(o.astype(dtype), np.tile(np.array([[1.0, 0, 0]], dtype), (8, 1)), dtype)
    rays = np.concatenate([rays, cluster_rays(orc, 56, dtype, 11)])           # ... among shorter rows and misses
    want = ilr.LeafScene([(aabbs, sph)], [0] * 12, x, dtype, leaf).trace(rays)
    lds_max = iar.engine_thresholds(ROOT)[1]
    tree = _gpu_trees(eng, ctx, [(aabbs, sph)])[0]
    with eng.Instances([tree], [0] * 12, x, ctx, leaf=leaf) as inst:
        for so in (True, False):
            ref = iar.rows(want["table"], len(rays), None, dtype, sort=so)
            assert np.diff(ref[0].astype(np.int64)).max() > lds_max
            _same(_csr(inst.allhits_batch(_rb(eng, rays), sort=so)), ilr.two(ref), (leaf, so))
        _same(inst.khits_batch(_rb(eng, rays), 64), ilr.two(ikr.definition(want["table"], len(rays), None, 64, dtype)), leaf)
        _same(inst.closest_hits(_rb(eng, rays)), ilr.two(want["closest"]), leaf)


# ---- 3. regions read boxes only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_on_a_box_set_is_the_triangle_set(eng, orc, ctx, dtype):
    c = ilr.case(dtype, 37, "box")
    trees = _gpu_trees(eng, ctx, c["trees"], spheres=False)
    for t, (aabbs, _) in zip(trees, c["trees"]):   # any triangles will do: a region never reads them
        t.set_triangles(np.ascontiguousarray(np.stack([aabbs[:, :3], aabbs[:, 3:], aabbs[:, [0, 4, 2]]], axis=1)))
    lo, hi = np.array([-4, -5, -3], dtype), np.array([5, 3, 6], dtype)
    planes = np.stack([eng.aabb_planes(lo, hi, dtype=dtype), eng.aabb_planes(lo * 3, hi * 3, dtype=dtype), eng.aabb_planes(hi, hi + 1, dtype=dtype)])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx, leaf="box") as box, eng.Instances(trees, c["tree_of"], c["x"], ctx) as tri:
        for kw in (dict(), dict(classify=True), dict(instances_only=True), dict(count_only=True)):
            a, b = box.region_batch(planes, **kw), tri.region_batch(planes, **kw)
            assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), kw
        assert len(box.region_batch(planes)["shape"]) >= 100
        a, b = box.region_masked_batch(planes, 5), tri.region_masked_batch(planes, 5)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- 4. a box set needs nothing but boxes; edge sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_sizes(eng, orc, ctx, dtype, leaf):
    c = ilr.case(dtype, 1, leaf)
    trees = _gpu_trees(eng, ctx, c["trees"], spheres=leaf == "sphere")
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx, leaf=leaf) as empty:
        assert empty.info() == (3, 0)
        for call in (empty.closest_hits, empty.any_hits):
            vals, inst, shape = call(rb, c["tmax"])
            assert vals.shape == (ilr.N_RAYS, 2) and (inst == NONE).all() and (shape == NONE).all()
            assert np.isinf(vals[:, 0]).all() and (vals[:, 0] > 0).all() and (vals[:, 1] == 0).all()
        ii, ss, vals = empty.khits_batch(rb, 3)
        assert vals.shape == (ilr.N_RAYS, 3, 2) and (ii == NONE).all() and (ss == NONE).all() and np.isinf(vals[..., 0]).all() and not vals[..., 1].any()
        rows = empty.allhits_batch(rb)
        assert not rows["offsets"].any() and rows["vals"].shape == (0, 2)
    with eng.Instances(trees, c["tree_of"], c["x"], ctx, leaf=leaf) as one:
        none = _rb(eng, c["rays"][:0])
        vals, inst, shape = one.closest_hits(none)
        assert vals.shape == (0, 2) and inst.shape == (0,) and shape.shape == (0,)
        assert one.khits_batch(none, 3)[2].shape == (0, 3, 2) and one.allhits_batch(none)["vals"].shape == (0, 2)
        _same(one.closest_hits(_rb(eng, c["rays"][:1])), tuple(a[:1] for a in ilr.two(c["free"]["closest"])), "one ray")


# ---- 5. staleness follows the array of the set's kind ----------------------------------------------------------------------------------------
def test_a_rebuilt_member_makes_a_sphere_set_stale(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    dtype = np.float32
    trees = ilr.member_trees(dtype)
    (a_aabbs, a_sph), (b_aabbs, b_sph) = trees[1], trees[2]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_spheres(a_sph)
    x = transforms(5, dtype, 31)
    rays = cluster_rays(orc, 600, dtype, 32)
    rb = _rb(eng, rays)
    with eng.Instances([member], [0] * 5, x, ctx, leaf="sphere") as inst:
        _same(inst.closest_hits(rb), ilr.two(ilr.LeafScene([trees[1]], [0] * 5, x, dtype, "sphere").trace(rays)["closest"]), "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no spheres
        for call in (lambda: inst.closest_hits(rb), lambda: inst.any_hits(rb), lambda: inst.khits_batch(rb, 2), lambda: inst.allhits_batch(rb)):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        with pytest.raises(BvhGpuError) as e:                           # the update applies the set's own kind's rule: no spheres yet
            inst.update(x)
        assert e.value.status == _lib.INVALID_ARG and "bvhgpu_tree_set_spheres" in str(e.value)
        member.set_spheres(b_sph[:100])
        with pytest.raises(BvhGpuError) as e:                           # the spheres are back, the commit is still the old member's
            inst.closest_hits(rb)
        assert "instances are stale" in str(e.value)
        inst.update(x)
        want = ilr.LeafScene([(b_aabbs[:100], b_sph[:100])], [0] * 5, x, dtype, "sphere").trace(rays)
        _same(inst.closest_hits(rb), ilr.two(want["closest"]), "after")
        _same(inst.any_hits(rb), ilr.two(want["first"]), "after")
        assert (want["closest"][1] != NONE).sum() >= 50


# ---- 6. the refusals of the raw C ABI --------------------------------------------------------------------------------------------------------
def test_refusals(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    trees = ilr.member_trees(dtype)
    with_spheres = _gpu_trees(eng, ctx, trees[:2])
    bare = _gpu_trees(eng, ctx, trees[:2], spheres=False)              # flattened; neither triangles nor spheres
    unflat = eng.Bvh.from_aabbs(trees[0][0], ctx)
    x = transforms(2, dtype, 41)
    of = np.array([0, 1], dtype=np.uint32)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def create(ts, leaf):
        h = C.c_void_p()
        arr = (C.c_void_p * len(ts))(*[t._t.value for t in ts])
        rc = lib.bvhgpu_instances_create_leaf_f32(ctx._h, arr, len(ts), ptr(of), ptr(x), 2, HOST, leaf, C.byref(h))
        assert rc == OK or not h.value, "a refused create returns no set"
        return rc, h

    LEAF = "leaf must be BVHGPU_LEAF_BOX, BVHGPU_LEAF_TRIANGLE or BVHGPU_LEAF_SPHERE"
    for leaf in (3, -1, 1 << 20):
        assert create(with_spheres, leaf)[0] == INVALID_ARG and LEAF in err()
    assert create([with_spheres[0], unflat], 7)[0] == INVALID_ARG and LEAF in err()       # before the member rules
    assert create([with_spheres[0], unflat], _lib.LEAF_BOX)[0] == _lib.NOT_FLATTENED      # ... which a box set's members must pass too
    assert create(bare, _lib.LEAF_SPHERE)[0] == INVALID_ARG and "bvhgpu_tree_set_spheres" in err()
    assert create([with_spheres[0], bare[1]], _lib.LEAF_SPHERE)[0] == INVALID_ARG and "bvhgpu_tree_set_spheres" in err()
    assert create(with_spheres, _lib.LEAF_TRIANGLE)[0] == INVALID_ARG and "instances need bvhgpu_tree_set_triangles on every member tree first" in err()
    with pytest.raises(BvhGpuError) as e:
        eng.Instances(bare, of, x, ctx, leaf="sphere")
    assert e.value.status == INVALID_ARG and "bvhgpu_tree_set_spheres" in str(e.value)
    with pytest.raises(ValueError):
        eng.Instances(bare, of, x, ctx, leaf="cube")
    assert lib.bvhgpu_instances_leaf(None, None) == INVALID_ARG

    pts = np.random.default_rng(3).uniform(-5, 5, size=(64, 3)).astype(dtype)
    md = np.full(64, 2.0, dtype=dtype)
    msg = "point queries measure triangle distance"
    for leaf, members in ((_lib.LEAF_BOX, bare), (_lib.LEAF_SPHERE, with_spheres)):       # a box set over members with neither array is created
        rc, h = create(members, leaf)
        assert rc == OK and h.value
        try:
            got = C.c_int(-1)
            assert lib.bvhgpu_instances_leaf(h, C.byref(got)) == OK and got.value == leaf and lib.bvhgpu_instances_leaf(h, None) == OK
            dist = np.full((64, 3), -7.5, dtype=dtype)
            ii, ss = np.full((64, 3), 0xABCD1234, dtype=np.uint32), np.full((64, 3), 0x1234ABCD, dtype=np.uint32)
            sentinel = (dist.tobytes(), ii.tobytes(), ss.tobytes())
            mask = np.full(64, 0xFFFFFFFF, dtype=np.uint32)
            calls = {
                "knearest": lambda: lib.bvhgpu_instances_knearest_f32(h, ptr(pts), 64, HOST, 3, ptr(ii), ptr(ss), ptr(dist)),
                "knearest_tree": lambda: lib.bvhgpu_instances_knearest_tree_f32(h, ptr(pts), 64, HOST, 3, ptr(md), ptr(ii), ptr(ss), ptr(dist)),
                "knearest_masked": lambda: lib.bvhgpu_instances_knearest_masked_f32(h, ptr(pts), ptr(mask), 64, HOST, 3, ptr(ii), ptr(ss), ptr(dist)),
                "knearest_tree_masked": lambda: lib.bvhgpu_instances_knearest_tree_masked_f32(h, ptr(pts), ptr(mask), 64, HOST, 3, ptr(md), ptr(ii), ptr(ss),
                                                                                             ptr(dist)),
            }
            for name, call in calls.items():
                assert call() == INVALID_ARG and msg in err(), name
                assert (dist.tobytes(), ii.tobytes(), ss.tobytes()) == sentinel, name
            for name, call in (("within", lambda hp: lib.bvhgpu_instances_within_f32(h, ptr(pts), ptr(md), 64, HOST, 0, hp)),
                               ("within_masked", lambda hp: lib.bvhgpu_instances_within_masked_f32(h, ptr(pts), ptr(md), ptr(mask), 64, HOST, 0, hp))):
                hits = C.c_void_p()
                assert call(C.byref(hits)) == INVALID_ARG and msg in err() and not hits.value, name
            # the refusal comes directly after the dtype rule: a flag bit that within would refuse is not reached, a wrong dtype is
            hits = C.c_void_p()
            assert lib.bvhgpu_instances_within_f32(h, ptr(pts), ptr(md), 64, HOST, 1 << 20, C.byref(hits)) == INVALID_ARG and msg in err()
            assert lib.bvhgpu_instances_within_f64(h, ptr(pts.astype(np.float64)), ptr(md.astype(np.float64)), 64, HOST, 0,
                                                   C.byref(hits)) == _lib.DTYPE_MISMATCH and not hits.value
            # the ray families answer: 2 scalars per record
            rays = cluster_rays(orc, 64, dtype, 42)
            vals = np.full((64, 2), -7.5, dtype=dtype)
            assert lib.bvhgpu_instances_trace_f32(h, ptr(rays), None, 64, HOST, 0, ptr(vals), ptr(ii[:, 0].copy()), ptr(ss[:, 0].copy())) == OK
            assert not (vals == -7.5).any()
            assert lib.bvhgpu_instances_trace_f32(h, None, None, 0, HOST, 0, None, None, None) == OK          # n_rays == 0 needs nothing
        finally:
            lib.bvhgpu_instances_destroy(h)
    # the Python class hands the refusal on
    with eng.Instances(bare, of, x, ctx, leaf="box") as inst:
        for call in (lambda: inst.within_batch(pts, 2.0), lambda: inst.knearest_batch(pts, 3), lambda: inst.nearest_batch(pts),
                     lambda: inst.knearest_tree_batch(pts, 3), lambda: inst.within_masked_batch(pts, 2.0, 1), lambda: inst.knearest_masked_batch(pts, 3, 1)):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == INVALID_ARG and msg in str(e.value)
        assert (inst.closest_hits(_rb(eng, cluster_rays(orc, 600, dtype, 43)))[1] != NONE).sum() >= 20
