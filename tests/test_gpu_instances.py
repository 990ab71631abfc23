"""Instanced scenes on the GPU (bvhgpu_instances_*): world boxes, closest and first hits byte for byte against tests/instances_ref.py (the
definition over the oracle) on the scenes tests/test_instances_cpu.py shows to be non-trivial; an identity anchor against the single-tree
walks that does not pass through that reference; re-posing, staleness, a failed update, edge sizes and the refusals of the raw C ABI.
Nothing here provokes a fault: a stale or uncommitted set is refused on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import instances_ref as ir
from knn_ref import same
from test_gpu_any_hit import _rb
from test_instances_cpu import SIZES, case, cluster_rays, member_trees, transforms

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
    """(vals, instance, shape) as numpy, indices as uint32 (rays in HBM come back as torch tensors, indices as int32)"""
    vals, inst, shape = got
    if not isinstance(vals, np.ndarray):
        import torch
        assert inst.dtype == torch.int32 and shape.dtype == torch.int32 and vals.is_cuda
        vals, inst, shape = vals.cpu().numpy(), inst.cpu().numpy().view(np.uint32), shape.cpu().numpy().view(np.uint32)
    return vals, inst, shape


def _agree(got, want, label):
    vals, inst, shape = _host(got)
    assert inst.dtype == np.uint32 and shape.dtype == np.uint32, label
    assert inst.tobytes() == want[1].tobytes(), label
    assert shape.tobytes() == want[2].tobytes(), label
    assert same(vals, want[0]), label


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_with_the_reference(eng, orc, ctx, dtype, n):
    c = case(orc, dtype, n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        assert inst.info() == (3, n)
        assert inst.world_boxes.tobytes() == c["scene"].w.tobytes()
        for tm, want in ((None, c["free"]), (c["tmax"], c["cut"])):
            rb = _rb(eng, c["rays"])
            _agree(inst.closest_hits(rb, tm), want["closest"], (n, "closest", "host"))
            _agree(inst.any_hits(rb, tm), want["first"], (n, "first", "host"))
            assert np.array_equal(inst.occluded(rb, tm), want["first"][1] != NONE)
            import torch
            rd = _dev_rays(eng, c["rays"])
            td = None if tm is None else torch.from_numpy(tm).cuda()
            _agree(inst.closest_hits(rd, td), want["closest"], (n, "closest", "device"))
            _agree(inst.any_hits(rd, td), want["first"], (n, "first", "device"))
            assert np.array_equal(inst.occluded(rd, td).cpu().numpy(), want["first"][1] != NONE)
        # transforms as n x 12 and as a GPU tensor give the same set
        with eng.Instances(trees, torch.from_numpy(c["tree_of"].astype(np.int32)).cuda(), torch.from_numpy(c["x"].reshape(n, 12)).cuda(), ctx) as dev:
            assert dev.world_boxes.tobytes() == c["scene"].w.tobytes()
            _agree(dev.closest_hits(_rb(eng, c["rays"])), c["free"]["closest"], (n, "device transforms"))


# ---- 2. identity anchor: not through the new reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree_walk(eng, orc, ctx, dtype):
    trees = member_trees(orc, dtype)
    B = _gpu_trees(eng, ctx, [trees[1]])[0]
    rays = cluster_rays(orc, 1500, dtype, 21)
    rays["o"] *= dtype(0.2)
    rb = _rb(eng, rays)
    isect, shape = B.closest_hits(rb)[:2]
    assert (shape != NONE).sum() >= 100
    tmax = (np.where(np.isfinite(isect[:, 0]), isect[:, 0], 50) * np.random.default_rng(5).uniform(0.3, 1.7, len(rays))).astype(dtype)
    with eng.Instances([B], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        vals, ii, ss = inst.closest_hits(rb)
        assert vals.tobytes() == isect.tobytes() and ss.tobytes() == shape.tobytes()
        assert (ii[shape != NONE] == 0).all() and (ii[shape == NONE] == NONE).all()
        aisect, ashape = B.any_hits(rb, tmax)
        vals, ii, ss = inst.any_hits(rb, tmax)
        assert vals.tobytes() == aisect.tobytes() and ss.tobytes() == ashape.tobytes()
        assert (ii[ashape != NONE] == 0).all() and (ii[ashape == NONE] == NONE).all()
        assert 20 <= (ashape != NONE).sum() < (shape != NONE).sum()


# ---- 3. update ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_is_a_fresh_set(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    x2 = transforms(37, dtype, 999)
    sc2 = ir.Scene(c["trees"], c["tree_of"], x2, dtype)
    want = sc2.trace(c["rays"], c["tmax"])
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances(trees, c["tree_of"], x2, ctx) as fresh:
        before = inst.closest_hits(rb, c["tmax"])
        assert inst.update(x2) is inst
        assert inst.world_boxes.tobytes() == sc2.w.tobytes() == fresh.world_boxes.tobytes()
        for call in ("closest_hits", "any_hits"):
            got, ref = getattr(inst, call)(rb, c["tmax"]), getattr(fresh, call)(rb, c["tmax"])
            _agree(got, want["closest" if call == "closest_hits" else "first"], call)
            _agree(got, ref, call)
        assert before[1].tobytes() != inst.closest_hits(rb, c["tmax"])[1].tobytes()


# ---- 4. staleness and a failed update ---------------------------------------------------------------------------------------------------
def test_a_rebuilt_member_makes_the_set_stale(eng, orc, ctx):
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
    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.closest_hits(rb), ir.Scene([trees[0]], [0] * 5, x, dtype).trace(rays)["closest"], "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        for call in (inst.closest_hits, inst.any_hits):
            with pytest.raises(BvhGpuError) as e:
                call(rb)
            assert e.value.status == _lib.INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        with pytest.raises(BvhGpuError) as e:                           # the update re-checks the members: no triangles yet
            inst.update(x)
        assert e.value.status == _lib.INVALID_ARG and "set_triangles" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x)
        _agree(inst.closest_hits(rb), ir.Scene([(b_aabbs[:100], b_tris[:100])], [0] * 5, x, dtype).trace(rays)["closest"], "after")


def test_a_failed_update_leaves_the_set_uncommitted(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    dtype = np.float32
    c = case(orc, dtype, 2)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rb = _rb(eng, c["rays"])
    bad = c["x"].copy()
    bad[1, 0, 0] = np.nan
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        with pytest.raises(BvhGpuError) as e:
            inst.update(bad)
        assert e.value.status == _lib.INVALID_ARG
        for call in (lambda: inst.closest_hits(rb), lambda: inst.any_hits(rb), lambda: inst.world_boxes):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == _lib.INVALID_ARG and "not committed" in str(e.value)
        inst.update(c["x"])
        _agree(inst.closest_hits(rb), c["free"]["closest"], "after a good update")
    with pytest.raises(BvhGpuError) as e:                               # a failed create returns no set
        eng.Instances(trees, c["tree_of"], bad, ctx)
    assert e.value.status == _lib.INVALID_ARG


# ---- 5. edge sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_sizes(eng, orc, ctx, dtype):
    c = case(orc, dtype, 1)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        assert empty.info() == (3, 0) and empty.world_boxes.shape == (0, 6)
        for call in (empty.closest_hits, empty.any_hits):
            vals, inst, shape = call(rb, c["tmax"])
            assert (inst == NONE).all() and (shape == NONE).all()
            assert np.isinf(vals[:, 0]).all() and (vals[:, 0] > 0).all() and (vals[:, 1:] == 0).all()
        assert not empty.occluded(rb).any()
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as one:
        none = _rb(eng, c["rays"][:0])
        vals, inst, shape = one.closest_hits(none)
        assert vals.shape == (0, 3) and inst.shape == (0,) and shape.shape == (0,)
        _agree(one.closest_hits(_rb(eng, c["rays"][:1])), tuple(a[:1] for a in c["free"]["closest"]), "one ray")


# ---- 6. the refusals of the raw C ABI -----------------------------------------------------------------------------------------------------
def test_refusals(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, ptr
    lib = _lib.load()
    trees32 = _gpu_trees(eng, ctx, member_trees(orc, np.float32))
    tree64 = _gpu_trees(eng, ctx, member_trees(orc, np.float64))[0]
    other_ctx = eng.Context(0)
    foreign = _gpu_trees(eng, other_ctx, member_trees(orc, np.float32)[:1])[0]
    a_aabbs, a_tris = member_trees(orc, np.float32)[0]
    unflat = eng.Bvh.from_aabbs(a_aabbs, ctx)
    bare = eng.Bvh.from_aabbs(a_aabbs, ctx).flatten()                  # flattened, no triangles
    x = transforms(2, np.float32, 41)
    of = np.array([0, 1], dtype=np.uint32)

    def handles(ts):
        return (C.c_void_p * len(ts))(*[t._t.value for t in ts])

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def create(ts, tof=of, xf=x, n=2, mem=HOST, f="f32", out=True, arr=True):
        h = C.c_void_p()
        rc = getattr(lib, f"bvhgpu_instances_create_{f}")(ctx._h, handles(ts) if arr else None, len(ts), ptr(tof), ptr(xf), n, mem,
                                                         C.byref(h) if out else None)
        assert rc == OK or not h.value, "a refused create returns no set"
        return rc, h

    good = trees32[:2]
    assert create(good, out=False)[0] == INVALID_ARG and "NULL" in err()
    assert create(good, arr=False)[0] == INVALID_ARG and "NULL argument" in err()
    assert create(good, xf=None)[0] == INVALID_ARG and "NULL argument" in err()
    assert create(good, tof=None)[0] == INVALID_ARG and "NULL argument" in err()
    assert create(good, mem=7)[0] == INVALID_ARG and "mem must be BVHGPU_HOST or BVHGPU_DEVICE" in err()
    assert create([trees32[0], tree64])[0] == DTYPE_MISMATCH and "dtype" in err()
    assert create(good, f="f64", xf=x.astype(np.float64))[0] == DTYPE_MISMATCH and "dtype" in err()
    assert create([trees32[0], foreign])[0] == INVALID_ARG and "another context" in err()
    assert create([trees32[0], unflat])[0] == NOT_FLATTENED and "bvhgpu_flatten" in err()
    assert create([trees32[0], bare])[0] == INVALID_ARG and "bvhgpu_tree_set_triangles" in err()
    assert create([unflat, tree64])[0] == DTYPE_MISMATCH                   # the first broken rule wins, whichever member breaks it
    assert create(good, tof=np.array([0, 2], dtype=np.uint32))[0] == INVALID_ARG and "tree_of" in err()
    rc, h = create(good)
    assert rc == OK and h.value
    try:
        dt, nt, ni = C.c_int(-1), C.c_size_t(99), C.c_size_t(99)
        assert lib.bvhgpu_instances_info(h, C.byref(dt), C.byref(nt), C.byref(ni)) == OK and (dt.value, nt.value, ni.value) == (0, 2, 2)
        assert lib.bvhgpu_instances_info(None, None, None, None) == INVALID_ARG
        # update
        assert lib.bvhgpu_instances_update_f32(None, ptr(x), 2, HOST) == INVALID_ARG
        assert lib.bvhgpu_instances_update_f32(h, None, 2, HOST) == INVALID_ARG and "NULL argument" in err()
        assert lib.bvhgpu_instances_update_f32(h, ptr(x), 2, 7) == INVALID_ARG and "mem must be" in err()
        assert lib.bvhgpu_instances_update_f64(h, ptr(x.astype(np.float64)), 2, HOST) == DTYPE_MISMATCH and "dtype" in err()
        assert lib.bvhgpu_instances_update_f32(h, ptr(transforms(3, np.float32, 1)), 3, HOST) == INVALID_ARG and "number of instances differs" in err()
        # trace: every refusal leaves the outputs as they were
        rays = cluster_rays(orc, 64, np.float32, 42)
        rays64 = cluster_rays(orc, 64, np.float64, 42)
        vals = np.full((64, 3), -7.5, dtype=np.float32)
        inst, shape = np.full(64, 0xABCD1234, dtype=np.uint32), np.full(64, 0x1234ABCD, dtype=np.uint32)
        sentinel = (vals.tobytes(), inst.tobytes(), shape.tobytes())

        def trace(s=h, r=rays, n=64, mem=HOST, flags=0, v=vals, i=inst, sh=shape, f="f32"):
            rc = getattr(lib, f"bvhgpu_instances_trace_{f}")(s, ptr(r), None, n, mem, flags, ptr(v), ptr(i), ptr(sh))
            assert rc == OK or (vals.tobytes(), inst.tobytes(), shape.tobytes()) == sentinel, "a refused trace wrote to an output"
            return rc

        assert trace(s=None) == INVALID_ARG
        assert trace(r=None) == INVALID_ARG and "NULL argument" in err()
        assert trace(v=None) == INVALID_ARG and "NULL argument" in err()
        assert trace(i=None) == INVALID_ARG and "NULL argument" in err()
        assert trace(sh=None) == INVALID_ARG and "NULL argument" in err()
        assert trace(mem=2) == INVALID_ARG and "mem must be" in err()
        assert trace(r=rays64, f="f64", v=np.zeros((64, 3))) == DTYPE_MISMATCH and "dtype" in err()
        for flags in (1, 8, 16, 1024 | 16, 1 << 31):
            assert trace(flags=flags) == INVALID_ARG and "0 or BVHGPU_TRAVERSE_FIRST" in err()
        # the order: an earlier rule wins over a later one (NULL argument, mem, dtype, flags, then the commit rule)
        assert trace(r=None, mem=2, f="f64", flags=8) == INVALID_ARG and "NULL argument" in err()
        assert trace(r=rays64, mem=2, f="f64", flags=8) == INVALID_ARG and "mem must be" in err()
        assert trace(r=rays64, f="f64", flags=8) == DTYPE_MISMATCH and "dtype" in err()
        bad = x.copy()
        bad.reshape(-1)[0] = np.nan
        assert lib.bvhgpu_instances_update_f32(h, ptr(bad), 2, HOST) == INVALID_ARG       # (a failed update: the set is uncommitted)
        assert trace(flags=8) == INVALID_ARG and "0 or BVHGPU_TRAVERSE_FIRST" in err()
        assert trace() == INVALID_ARG and "not committed" in err()
        assert lib.bvhgpu_instances_update_f32(h, ptr(x), 2, HOST) == OK
        assert lib.bvhgpu_instances_boxes(h, None, HOST) == INVALID_ARG and "out is NULL" in err()
        assert lib.bvhgpu_instances_boxes(h, ptr(np.zeros((2, 6), dtype=np.float32)), 9) == INVALID_ARG and "mem must be" in err()
        assert trace(n=0, r=None, v=None, i=None, sh=None) == OK          # n_rays == 0 needs nothing
        assert trace() == OK and trace(flags=1024) == OK
        assert (vals.tobytes(), inst.tobytes(), shape.tobytes()) != sentinel
    finally:
        lib.bvhgpu_instances_destroy(h)
        lib.bvhgpu_instances_destroy(None)
        foreign.close()
        other_ctx.close()
