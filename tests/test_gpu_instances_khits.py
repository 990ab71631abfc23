"""k-hits over instanced scenes on the GPU (bvhgpu_instances_khits_*): every row byte for byte against the definition of
tests/instances_khits_ref.py (the sorted all-hits rows cut to k and padded) on the inputs tests/test_instances_khits_cpu.py shows to be
worth running — the cluster scene free and cut, HOST and HBM; the stack scene with row lengths planned around every k and ties at the cut,
at every block size; anchors that do not pass through the new reference (the engine's own all-hits cut in numpy, closest_hits at k = 1, an
identity instance against the member's own khits_batch); edge sizes, empty sets, all-miss rays and useless tmax; tree generations and the
refusals of the raw C ABI.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import numpy as np
import pytest

import instances_khits_ref as ikh
import instances_ref as ir
from test_gpu_any_hit import _rb
from test_instances_allhits_cpu import stack_case
from test_instances_cpu import N_RAYS, SIZES, case, cluster_rays, member_trees, transforms
from test_instances_khits_cpu import K, block_lds, cluster_want, stack_plan

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
ANCHOR_KS = (1, 3, 9, 17, 64)


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


def _host(got, dtype):
    """(instance, shape, vals) as numpy, indices as uint32 (rays in HBM come back as torch tensors)"""
    inst, shape, vals = got
    if not isinstance(inst, np.ndarray):
        import torch
        assert inst.dtype == torch.int32 and shape.dtype == torch.int32 and vals.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
        assert inst.is_cuda and shape.is_cuda and vals.is_cuda
        inst, shape, vals = inst.cpu().numpy().view(np.uint32), shape.cpu().numpy().view(np.uint32), vals.cpu().numpy()
    return inst, shape, vals


def _agree(got, want, dtype, label):
    inst, shape, vals = _host(got, dtype)
    assert inst.dtype == np.uint32 and shape.dtype == np.uint32 and vals.dtype == dtype, label
    assert inst.shape == shape.shape == want[0].shape and vals.shape == want[2].shape, (label, inst.shape, vals.shape)
    assert inst.tobytes() == want[0].tobytes(), label
    assert shape.tobytes() == want[1].tobytes(), label
    assert vals.tobytes() == want[2].tobytes(), label


def _cut_csr(got, n, k, dtype):
    """the engine's own sorted all-hits CSR cut to k and padded, in numpy"""
    off = got["offsets"].astype(np.int64)
    oi, os_ = np.full((n, k), NONE, np.uint32), np.full((n, k), NONE, np.uint32)
    ov = np.zeros((n, k, 3), dtype)
    ov[:, :, 0] = np.inf
    for j in range(n):
        m = min(k, int(off[j + 1] - off[j]))
        oi[j, :m], os_[j, :m], ov[j, :m] = got["instance"][off[j]:off[j] + m], got["shape"][off[j]:off[j] + m], got["vals"][off[j]:off[j] + m]
    return oi, os_, ov


# ---- 1. the cluster scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene(eng, orc, ctx, dtype, n):
    import torch
    c = case(orc, dtype, n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        rb, rd = _rb(eng, c["rays"]), _dev_rays(eng, c["rays"])
        for cut in (False, True):
            tm = c["tmax"] if cut else None
            td = torch.from_numpy(c["tmax"]).cuda() if cut else None
            for k in (1, 2, 3, 4, 8):
                want = cluster_want(orc, dtype, n, cut, k)
                _agree(inst.khits_batch(rb, k, tm), want, dtype, (n, cut, k, "host"))
                got = inst.khits_batch(rd, k, td)
                assert got[0].device == rd.device.device and tuple(got[2].shape) == (N_RAYS, k, 3)
                _agree(got, want, dtype, (n, cut, k, "device"))


# ---- 2. the stack scene: row lengths around k, ties at the cut, every block size -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stack_scene(eng, orc, ctx, dtype):
    s = stack_case(orc, dtype)
    trees = _gpu_trees(eng, ctx, s["trees"])
    assert {block_lds(k, dtype)[0] for k in K} == {256, 128, 64}
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        for k in K:
            p = stack_plan(orc, dtype, k)
            _agree(inst.khits_batch(_rb(eng, p["rays"]), k, p["tmax"]), p["want"], dtype, ("stack", k))


# ---- 3. anchors that do not pass through the new reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_the_heads_of_the_engines_own_allhits(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for tm in (None, c["tmax"]):
            full = inst.allhits_batch(rb, tm, sort=True)
            assert (np.diff(full["offsets"].astype(np.int64)) >= 2).sum() >= 20
            for k in ANCHOR_KS:
                _agree(inst.khits_batch(rb, k, tm), _cut_csr(full, N_RAYS, k, dtype), dtype, ("cluster", k))
            # k = 1 is closest_hits
            vals, ii, ss = inst.closest_hits(rb, tm)
            gi, gs, gv = inst.khits_batch(rb, 1, tm)
            assert gv[:, 0].tobytes() == vals.tobytes() and gi[:, 0].tobytes() == ii.tobytes() and gs[:, 0].tobytes() == ss.tobytes()
            assert 20 <= (ii != NONE).sum() <= N_RAYS - 20
    s = stack_case(orc, dtype)
    trees = _gpu_trees(eng, ctx, s["trees"])
    with eng.Instances(trees, s["tree_of"], s["x"], ctx) as inst:
        for k in ANCHOR_KS:
            p = stack_plan(orc, dtype, k)
            rb = _rb(eng, p["rays"])
            full = inst.allhits_batch(rb, p["tmax"], sort=True)
            _agree(inst.khits_batch(rb, k, p["tmax"]), _cut_csr(full, len(p["rays"]), k, dtype), dtype, ("stack", k))
        vals, ii, ss = inst.closest_hits(rb, p["tmax"])
        gi, gs, gv = inst.khits_batch(rb, 1, p["tmax"])
        assert gv[:, 0].tobytes() == vals.tobytes() and gi[:, 0].tobytes() == ii.tobytes() and gs[:, 0].tobytes() == ss.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_members_own_khits(eng, orc, ctx, dtype):
    """one identity instance of the stack member (128 triangles, 64 of them hit from either side) against FlatBvh.khits_batch on that member"""
    s = stack_case(orc, dtype)
    S = _gpu_trees(eng, ctx, [s["trees"][0]])[0]
    rays = np.ascontiguousarray(s["rays"][:64])
    rb = _rb(eng, rays)
    tmax = np.random.default_rng(5).uniform(4.0, 14.0, len(rays)).astype(dtype)
    tmax[1::4] += dtype(392.0)                                           # the rays that come back from z = 405
    tmax[0] = 4.5                                                        # in front of the first triangle: an empty row
    with eng.Instances([S], [0], np.eye(3, 4, dtype=dtype)[None], ctx) as inst:
        for k in ANCHOR_KS:
            for tm in (None, tmax):
                vals, shape = S.khits_batch(rb, k, "triangle", tm)
                gi, gs, gv = inst.khits_batch(rb, k, tm)
                assert gs.tobytes() == shape.tobytes() and gv.tobytes() == vals.tobytes(), (k, tm is None)
                assert np.array_equal(gi == 0, shape != NONE) and np.array_equal(gi == NONE, shape == NONE)
            filled = (shape != NONE).sum(axis=1)
            assert (filled > 0).sum() >= 32 and filled[0] == 0, k                # rows with entries, and one that is all padding


# ---- 4. ray counts, empty sets, rays that miss, tmax that admits nothing ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_counts(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (8, 16, 64):                                            # blocks of 256, 128 and 64 lanes
            want = cluster_want(orc, dtype, 37, True, k)
            for m in (0, 1, 63, 64, 65, 257):
                _agree(inst.khits_batch(_rb(eng, c["rays"][:m]), k, c["tmax"][:m]), tuple(w[:m] for w in want), dtype, (k, m))
            _agree(inst.khits_batch(_dev_rays(eng, c["rays"][:65]), k), tuple(w[:65] for w in cluster_want(orc, dtype, 37, False, k)), dtype, (k, "device"))
        gi, gs, gv = inst.khits_batch(_rb(eng, c["rays"][:0]), 3)
        assert gi.shape == gs.shape == (0, 3) and gv.shape == (0, 3, 3) and gv.dtype == dtype
        gi, gs, gv = inst.khits_batch(_dev_rays(eng, c["rays"][:0]), 3)
        assert tuple(gi.shape) == (0, 3) and tuple(gv.shape) == (0, 3, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding(eng, orc, ctx, dtype):
    import torch
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    n = 130
    o = np.random.default_rng(3).uniform(-5, 5, size=(n, 3))
    o[:, 0] += 100.0
    d = np.tile([[1.0, 0.0, 0.0]], (n, 1))                               # from x ~ 100 along +x: away from the cluster
    away = orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        for k in (1, 8, 16, 64):
            want = ikh.padding(n, k, dtype)
            _agree(inst.khits_batch(_rb(eng, away), k), want, dtype, ("all miss", k))
            _agree(inst.khits_batch(_dev_rays(eng, away), k), want, dtype, ("all miss, device", k))
            for bad in (0.0, -0.0, -1.0, np.nan, -np.inf):
                _agree(inst.khits_batch(_rb(eng, c["rays"][:n]), k, np.full(n, bad, dtype)), want, dtype, ("tmax", bad, k))
        ti, _, tv = inst.khits_batch(_dev_rays(eng, away), 5)
        assert (ti == -1).all() and torch.isposinf(tv[:, :, 0]).all()    # NONE reads -1 in torch.int32
        # a mixed tmax: rows of the rays it spares are what they were
        tm = c["tmax"][:n].copy()
        tm[::2] = np.nan
        want = [w[:n].copy() for w in cluster_want(orc, dtype, 37, True, 8)]
        pad = ikh.padding(n, 8, dtype)
        for w, p in zip(want, pad):
            w[::2] = p[::2]
        _agree(inst.khits_batch(_rb(eng, c["rays"][:n]), 8, tm), want, dtype, "mixed tmax")
    with eng.Instances(trees, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        for k in (1, 5, 64):
            for rays in (_rb(eng, c["rays"][:n]), _dev_rays(eng, c["rays"][:n])):
                _agree(empty.khits_batch(rays, k, None), ikh.padding(n, k, dtype), dtype, ("no instances", k))
        _agree(empty.khits_batch(_rb(eng, c["rays"][:n]), 5, c["tmax"][:n]), ikh.padding(n, 5, dtype), dtype, "no instances, tmax")


# ---- 5. tree generations -------------------------------------------------------------------------------------------------------------------
def test_tree_generations(eng, orc, ctx):
    from bvh_amd import BvhGpuError, _lib
    from bvh_amd._lib import HOST, INVALID_ARG, ptr
    dtype, k = np.float32, 5
    trees = member_trees(orc, dtype)
    (a_aabbs, a_tris), (b_aabbs, b_tris) = trees[0], trees[1]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    x = transforms(5, dtype, 31)
    rays = cluster_rays(orc, 600, dtype, 32)
    rb = _rb(eng, rays)

    def ref(tr, xf):
        return ikh.definition(ir.Scene([tr], [0] * 5, xf, dtype).trace(rays)["table"], len(rays), None, k, dtype)

    with eng.Instances([member], [0] * 5, x, ctx) as inst:
        _agree(inst.khits_batch(rb, k), ref(trees[0], x), dtype, "before")
        member.rebuild(b_aabbs[:100], flatten=True)                      # another shape count: new arrays, a new generation, no triangles
        with pytest.raises(BvhGpuError) as e:
            inst.khits_batch(rb, k)
        assert e.value.status == INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        # the stale call through the raw ABI leaves the output buffers as they were
        oi, os_, ov = np.full((600, k), 0xABABABAB, np.uint32), np.full((600, k), 0xABABABAB, np.uint32), np.full((600, k, 3), 7.0, dtype)
        rc = _lib.load().bvhgpu_instances_khits_f32(inst._s, ptr(rays), None, 600, HOST, k, ptr(oi), ptr(os_), ptr(ov))
        assert rc == INVALID_ARG and (oi == 0xABABABAB).all() and (os_ == 0xABABABAB).all() and (ov == 7.0).all()
        member.set_triangles(b_tris[:100])
        inst.update(x)
        new = (b_aabbs[:100], b_tris[:100])
        want = ref(new, x)
        assert (want[1] != NONE).sum() >= 100
        got = inst.khits_batch(rb, k)                                    # the first reader of the new generation is this entry
        _agree(got, want, dtype, "after")
        # a re-pose: the rows follow the new pose
        x2 = transforms(5, dtype, 999)
        inst.update(x2)
        want2 = ref(new, x2)
        assert want2[0].tobytes() != want[0].tobytes()
        _agree(inst.khits_batch(rb, k), want2, dtype, "re-posed")
        # a failed update (a NaN) leaves the set refusing
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        with pytest.raises(BvhGpuError) as e:
            inst.khits_batch(rb, k)
        assert e.value.status == INVALID_ARG and "not committed" in str(e.value)


# ---- 6. the refusals of the raw C ABI, in the header's order ---------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype, k = np.float32, 5
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rays = np.ascontiguousarray(c["rays"][150:214])               # (the batch's first 150 rays are the unaimed ones)
    rays64 = np.ascontiguousarray(case(orc, np.float64, 37)["rays"][150:214])
    want = tuple(w[150:214] for w in cluster_want(orc, dtype, 37, False, k))
    assert (want[1] != NONE).sum() >= 50
    f32, f64 = lib.bvhgpu_instances_khits_f32, lib.bvhgpu_instances_khits_f64
    STALE, UNCOMMITTED = "instances are stale: call bvhgpu_instances_update", "instances are not committed"
    oi, os_, ov = np.full((64, 64), 0xABABABAB, np.uint32), np.full((64, 64), 0xABABABAB, np.uint32), np.full((64, 64, 3), 7.0, dtype)
    ov64 = np.full((64, 64, 3), 7.0, np.float64)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text):
        assert rc == status and text in err(), (rc, err())
        assert (oi == 0xABABABAB).all() and (os_ == 0xABABABAB).all() and (ov == 7.0).all() and (ov64 == 7.0).all()

    member = eng.Bvh.from_aabbs(c["trees"][0][0], ctx)
    member.flatten_in_place()
    member.set_triangles(c["trees"][0][1])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances([member], [0] * 37, c["x"], ctx) as stale, \
            eng.Instances(trees, c["tree_of"], c["x"], ctx) as broken:
        member.rebuild(c["trees"][1][0][:100], flatten=True)             # a member without triangles, of another generation
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        s = inst._s
        R, I, S, V = ptr(rays), ptr(oi), ptr(os_), ptr(ov)
        # each rule alone
        assert f32(None, R, None, 64, HOST, k, I, S, V) == INVALID_ARG
        refused(INVALID_ARG, INVALID_ARG, "")
        for bad_k in (0, _lib.INSTANCES_KHITS_MAX_K + 1, 0xFFFFFFFF):
            refused(f32(s, R, None, 64, HOST, bad_k, I, S, V), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KHITS_MAX_K")
        refused(f32(s, None, None, 64, HOST, k, I, S, V), INVALID_ARG, "NULL argument")
        refused(f32(s, R, None, 64, HOST, k, None, S, V), INVALID_ARG, "NULL argument")
        refused(f32(s, R, None, 64, HOST, k, I, None, V), INVALID_ARG, "NULL argument")
        refused(f32(s, R, None, 64, HOST, k, I, S, None), INVALID_ARG, "NULL argument")
        refused(f32(s, R, None, 64, 7, k, I, S, V), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE")
        refused(f64(s, ptr(rays64), None, 64, HOST, k, I, S, ptr(ov64)), DTYPE_MISMATCH, "instance set dtype differs from ray dtype")
        refused(f32(broken._s, R, None, 64, HOST, k, I, S, V), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, R, None, 64, HOST, k, I, S, V), INVALID_ARG, STALE)
        # n * k = 2^32 and n = 2^32 - 1: refused before anything is sized by them, allocated or launched
        refused(f32(s, R, None, 1 << 26, HOST, 64, I, S, V), OVERFLOW, "too many results (rays x k)")
        refused(f32(s, R, None, 0xFFFFFFFF, HOST, 1, I, S, V), OVERFLOW, "too many results (rays x k)")
        # the order: an earlier rule wins over a later one
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, 0, I, S, V), INVALID_ARG, "k must be")
        refused(f64(stale._s, None, None, 0xFFFFFFFF, 7, k, I, S, V), INVALID_ARG, "NULL argument")
        refused(f64(stale._s, R, None, 0xFFFFFFFF, 7, k, I, S, V), INVALID_ARG, "mem must be")
        refused(f64(stale._s, R, None, 0xFFFFFFFF, HOST, k, I, S, V), DTYPE_MISMATCH, "dtype")
        refused(f32(broken._s, R, None, 0xFFFFFFFF, HOST, k, I, S, V), INVALID_ARG, UNCOMMITTED)
        refused(f32(stale._s, R, None, 0xFFFFFFFF, HOST, k, I, S, V), INVALID_ARG, STALE)
        # the stale check is bvhgpu_instances_trace_*'s: the same words from both
        v, ti, tsh = np.zeros((64, 3), dtype), np.zeros(64, np.uint32), np.zeros(64, np.uint32)
        assert lib.bvhgpu_instances_trace_f32(stale._s, R, None, 64, HOST, 0, ptr(v), ptr(ti), ptr(tsh)) == INVALID_ARG
        trace_words = err()
        assert f32(stale._s, R, None, 64, HOST, k, I, S, V) == INVALID_ARG and err() == trace_words
        # NULL buffers are fine where there is nothing to read or write
        assert f32(s, None, None, 0, HOST, k, None, None, None) == OK
        refused(OK, OK, "")
        # a later valid call still answers, on the set that refused
        gi, gs, gv = np.zeros((64, k), np.uint32), np.zeros((64, k), np.uint32), np.zeros((64, k, 3), dtype)
        assert f32(s, R, None, 64, HOST, k, ptr(gi), ptr(gs), ptr(gv)) == OK
        _agree((gi, gs, gv), want, dtype, "after the refusals")
        _agree(inst.khits_batch(_rb(eng, rays), k), want, dtype, "after the refusals, through the binding")
        # the binding refuses a k out of range by the engine's status, and a ray batch of another dtype by itself
        for bad_k in (0, 65, -1):
            with pytest.raises(_lib.BvhGpuError) as e:
                inst.khits_batch(_rb(eng, rays), bad_k)
            assert e.value.status == INVALID_ARG and "k must be" in str(e.value)
        with pytest.raises(_lib.BvhGpuError) as e:
            inst.khits_batch(_rb(eng, rays64), k)
        assert e.value.status == DTYPE_MISMATCH
