"""Per-instance visibility masks on the GPU (bvhgpu_instances_set_masks, bvhgpu_instances_{trace,khits,allhits}_masked_*): everything byte
for byte.  The three cluster scenes with the masks tests/test_instances_masks_cpu.py shows to be worth running, against the filtered
definition of tests/instances_masks_ref.py — f32 and f64, HOST and HBM rays, free and cut; the anchor that does not pass through the new
reference (the engine's own unmasked all-hits rows of the same run with the invisible pairs filtered out in numpy, and their heads); the
all-ones identity with every unmasked entry; the edges; the masks' lifetime over update, a failed update and a stale member; the refusals
of the eight symbols.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import instances_khits_ref as ikh
import instances_masks_ref as imr
import instances_ref as ir
from test_gpu_any_hit import _rb
from test_instances_cpu import N_RAYS, SIZES, case, cluster_rays, member_trees, transforms
from test_instances_masks_cpu import ALL, HIGH, KS, inst_masks, masked_want, ray_masks

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


def _dev_mask(mask):
    import torch
    return torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint32).view(np.int32).copy()).cuda()


def _gpu_trees(eng, ctx, trees):
    out = []
    for aabbs, tris in trees:
        flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris)
        out.append(flat)
    return out


def _np(x, index=False):
    if isinstance(x, np.ndarray):
        return x
    x = x.cpu().numpy()
    return x.view(np.uint32) if index else x


def _same(got, want, index, label):
    """a tuple of arrays (torch tensors of rays in HBM brought home; `index`: which are indices) against the reference's, byte for byte"""
    assert len(got) == len(want), label
    for k, (g, w, ix) in enumerate(zip(got, want, index)):
        g = _np(g, ix)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (label, k)


def _trace_same(got, want, label):
    _same(got, want, (False, True, True), label)


def _khits_same(got, want, label):
    _same(got, want, (True, True, False), label)


def _csr(got):
    off = got["offsets"]
    off = off if isinstance(off, np.ndarray) else off.cpu().numpy().astype(np.uint32)
    if set(got) == {"offsets"}:
        return (off,)
    return off, _np(got["instance"], True), _np(got["shape"], True), _np(got["vals"])


def _csr_same(got, want, label):
    g = _csr(got)
    assert len(g) == len(want), label
    for k, (a, b) in enumerate(zip(g, want)):
        assert a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a.tobytes() == b.tobytes(), (label, k)


def _filter_csr(full, M, R, n):
    """the engine's own unmasked CSR with the pairs of invisible instances taken out, in numpy"""
    off, inst, shape, vals = _csr(full)
    ray_of = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    keep = (M[inst.astype(np.int64)] & R[ray_of]) != 0
    new_off = np.concatenate([[0], np.cumsum(np.bincount(ray_of[keep], minlength=n))]).astype(np.uint32)
    return new_off, np.ascontiguousarray(inst[keep]), np.ascontiguousarray(shape[keep]), np.ascontiguousarray(vals[keep])


def _heads(rows, n, dtype):
    """(vals[n,3], instance[n], shape[n]): the first entry of every row, a miss where the row is empty"""
    oi, os_, ov = ikh.cut_rows(rows, n, 1, dtype)
    return np.ascontiguousarray(ov[:, 0]), np.ascontiguousarray(oi[:, 0]), np.ascontiguousarray(os_[:, 0])


# ---- 1. the three scenes against the filtered definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scenes_against_the_reference(eng, orc, ctx, dtype, n):
    import torch
    c = case(orc, dtype, n)
    M, R = inst_masks(n), ray_masks(n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        assert inst.set_masks(M) is inst
        rb, rd, Rd = _rb(eng, c["rays"]), _dev_rays(eng, c["rays"]), _dev_mask(R)
        for cut in (False, True):
            w = masked_want(orc, dtype, n, cut)
            tm = c["tmax"] if cut else None
            td = torch.from_numpy(c["tmax"]).cuda() if cut else None
            occ = w["first"][1] != NONE
            for where, rays, rm, t in (("host", rb, R, tm), ("device", rd, Rd, td)):
                _trace_same(inst.closest_hits_masked(rays, rm, t), w["closest"], (n, cut, where, "closest"))
                _trace_same(inst.any_hits_masked(rays, rm, t), w["first"], (n, cut, where, "first"))
                assert np.array_equal(_np(inst.occluded_masked(rays, rm, t)), occ), (n, cut, where, "occluded")
                for k in KS:
                    _khits_same(inst.khits_masked_batch(rays, k, rm, t), w["khits"][k], (n, cut, where, k))
                _csr_same(inst.allhits_masked_batch(rays, rm, t), w["sorted"], (n, cut, where, "sorted"))
                _csr_same(inst.allhits_masked_batch(rays, rm, t, sort=False), w["listed"], (n, cut, where, "list order"))
                _csr_same(inst.allhits_masked_batch(rays, rm, t, count_only=True), w["sorted"][:1], (n, cut, where, "count"))
                _csr_same(inst.allhits_masked_batch(rays, rm, t, sort=False, count_only=True), w["listed"][:1], (n, cut, where, "count, list order"))
        assert inst._hits.walk_kernel().startswith("bvhgpu::k_instances_allhits_count<") and inst._hits.walk_kernel().endswith(", true>")
        got = inst.closest_hits_masked(rd, Rd)
        assert got[1].device == rd.device.device and got[1].dtype == torch.int32


# ---- 2. the anchor: the engine's own unmasked rows, filtered ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_rows_are_the_unmasked_rows_filtered(eng, orc, ctx, dtype, n):
    c = case(orc, dtype, n)
    M, R = inst_masks(n), ray_masks(n)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rb = _rb(eng, c["rays"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        inst.set_masks(M)
        for tm in (None, c["tmax"]):
            srt = _filter_csr(inst.allhits_batch(rb, tm, sort=True), M, R, N_RAYS)           # (the unmasked entry ignores the masks)
            lst = _filter_csr(inst.allhits_batch(rb, tm, sort=False), M, R, N_RAYS)
            if n == 37 and tm is None:
                assert 0 < int(srt[0][-1]) == 1585
            _csr_same(inst.allhits_masked_batch(rb, R, tm, sort=True), srt, (n, "sorted"))
            _csr_same(inst.allhits_masked_batch(rb, R, tm, sort=False), lst, (n, "list order"))
            _trace_same(inst.closest_hits_masked(rb, R, tm), _heads(srt, N_RAYS, dtype), (n, "closest"))
            _trace_same(inst.any_hits_masked(rb, R, tm), _heads(lst, N_RAYS, dtype), (n, "first"))
            for k in KS:
                _khits_same(inst.khits_masked_batch(rb, k, R, tm), ikh.cut_rows(srt, N_RAYS, k, dtype), (n, k))


# ---- 3. all ones: every masked entry is its unmasked counterpart ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_ones_is_the_unmasked_entry(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        assert (inst.masks == ALL).all() and inst.masks.dtype == np.uint32 and inst.masks.shape == (37,)

        def identical(label):
            for rays, tm in ((_rb(eng, c["rays"]), c["tmax"]), (_dev_rays(eng, c["rays"]), None)):
                _trace_same(inst.closest_hits_masked(rays, None, tm), [_np(x, i) for x, i in zip(inst.closest_hits(rays, tm), (0, 1, 1))], label)
                _trace_same(inst.any_hits_masked(rays, None, tm), [_np(x, i) for x, i in zip(inst.any_hits(rays, tm), (0, 1, 1))], label)
                assert np.array_equal(_np(inst.occluded_masked(rays, None, tm)), _np(inst.occluded(rays, tm))), label
                for k in (1, 9, 64):
                    _khits_same(inst.khits_masked_batch(rays, k, None, tm), [_np(x, i) for x, i in zip(inst.khits_batch(rays, k, tm), (1, 1, 0))], (label, k))
                for so in (True, False):
                    for co in (False, True):
                        _csr_same(inst.allhits_masked_batch(rays, None, tm, so, co), _csr(inst.allhits_batch(rays, tm, so, co)), (label, so, co))
        identical("new set")
        assert (inst.closest_hits(_rb(eng, c["rays"]))[1] != NONE).sum() >= 100
        inst.set_masks(inst_masks(37))
        got = inst.closest_hits_masked(_rb(eng, c["rays"]), None)                 # (ray masks all ones: only instance 5 is hidden)
        want = imr.closest(c["free"]["table"], inst_masks(37), None, N_RAYS, None, dtype)
        _trace_same(got, want, "instance masks, no ray mask")
        assert (want[1] != c["free"]["closest"][1]).sum() >= 1
        inst.set_masks(None)
        assert (inst.masks == ALL).all()
        identical("after set_masks(None)")


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges(eng, orc, ctx, dtype):
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    n = 130
    rays = np.ascontiguousarray(c["rays"][150:150 + n])
    rb, rd = _rb(eng, rays), _dev_rays(eng, rays)
    miss = (np.concatenate([np.full((n, 1), np.inf), np.zeros((n, 2))], axis=1).astype(dtype), np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32))
    empty_csr = (np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), dtype))

    def nothing(inst, rm, rm_dev, label):
        for r, m in ((rb, rm), (rd, rm_dev)):
            _trace_same(inst.closest_hits_masked(r, m), miss, label)
            _trace_same(inst.any_hits_masked(r, m), miss, label)
            assert not _np(inst.occluded_masked(r, m)).any(), label
            for k in (1, 5, 64):
                _khits_same(inst.khits_masked_batch(r, k, m), ikh.padding(n, k, dtype), (label, k))
            for so in (True, False):
                _csr_same(inst.allhits_masked_batch(r, m, None, so), empty_csr, (label, so))
                _csr_same(inst.allhits_masked_batch(r, m, None, so, True), empty_csr[:1], (label, so, "count"))

    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        assert (inst.closest_hits(rb)[1] != NONE).sum() >= 50                        # these rays do hit
        inst.set_masks(np.zeros(37, np.uint32))
        nothing(inst, None, None, "all instance masks 0")
        nothing(inst, ALL, ALL, "all instance masks 0, scalar ray mask")
        inst.set_masks(inst_masks(37))
        nothing(inst, np.zeros(n, np.uint32), _dev_mask(np.zeros(n, np.uint32)), "all ray masks 0")
        nothing(inst, 0, 0, "scalar ray mask 0")
        # a scalar is every ray's mask
        table = c["free"]["table"]
        for scalar in (HIGH, 5, ALL):
            R = np.full(N_RAYS, scalar, np.uint32)
            want = tuple(x[150:150 + n] for x in imr.closest(table, inst_masks(37), R, N_RAYS, None, dtype))
            assert (want[1] != NONE).sum() >= 5
            for r in (rb, rd):
                _trace_same(inst.closest_hits_masked(r, scalar), want, ("scalar", scalar))
                _trace_same(inst.closest_hits_masked(r, np.full(n, scalar, np.uint32) if r is rb else _dev_mask(np.full(n, scalar, np.uint32))), want, ("array", scalar))
                _khits_same(inst.khits_masked_batch(r, 3, scalar), tuple(x[150:150 + n] for x in imr.khits(table, inst_masks(37), R, N_RAYS, None, 3, dtype)), ("khits", scalar))
            got = _csr(inst.allhits_masked_batch(rb, scalar))
            full = imr.allhits(table, inst_masks(37), R, N_RAYS, None, dtype)
            lo, hi = int(full[0][150]), int(full[0][150 + n])
            assert got[0].tobytes() == (full[0][150:150 + n + 1] - full[0][150]).astype(np.uint32).tobytes()
            assert got[1].tobytes() == full[1][lo:hi].tobytes() and got[2].tobytes() == full[2][lo:hi].tobytes() and got[3].tobytes() == full[3][lo:hi].tobytes()
        # no rays
        for r, m in ((_rb(eng, rays[:0]), np.zeros(0, np.uint32)), (_dev_rays(eng, rays[:0]), _dev_mask(np.zeros(0, np.uint32))), (_rb(eng, rays[:0]), None), (_rb(eng, rays[:0]), 3)):
            v, i, s = inst.closest_hits_masked(r, m)
            assert tuple(v.shape) == (0, 3) and tuple(i.shape) == (0,)
            gi, gs, gv = inst.khits_masked_batch(r, 3, m)
            assert tuple(gi.shape) == (0, 3) and tuple(gv.shape) == (0, 3, 3)
            got = inst.allhits_masked_batch(r, m)
            assert _csr(got)[0].tolist() == [0] and tuple(got["vals"].shape) == (0, 3)
    # the one instance of the 1-instance set hidden, then shown again
    c1 = case(orc, dtype, 1)
    t1 = _gpu_trees(eng, ctx, c1["trees"])
    r1 = np.ascontiguousarray(c1["rays"][150:150 + n])
    with eng.Instances(t1, c1["tree_of"], c1["x"], ctx) as one:
        rb, rd = _rb(eng, r1), _dev_rays(eng, r1)
        assert (one.closest_hits(rb)[1] != NONE).sum() >= 5
        one.set_masks([0])
        nothing(one, None, None, "the single instance hidden")
        one.set_masks([4])
        nothing(one, 3, 3, "the single instance hidden from these rays")
        _trace_same(one.closest_hits_masked(rb, 6), one.closest_hits(rb), "the single instance shown")
    # a set without instances
    with eng.Instances(trees, np.zeros(0, np.uint32), np.zeros((0, 3, 4), dtype), ctx) as none:
        rb, rd = _rb(eng, rays), _dev_rays(eng, rays)
        assert none.masks.shape == (0,) and none.set_masks(None) is none and none.set_masks(np.zeros(0, np.uint32)) is none
        nothing(none, None, None, "no instances")
        nothing(none, np.full(n, 5, np.uint32), _dev_mask(np.full(n, 5, np.uint32)), "no instances, ray masks")


# ---- 5. the masks' lifetime -------------------------------------------------------------------------------------------------------------------
def test_lifetime(eng, orc, ctx):
    import torch
    from bvh_amd import BvhGpuError
    from bvh_amd._lib import INVALID_ARG
    dtype = np.float32
    trees = member_trees(orc, dtype)
    (a_aabbs, a_tris), (b_aabbs, b_tris) = trees[0], trees[1]
    member = eng.Bvh.from_aabbs(a_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(a_tris)
    ni = 9
    x = transforms(ni, dtype, 31)
    nr = 2000
    rays = cluster_rays(orc, nr, dtype, 32)
    rb = _rb(eng, rays)
    M = inst_masks(ni)
    R = np.tile(ray_masks(ni), 2)[:nr]

    def ref(tr, xf):
        t = ir.Scene([tr], [0] * ni, xf, dtype).trace(rays)["table"]
        return imr.closest(t, M, R, nr, None, dtype), imr.allhits(t, M, R, nr, None, dtype), imr.closest(t, np.full(ni, ALL, np.uint32), None, nr, None, dtype)

    with eng.Instances([member], [0] * ni, x, ctx) as inst:
        inst.set_masks(M)
        assert inst.masks.tobytes() == M.tobytes()
        inst.set_masks(torch.from_numpy(M.view(np.int32).copy()).cuda())             # from HBM: the same bits
        assert inst.masks.tobytes() == M.tobytes()
        cl, ah, free = ref(trees[0], x)
        assert (cl[1] != free[1]).sum() >= 20 and (cl[1] != NONE).sum() >= 20
        _trace_same(inst.closest_hits_masked(rb, R), cl, "before")
        # a re-pose keeps the masks: the reference at the new pose, under the same masks
        x2 = transforms(ni, dtype, 999)
        inst.update(x2)
        assert inst.masks.tobytes() == M.tobytes()
        cl2, ah2, free2 = ref(trees[0], x2)
        assert cl2[1].tobytes() != cl[1].tobytes() and (cl2[1] != free2[1]).sum() >= 20
        _trace_same(inst.closest_hits_masked(rb, R), cl2, "re-posed")
        _csr_same(inst.allhits_masked_batch(rb, R), ah2, "re-posed, all hits")
        _trace_same(inst.closest_hits(rb), free2, "re-posed, the unmasked entry")
        # a failed update: the set refuses as uncommitted, and still takes masks
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        M2 = np.roll(M, 1)
        assert inst.set_masks(M2) is inst and inst.masks.tobytes() == M2.tobytes()
        for call in (lambda: inst.closest_hits_masked(rb, R), lambda: inst.any_hits_masked(rb, R), lambda: inst.khits_masked_batch(rb, 3, R),
                     lambda: inst.allhits_masked_batch(rb, R)):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == INVALID_ARG and "not committed" in str(e.value)
        inst.update(x2)
        t2 = ir.Scene([trees[0]], [0] * ni, x2, dtype).trace(rays)["table"]
        _trace_same(inst.closest_hits_masked(rb, R), imr.closest(t2, M2, R, nr, None, dtype), "the masks set while uncommitted")
        inst.set_masks(M)
        # a stale member: refused like the unmasked entries, and the masks can still be set
        member.rebuild(b_aabbs[:100], flatten=True)
        for call in (lambda: inst.closest_hits_masked(rb, R), lambda: inst.khits_masked_batch(rb, 3, R), lambda: inst.allhits_masked_batch(rb, R),
                     lambda: inst.closest_hits(rb)):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        assert inst.set_masks(M2) is inst and inst.masks.tobytes() == M2.tobytes()
        member.set_triangles(b_tris[:100])
        inst.update(x2)
        t3 = ir.Scene([(b_aabbs[:100], b_tris[:100])], [0] * ni, x2, dtype).trace(rays)["table"]
        want = imr.closest(t3, M2, R, nr, None, dtype)
        assert (want[1] != NONE).sum() >= 20
        _trace_same(inst.closest_hits_masked(rb, R), want, "the new generation")


# ---- 6. the refusals of the raw C ABI ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype, k, n = np.float32, 5, 64
    c = case(orc, dtype, 37)
    trees = _gpu_trees(eng, ctx, c["trees"])
    rays = np.ascontiguousarray(c["rays"][150:214])
    rays64 = np.ascontiguousarray(case(orc, np.float64, 37)["rays"][150:214])
    M, R = inst_masks(37), np.ascontiguousarray(ray_masks(37)[150:214])
    SENT = 0xABABABAB
    ov, oi, os_ = np.full((n, 64, 3), 7.0, dtype), np.full((n, 64), SENT, np.uint32), np.full((n, 64), SENT, np.uint32)
    ov64 = np.full((n, 64, 3), 7.0, np.float64)
    om = np.full(37, SENT, np.uint32)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def untouched():
        assert (ov == 7.0).all() and (oi == SENT).all() and (os_ == SENT).all() and (ov64 == 7.0).all() and (om == SENT).all()

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
        inst.set_masks(M)
        s, S, B = inst._s, stale._s, broken._s
        Rp, Mp, V, I, Sh, V64 = ptr(rays), ptr(R), ptr(ov), ptr(oi), ptr(os_), ptr(ov64)
        R64 = ptr(rays64)

        def both(plain, masked, args, status, text):
            """the unmasked entry and its masked form (ray_mask after tmax) refuse alike: status, message, nothing written"""
            rc0 = plain(*args)
            e0 = err()
            rc1 = masked(*args[:3], Mp, *args[3:])
            assert rc0 == rc1 == status and err() == e0 and text in e0, (rc0, rc1, e0, err())
            assert masked(*args[:3], None, *args[3:]) == status and err() == e0
            untouched()

        # ---- trace: a NULL set; a NULL argument; mem; dtype; flags; uncommitted; stale; the batch size ----
        t32, t64 = lib.bvhgpu_instances_trace_f32, lib.bvhgpu_instances_trace_f64
        m32, m64 = lib.bvhgpu_instances_trace_masked_f32, lib.bvhgpu_instances_trace_masked_f64
        assert m32(None, Rp, None, Mp, n, HOST, 0, V, I, Sh) == INVALID_ARG == t32(None, Rp, None, n, HOST, 0, V, I, Sh)
        untouched()
        UNC, STALE = "instances are not committed", "instances are stale: call bvhgpu_instances_update"
        for args, status, text in (
                ((s, None, None, n, HOST, 0, V, I, Sh), INVALID_ARG, "NULL argument"), ((s, Rp, None, n, HOST, 0, None, I, Sh), INVALID_ARG, "NULL argument"),
                ((s, Rp, None, n, HOST, 0, V, None, Sh), INVALID_ARG, "NULL argument"), ((s, Rp, None, n, HOST, 0, V, I, None), INVALID_ARG, "NULL argument"),
                ((s, Rp, None, n, 7, 0, V, I, Sh), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                ((s, Rp, None, n, HOST, 2, V, I, Sh), INVALID_ARG, "instance trace flags"), ((s, Rp, None, n, HOST, 1 << 31, V, I, Sh), INVALID_ARG, "instance trace flags"),
                ((B, Rp, None, n, HOST, 0, V, I, Sh), INVALID_ARG, UNC), ((S, Rp, None, n, HOST, 0, V, I, Sh), INVALID_ARG, STALE),
                ((s, Rp, None, 0xFFFFFFFF, HOST, 0, V, I, Sh), OVERFLOW, "2^32-2 rays"),
                # the order: an earlier rule wins over a later one
                ((S, None, None, 0xFFFFFFFF, 7, 2, V, I, Sh), INVALID_ARG, "NULL argument"), ((S, Rp, None, 0xFFFFFFFF, 7, 2, V, I, Sh), INVALID_ARG, "mem must be"),
                ((S, Rp, None, 0xFFFFFFFF, HOST, 2, V, I, Sh), INVALID_ARG, "instance trace flags"), ((B, Rp, None, 0xFFFFFFFF, HOST, 0, V, I, Sh), INVALID_ARG, UNC),
                ((S, Rp, None, 0xFFFFFFFF, HOST, 0, V, I, Sh), INVALID_ARG, STALE)):
            both(t32, m32, args, status, text)
        both(t64, m64, (s, R64, None, n, HOST, 0, V64, I, Sh), DTYPE_MISMATCH, "instance set dtype differs from ray dtype")
        both(t64, m64, (S, R64, None, 0xFFFFFFFF, HOST, 2, V64, I, Sh), DTYPE_MISMATCH, "dtype")
        assert m32(s, None, None, None, 0, HOST, 0, None, None, None) == OK
        # ---- khits: a NULL set; k; a NULL argument; mem; dtype; uncommitted; stale; the size ----
        k32, k64 = lib.bvhgpu_instances_khits_f32, lib.bvhgpu_instances_khits_f64
        km32, km64 = lib.bvhgpu_instances_khits_masked_f32, lib.bvhgpu_instances_khits_masked_f64
        assert km32(None, Rp, None, Mp, n, HOST, k, I, Sh, V) == INVALID_ARG
        untouched()
        for args, status, text in (
                ((s, Rp, None, n, HOST, 0, I, Sh, V), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KHITS_MAX_K"),
                ((s, Rp, None, n, HOST, 65, I, Sh, V), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KHITS_MAX_K"),
                ((s, Rp, None, n, HOST, 0xFFFFFFFF, I, Sh, V), INVALID_ARG, "k must be"),
                ((s, None, None, n, HOST, k, I, Sh, V), INVALID_ARG, "NULL argument"), ((s, Rp, None, n, HOST, k, None, Sh, V), INVALID_ARG, "NULL argument"),
                ((s, Rp, None, n, HOST, k, I, None, V), INVALID_ARG, "NULL argument"), ((s, Rp, None, n, HOST, k, I, Sh, None), INVALID_ARG, "NULL argument"),
                ((s, Rp, None, n, 7, k, I, Sh, V), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                ((B, Rp, None, n, HOST, k, I, Sh, V), INVALID_ARG, UNC), ((S, Rp, None, n, HOST, k, I, Sh, V), INVALID_ARG, STALE),
                ((s, Rp, None, 1 << 26, HOST, 64, I, Sh, V), OVERFLOW, "too many results (rays x k)"),
                ((s, Rp, None, 0xFFFFFFFF, HOST, 1, I, Sh, V), OVERFLOW, "too many results (rays x k)"),
                ((S, None, None, 0xFFFFFFFF, 7, 0, I, Sh, V), INVALID_ARG, "k must be"), ((S, None, None, 0xFFFFFFFF, 7, k, I, Sh, V), INVALID_ARG, "NULL argument"),
                ((S, Rp, None, 0xFFFFFFFF, 7, k, I, Sh, V), INVALID_ARG, "mem must be"), ((B, Rp, None, 0xFFFFFFFF, HOST, k, I, Sh, V), INVALID_ARG, UNC),
                ((S, Rp, None, 0xFFFFFFFF, HOST, k, I, Sh, V), INVALID_ARG, STALE)):
            both(k32, km32, args, status, text)
        both(k64, km64, (s, R64, None, n, HOST, k, I, Sh, V64), DTYPE_MISMATCH, "instance set dtype differs from ray dtype")
        assert km32(s, None, None, None, 0, HOST, k, None, None, None) == OK
        # ---- allhits: a NULL set; a NULL hits; NULL rays; mem; dtype; flags; uncommitted; stale; the batch size.  *hits stays as it was ----
        a32, a64 = lib.bvhgpu_instances_allhits_f32, lib.bvhgpu_instances_allhits_f64
        am32, am64 = lib.bvhgpu_instances_allhits_masked_f32, lib.bvhgpu_instances_allhits_masked_f64
        h = C.c_void_p()
        assert am32(None, Rp, None, Mp, n, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        both(a32, am32, (s, Rp, None, n, HOST, 0, None), INVALID_ARG, "hits is NULL")
        for keep in (None, "made"):
            if keep:
                assert am32(s, Rp, None, Mp, n, HOST, 0, C.byref(h)) == OK and h.value
                keep = h.value
            for args, status, text in (
                    ((s, None, None, n, HOST, 0, C.byref(h)), INVALID_ARG, "rays is NULL"), ((s, Rp, None, n, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                    ((s, Rp, None, n, HOST, 4, C.byref(h)), INVALID_ARG, "instance all-hits flags"), ((s, Rp, None, n, HOST, 3 | 16, C.byref(h)), INVALID_ARG, "instance all-hits flags"),
                    ((B, Rp, None, n, HOST, 0, C.byref(h)), INVALID_ARG, UNC), ((S, Rp, None, n, HOST, 0, C.byref(h)), INVALID_ARG, STALE),
                    ((s, Rp, None, 0xFFFFFFFF, HOST, 0, C.byref(h)), OVERFLOW, "2^32-2 rays"),
                    ((S, None, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "rays is NULL"), ((S, Rp, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "mem must be"),
                    ((S, Rp, None, 0xFFFFFFFF, HOST, 8, C.byref(h)), INVALID_ARG, "instance all-hits flags"), ((B, Rp, None, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, UNC),
                    ((S, Rp, None, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, STALE)):
                both(a32, am32, args, status, text)
                assert h.value == keep
            both(a64, am64, (s, R64, None, n, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "instance set dtype differs from ray dtype")
            assert h.value == keep
        # the result object a refused batch left alone still holds the masked batch made before: read by the unmasked family's fetch
        want = imr.allhits(c["free"]["table"], M, ray_masks(37), N_RAYS, None, dtype)
        lo, hi = int(want[0][150]), int(want[0][214])
        nr, tot = C.c_size_t(), C.c_uint64()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (n, hi - lo) and hi - lo >= 20
        off, gi, gs, gv = np.zeros(n + 1, np.uint32), np.zeros(hi - lo, np.uint32), np.zeros(hi - lo, np.uint32), np.zeros((hi - lo, 3), dtype)
        assert lib.bvhgpu_hits_fetch_instances_allhits(h, ptr(off), ptr(gi), ptr(gs), ptr(gv), HOST) == OK
        assert off.tobytes() == (want[0][150:215] - want[0][150]).astype(np.uint32).tobytes()
        assert gi.tobytes() == want[1][lo:hi].tobytes() and gs.tobytes() == want[2][lo:hi].tobytes() and gv.tobytes() == want[3][lo:hi].tobytes()
        assert lib.bvhgpu_hits_fetch_allhits(h, ptr(off), ptr(gs), ptr(gv), HOST) == INVALID_ARG        # (not a single-tree all-hits result)
        lib.bvhgpu_hits_destroy(h)
        # ---- set_masks and masks ----
        sm, gm = lib.bvhgpu_instances_set_masks, lib.bvhgpu_instances_masks
        assert sm(None, ptr(M), 37, HOST) == INVALID_ARG and gm(None, ptr(om), HOST) == INVALID_ARG
        for args, text in (((s, ptr(M), 37, 7), "set_masks: mem must be BVHGPU_HOST or BVHGPU_DEVICE"), ((s, None, 37, 7), "set_masks: mem must be"),
                           ((s, ptr(M), 36, HOST), "set_masks: the number of masks differs from the set's number of instances"),
                           ((s, ptr(M), 38, HOST), "set_masks: the number of masks differs"), ((s, None, 0, HOST), "set_masks: the number of masks differs"),
                           ((s, ptr(M), 0, DEVICE), "set_masks: the number of masks differs"), ((s, ptr(M), 38, 7), "set_masks: mem must be")):
            assert sm(*args) == INVALID_ARG and text in err(), (args, err())
            assert inst.masks.tobytes() == M.tobytes()                               # the set's masks are what they were
        assert gm(s, None, HOST) == INVALID_ARG and "out is NULL" in err()
        assert gm(s, ptr(om), 7) == INVALID_ARG and "mem must be BVHGPU_HOST or BVHGPU_DEVICE" in err()
        untouched()
        assert sm(B, ptr(M), 37, HOST) == OK and gm(B, ptr(om), HOST) == OK and om.tobytes() == M.tobytes()      # an uncommitted set takes and shows masks
        assert sm(S, ptr(M), 37, HOST) == OK                                                                     # ... and so does a stale one
        om[:] = SENT
        # a later valid call still answers, on the set that refused
        gv, gi, gs = np.zeros((n, 3), dtype), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        assert m32(s, Rp, None, Mp, n, HOST, 0, ptr(gv), ptr(gi), ptr(gs)) == OK
        want = tuple(x[150:214] for x in masked_want(orc, dtype, 37, False)["closest"])
        assert (want[1] != NONE).sum() >= 20
        _trace_same((gv, gi, gs), want, "after the refusals")
        untouched()
