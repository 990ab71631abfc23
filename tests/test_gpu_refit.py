"""bvhgpu_refit_* end to end.  Refit rewrites every array the walks read — the BvhNode boxes, the tree's own copy of the shape AABBs and,
through the re-flatten, flat / trav / wide / the guide boxes / the LDS slot tables — and clears exact_only.  Here it runs on the trees that
exercise every builder tier (tests/test_refit_cpu.py: identical centroids, the deep tree, the overflow band, ragged sizes, signed zeros),
twice per tree, and afterwards every array and every consumer is compared with the references the suite already has, bit for bit: the
oracle's refit (pinned by test_refit_cpu.py) for the arrays, the oracle's walks and the Python restatements for the queries.  Also: the walk
a tree with empty child boxes gets after its first refit (exact_only), a batch in flight when the refit arrives, the error returns, and the
input contract — NaN / ±inf is answered with INVALID_ARG and the tree stays byte for byte what it was."""
import functools

import numpy as np
import pytest

import knn_ref as kr
import knn_tree_ref as ktr
import query_ref as qr
from test_fp_extremes_cpu import same
from test_gpu_any_hit import first_match
from test_refit_cpu import SCENES, has_empty_child, moved, scene

pytestmark = pytest.mark.gpu

N_RAYS, N_POINTS, N_KNN, N_QUERIES = 1500, 300, 60, 150
KS = (1, 5)
CASES = [(name, dt) for name in SCENES for dt in (np.float32, np.float64) if not (name == "deep" and dt == np.float64)]
CASE_IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in CASES]


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


def _rb(eng, rays):
    return eng.RayBatch(len(rays), np.float32 if rays.dtype.itemsize == 36 else np.float64, host=np.ascontiguousarray(rays))


def _tris_of(aabbs):
    """one triangle per box whose AABB is the box: [min, max, (min.x, max.y, min.z)]"""
    lo, hi = aabbs[:, :3], aabbs[:, 3:]
    return np.ascontiguousarray(np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], axis=1)], axis=1))


def _bounds(a, sc):
    lo, hi = a[:, :3].min(axis=0).astype(np.float64), a[:, 3:].max(axis=0).astype(np.float64)
    ext = np.maximum(hi - lo, sc)
    return lo - 0.25 * ext, hi + 0.25 * ext


def _rays(orc, a, sc, m, dtype, seed):
    """rays from around the scene aimed at (moved) shapes, a fifth in random directions, some parallel to an axis"""
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(a, sc)
    o = rng.uniform(lo, hi, size=(m, 3)).astype(dtype)
    tgt = a[rng.integers(0, len(a), m)].astype(np.float64).reshape(m, 2, 3).mean(axis=1)
    d = tgt - o.astype(np.float64)
    d[: m // 5] = rng.normal(size=(m // 5, 3))
    d[m // 5: m // 4] = rng.integers(-1, 2, size=(m // 4 - m // 5, 3))
    d[np.all(d == 0, axis=1)] = [1, 0, 0]
    d /= np.abs(d).max(axis=1, keepdims=True)                  # (Ray::new squares the components: keep them representable)
    return orc.make_rays(o, d.astype(dtype), dtype)


def _crossing_rays(orc, a, m, dtype, seed):
    """rays across the chain of the deep scene where its boxes stand apart (from shape 1300 on the spacing, 0.004 x, exceeds 0.7 and the
    boxes are 0.5 wide): each comes from below one box, stays within 0.1 of the middle of that box's x range while it is between the planes
    y = 0 and y = 0.5 that hold every box, and so meets that one shape and, in every node above it, the one child box that holds it — the
    other boxes are more than 0.3 away in x.  No step of the wide walk finds a second grandchild to push, whatever the depth of the tree."""
    rng = np.random.default_rng(seed)
    b = a[rng.integers(1300, 3000, m)].astype(np.float64)
    u = rng.uniform(0.02, 0.1, size=(m, 2)) * rng.choice([-1.0, 1.0], size=(m, 2))
    mid = (b[:, :3] + b[:, 3:]) * 0.5
    o = np.stack([mid[:, 0] + u[:, 0], np.full(m, -4.0), mid[:, 2] + u[:, 1]], axis=1).astype(dtype)
    d = mid - o.astype(np.float64)
    d /= np.abs(d).max(axis=1, keepdims=True)
    return orc.make_rays(o, d.astype(dtype), dtype)


def _points(a, sc, m, dtype, seed):
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(a, sc)
    p = rng.uniform(lo, hi, size=(m, 3))
    b = a[rng.integers(0, len(a), m // 2)].astype(np.float64)
    p[: m // 2] = (b[:, :3] + b[:, 3:]) * 0.5 + rng.normal(size=(m // 2, 3)) * sc
    return p.astype(dtype)


class _Step:
    """one refit of a case: the moved boxes and triangles, and the oracle's tree after it"""

    def __init__(self, orc, name, a0, sc, dtype, nodes_before, seed):
        self.aabbs, shift = moved(name, a0, sc, dtype, seed)
        self.tris = np.ascontiguousarray(_tris_of(a0) + shift)
        self.nodes = orc.refit(nodes_before, self.aabbs)
        self.flat = orc.flatten(self.nodes)
        self.rays = _rays(orc, self.aabbs, sc, N_RAYS, dtype, seed + 100)
        self.off, self.idx, self.ts, _ = orc.traverse_flat(self.flat, self.aabbs, self.rays, want_t=True)
        self.oisect, self.oclosest, self.oprim = orc.triangle_stage(self.tris, self.rays, self.off, self.idx)


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """built once per scene and dtype, shared by the tests, never written to"""
    from oracle import orc
    a0, sc = scene(name, dtype)
    a0 = np.ascontiguousarray(a0)
    built = orc.build(a0)
    s1 = _Step(orc, name, a0, sc, dtype, built.nodes, 41)
    s2 = _Step(orc, name, a0, sc, dtype, s1.nodes, 42)
    return dict(name=name, dtype=dtype, a0=a0, sc=sc, built=built, steps=(s1, s2))


def _wide_ctx(eng):
    from bvh_amd import Context
    from bvh_amd._lib import TUNE_TRAVERSE_LDS_MIN_RAYS
    ctx = Context(0)
    ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)              # the wide walk takes the small batch
    return ctx


def _device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _check_arrays(orc, bvh, flat, step, built, label):
    assert bvh.nodes.tobytes() == step.nodes.tobytes(), label
    assert orc.check_tree(bvh.nodes, step.aabbs) == 0, label
    assert np.array_equal(bvh.shape_nodes, built.shape_node), label
    assert flat.nodes.tobytes() == step.flat.tobytes(), label


# ---- a. the arrays ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_arrays_after_each_refit(eng, orc, name, dtype):
    """BvhNode array == the oracle's refit of the oracle's tree, consistent and tight, shape → node map untouched, FlatNode array == the
    oracle's flatten of that tree — for a tree that was flattened before the refit and for one whose first flatten() comes after it, for
    numpy input and for a tensor in HBM, after the first refit and after a second one on the same tree."""
    from bvh_amd import Context
    c = _case(name, dtype)
    before = eng.Bvh.from_aabbs(c["a0"], Context(0))
    flat_before = before.flatten()
    after = eng.Bvh.from_aabbs(c["a0"], Context(0))                 # not flattened yet
    dev = eng.Bvh.from_aabbs(c["a0"], Context(0))
    flat_dev = dev.flatten()
    assert before.nodes.tobytes() == c["built"].nodes.tobytes()
    flat_after = None
    for k, step in enumerate(c["steps"]):
        before.refit(step.aabbs)
        after.refit(step.aabbs)
        keep = _device(step.aabbs)
        dev.refit(keep)
        if flat_after is None:
            flat_after = after.flatten()
        _check_arrays(orc, before, flat_before, step, c["built"], ("flattened before", k))
        _check_arrays(orc, after, flat_after, step, c["built"], ("flattened after", k))
        _check_arrays(orc, dev, flat_dev, step, c["built"], ("device input", k))
        off, idx, _, _ = flat_after.traverse_batch(_rb(eng, step.rays))
        assert np.array_equal(off, step.off) and np.array_equal(idx, step.idx), k
    for t in (before, after, dev):
        t.close()


# ---- b. every consumer ----------------------------------------------------------------------------------------------------------
def _t_slices(eng, flat, step, label):
    off, idx, ts, st = flat.traverse_batch(_rb(eng, step.rays), want_t=True)
    assert np.array_equal(off, step.off) and np.array_equal(idx, step.idx), label
    if len(idx):
        assert same(ts, step.ts), label
    return st


def _ray_consumers(eng, orc, flat, step, dtype, ordered, tmax, want_any, label, full):
    rb = _rb(eng, step.rays)
    off, idx, _, st = flat.traverse_batch(rb)
    assert np.array_equal(off, step.off) and np.array_equal(idx, step.idx), label
    _, _, isect, _ = flat.intersect_triangles(rb)
    cl, prim, _ = flat.closest_hits(rb)
    assert same(isect, step.oisect) and same(cl, step.oclosest) and np.array_equal(prim, step.oprim), label
    isect_a, shape_a = flat.any_hits(rb, tmax)
    assert same(isect_a, want_any[0]) and np.array_equal(shape_a, want_any[1]), label
    if not full:
        return st
    _t_slices(eng, flat, step, label)
    if ordered:
        for order, asc in (("nearest", True), ("farthest", False)):
            noff, nidx, _, _ = flat.traverse_batch(rb, order=order)
            qoff, qidx = orc.traverse_child_ordered(step.nodes, step.aabbs, step.rays, asc)
            assert np.array_equal(noff, qoff) and np.array_equal(nidx, qidx), (label, order)
    if len(step.aabbs) >= 2:
        for order, asc in (("nearest_heap", True), ("farthest_heap", False)):
            noff, nidx, _, _ = flat.traverse_batch(rb, order=order)
            qoff, qidx = orc.traverse_distance(step.nodes, step.aabbs, step.rays, asc)
            assert np.array_equal(noff, qoff) and np.array_equal(nidx, qidx), (label, order)
    return st


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_every_consumer_on_the_refitted_tree(eng, orc, name, dtype):
    from bvh_amd import Context, FlatBvh
    from bvh_amd._lib import TUNE_QUERY_VARIANT, TUNE_WIDE_F64_GUIDE, TUNE_WIDE_ITEMS_LOG4
    c = _case(name, dtype)
    sc, n = c["sc"], len(c["a0"])
    rng = np.random.default_rng(7)
    ctx, wctx = Context(0), _wide_ctx(eng)
    bvh, wbvh = eng.Bvh.from_aabbs(c["a0"], ctx), eng.Bvh.from_aabbs(c["a0"], wctx)
    flat, wflat = bvh.flatten(), wbvh.flatten()
    depth = orc.tree_stats(c["built"].nodes, c["a0"])["max_depth"]
    ordered = depth < 31                                                        # the child-ordered iterator's stack (as in the fuzz test)
    # The wide walk visits two binary levels per step, pushes at most 3 entries per step and gives a lane WIDE_STACK entries at the least
    # (walk_wide.hip: WideGeom's 6 in LDS for rays cut into items, WIDE_GSTACK = 24 in HBM; the engine reports no replay, so the figures
    # are restated here and noted beside WIDE_GSTACK).  Up to this depth no lane can outgrow them, so the batch stays with the wide walk;
    # on a deeper tree (the deep scene) a lane may, and the engine then answers the batch again with the binary walk.
    WIDE_STACK = 6 + 24
    stays_wide = n >= 64 and 3 * ((depth + 1) // 2) <= WIDE_STACK
    for k, step in enumerate(c["steps"]):
        bvh.refit(step.aabbs); wbvh.refit(step.aabbs)
        flat.set_triangles(step.tris); wflat.set_triangles(step.tris)           # the caller's to refresh
        cd = step.oclosest[:, 0].astype(np.float64)
        tmax = (np.where(np.isfinite(cd), cd, 200.0 * sc) * rng.uniform(0.3, 1.7, size=len(cd))).astype(dtype)
        want_any = first_match(step.off, step.idx, step.oisect, tmax)
        # rays: the default context, then the wide walk on the small batch with whole rays and with 16 items per ray (f64: over the f32
        # guide boxes and over the f64 boxes)
        _ray_consumers(eng, orc, flat, step, dtype, ordered, tmax, want_any, ("default", k), full=True)
        for items in (0, 2):
            for guide in ((1, 0) if dtype == np.float64 else (None,)):
                wctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, items)
                if guide is not None:
                    wctx.set_tuning(TUNE_WIDE_F64_GUIDE, guide)
                st = _ray_consumers(eng, orc, wflat, step, dtype, ordered, tmax, want_any, ("wide", k, items, guide), full=False)
                if stays_wide:
                    assert "k_traverse_wide" in st["kernel"], st["kernel"]     # a refitted tree has no empty child box: the wide walk may run
        # t-slices are not the wide walk's: on this context they go to the persistent binary walk, whose LDS top is read through the
        # slot tables (slot_entry / node_slot) that the re-flatten rewrote (the four orders take one kernel whatever the context)
        st = _t_slices(eng, wflat, step, ("wide ctx, t-slices", k))
        if n >= 64:
            assert "k_traverse_lds" in st["kernel"], st["kernel"]
        # the tree's own copy of the shape AABBs (k_refit_leaves writes it) after either refit
        pts = _points(step.aabbs, sc, N_POINTS, dtype, 9)
        kp = pts[:: N_POINTS // N_KNN]
        want = kr.knearest(step.flat, step.aabbs, kp, KS)
        for kk in KS:
            s_, d_ = flat.knearest_batch(kp, kk)
            assert np.array_equal(s_, want[kk][0]) and kr.same(d_, want[kk][1]), (k, kk)
        if k == 0:                                                              # the other point and box consumers: after the second refit only (run time)
            continue
        # points
        for use_tris in (False, True):
            s_, d_ = flat.nearest_batch(pts, triangles=use_tris)
            os_, od_ = orc.nearest(step.flat, step.aabbs, pts, step.tris if use_tris else None)
            assert np.array_equal(s_, os_) and same(d_, od_), use_tris
        for md in (None, dtype(4.0 * sc)):
            want = ktr.knearest_tree(step.nodes, step.aabbs, kp, KS, max_dist=md)
            for kk in KS:
                s_, d_ = bvh.knearest_tree_batch(kp, kk, max_dist=md)
                assert np.array_equal(s_, want[kk][0]) and kr.same(d_, want[kk][1]), (kk, md)
        # AABB / point / ball queries around moved shapes, both walks
        b = step.aabbs[rng.integers(0, n, N_QUERIES)].astype(np.float64)
        cq = (b[:, :3] + b[:, 3:]) * 0.5 + rng.normal(size=(N_QUERIES, 3)) * sc
        e = rng.uniform(0, 3, size=(N_QUERIES, 3)) * sc
        for kind, q64 in ((qr.AABB, np.concatenate([cq - e, cq + e], axis=1)), (qr.POINT, cq), (qr.BALL, np.concatenate([cq, e[:, :1]], axis=1))):
            q = q64.astype(dtype)
            qoff, qidx = qr.walk(step.flat, step.aabbs, kind, q)
            for variant in (0, 1):
                wctx.set_tuning(TUNE_QUERY_VARIANT, variant)
                goff, gidx = wflat.query_batch(kind, q)
                assert goff.tobytes() == qoff.tobytes() and gidx.tobytes() == qidx.tobytes(), (kind, variant)
        wctx.set_tuning(TUNE_QUERY_VARIANT, -1)
        # self-overlap: the tree's own (moved) boxes are the queries
        soff, sidx = flat.self_overlaps()
        eoff, eidx = flat.query_batch("aabb", step.aabbs)
        assert soff.tobytes() == eoff.tobytes() and sidx.tobytes() == eidx.tobytes()
        rows = rng.integers(0, n, min(n, 100))
        roff, ridx = qr.walk(step.flat, step.aabbs, qr.AABB, step.aabbs[rows])
        for j, i in enumerate(rows):
            got = sidx[soff[i]:soff[i + 1]]
            assert i in got and np.array_equal(got, ridx[roff[j]:roff[j + 1]]), i
        # the host batch out of pageable memory
        hoff, hidx = np.zeros(len(step.rays) + 1, np.uint32), np.zeros(max(len(step.idx), 1), np.uint32)
        assert bvh.traverse_host(np.ascontiguousarray(step.rays), None, hoff, hidx) == len(step.idx)
        assert np.array_equal(hoff, step.off) and np.array_equal(hidx[:len(step.idx)], step.idx)
        # the scene blob of the refitted tree on a peer
        blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
        flat.scene_export(blob)
        peer = FlatBvh.scene_import(blob, len(blob), ctx)
        poff, pidx, _, _ = peer.traverse_batch(_rb(eng, step.rays))
        assert np.array_equal(poff, step.off) and np.array_equal(pidx, step.idx)
        peer.close()
    bvh.close(); wbvh.close()


# ---- c. exact_only ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("overflow", np.float32), ("overflow", np.float64), ("deep", np.float32)],
                         ids=["overflow-float32", "overflow-float64", "deep-float32"])
def test_first_wide_walk_of_a_tree_with_empty_child_boxes_comes_after_its_refit(eng, orc, name, dtype):
    """A split without SAH winner leaves empty child boxes and the tree to the binary walk.  A refit — with the very boxes of the build —
    turns them into exact joins: the node array differs from the built one, and the wide walk, which this tree has never seen, answers the
    same batch; a rebuild brings the built tree and the binary walk back."""
    c = _case(name, dtype)
    a0, built = c["a0"], c["built"].nodes
    assert has_empty_child(built)
    ctx = _wide_ctx(eng)
    bvh = eng.Bvh.from_aabbs(a0, ctx)
    flat = bvh.flatten()
    # (the wide walk keeps a batch while no lane outgrows its stack — 3 pushes per step, 30 entries at the least: enough for every ray on the
    #  overflow band's 18 levels, and on the 27 levels of the deep tree for rays that cross the chain, which push nothing)
    rays = _crossing_rays(orc, a0, N_RAYS, dtype, 5) if name == "deep" else _rays(orc, a0, c["sc"], N_RAYS, dtype, 5)
    rb = _rb(eng, rays)

    def batch(nodes):
        off, idx, _, st = flat.traverse_batch(rb)
        ooff, oidx, _, _ = orc.traverse_flat(orc.flatten(nodes), a0, rays)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        assert len(oidx) > 0
        return st["kernel"]

    assert bvh.nodes.tobytes() == built.tobytes()
    assert "k_traverse_wide" not in batch(built)
    bvh.refit(a0)
    refitted = orc.refit(built, a0)
    assert bvh.nodes.tobytes() == refitted.tobytes() and refitted.tobytes() != built.tobytes()
    assert flat.nodes.tobytes() == orc.flatten(refitted).tobytes()
    assert "k_traverse_wide" in batch(refitted)
    bvh.rebuild(a0, flatten=True)
    assert bvh.nodes.tobytes() == built.tobytes()
    assert flat.nodes.tobytes() == orc.flatten(built).tobytes()
    assert "k_traverse_wide" not in batch(built)
    bvh.close()


# ---- d. a batch in flight -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refit_with_a_batch_or_a_build_in_flight(eng, orc, dtype):
    import torch
    from bvh_amd import RayBatch
    from bvh_amd.api import _Hits
    c = _case("ragged4097", dtype)
    a0, built = c["a0"], c["built"].nodes
    s1, s2 = c["steps"]
    ctx = _wide_ctx(eng)
    bvh = eng.Bvh.from_aabbs(a0, ctx)
    flat = bvh.flatten()
    rays = s1.rays
    keep = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    rb = RayBatch.from_device(keep, len(rays), dtype)
    hits = _Hits(ctx)
    ooff0, oidx0, _, _ = orc.traverse_flat(orc.flatten(built), a0, rays)
    assert not np.array_equal(oidx0, s1.idx)                       # the two trees do answer differently
    bvh.traverse_async(rb, hits)
    bvh.refit(s1.aabbs)                                            # completes the batch first, on the tree it was enqueued on
    st = hits.wait()
    off, idx = hits.fetch(len(rays))
    assert np.array_equal(off, ooff0) and np.array_equal(idx, oidx0) and st["hits"] == len(oidx0)
    bvh.traverse_async(rb, hits)
    st = hits.wait()
    off, idx = hits.fetch(len(rays))
    assert np.array_equal(off, s1.off) and np.array_equal(idx, s1.idx) and st["hits"] == len(s1.idx)
    # a refit right behind an asynchronous rebuild: the build is completed first
    dev0 = _device(a0)
    bvh.rebuild_async(dev0)
    bvh.refit(s2.aabbs)
    want = orc.refit(built, s2.aabbs)
    assert bvh.nodes.tobytes() == want.tobytes()
    assert flat.nodes.tobytes() == orc.flatten(want).tobytes()
    assert want.tobytes() == s2.nodes.tobytes()                    # (a refit forgets the boxes it finds)
    bvh.close()


# ---- e. errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_errors_leave_the_tree_usable(eng, orc, dtype):
    from bvh_amd import Context, FlatBvh, _lib
    from bvh_amd._lib import HOST, INVALID_ARG, BvhGpuError, check, ptr
    c = _case("ragged1025", dtype)
    a0, built = c["a0"], c["built"]
    s1 = c["steps"][0]
    n = len(a0)
    ctx = Context(0)
    bvh = eng.Bvh.from_aabbs(a0, ctx)
    flat = bvh.flatten()
    fn = getattr(_lib.load(), f"bvhgpu_refit_{bvh.sfx}")
    oflat0 = orc.flatten(built.nodes)
    rays = s1.rays
    ooff0, oidx0, _, _ = orc.traverse_flat(oflat0, a0, rays)

    def usable(tree, nodes=None):
        off, idx, _, _ = tree.traverse_batch(_rb(eng, rays))
        assert np.array_equal(off, ooff0) and np.array_equal(idx, oidx0)
        if nodes is not None:
            assert tree.nodes.tobytes() == nodes.tobytes()

    def refused(tree, *args):
        with pytest.raises(BvhGpuError) as e:
            check(fn(tree._t, *args), ctx._h)
        assert e.value.status == INVALID_ARG

    with pytest.raises(BvhGpuError) as e:
        bvh.refit(s1.aabbs[:n - 1])                                # the shape count must match
    assert e.value.status == INVALID_ARG
    usable(flat, oflat0)
    refused(bvh, None, n, HOST)                                    # NULL with n > 0
    usable(flat, oflat0)
    refused(bvh, ptr(s1.aabbs), n, 7)                              # a memory kind that does not exist
    usable(flat, oflat0)
    assert bvh.nodes.tobytes() == built.nodes.tobytes()
    # trees without a BvhNode array: an imported scene, an uploaded FlatBvh
    blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
    flat.scene_export(blob)
    imp = FlatBvh.scene_import(blob, len(blob), ctx)
    up = FlatBvh.from_flat_nodes(oflat0, a0, ctx)
    for t in (imp, up):
        refused(t, ptr(s1.aabbs), n, HOST)
        usable(t)
        t.close()
    # and the tree still takes a refit
    bvh.refit(s1.aabbs)
    assert bvh.nodes.tobytes() == s1.nodes.tobytes() and flat.nodes.tobytes() == s1.flat.tobytes()
    bvh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refit_of_no_shape_and_of_one_shape(eng, orc, dtype):
    from bvh_amd import Context
    ctx = Context(0)
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx)
    empty.flatten_in_place()
    empty.refit(np.zeros((0, 6), dtype))
    assert len(empty.nodes) == 0 and len(empty.flatten().nodes) == 0
    box = np.array([[0, 0, 0, 1, 1, 1]], dtype)
    new = np.array([[10, -0.0, 0.0, 11, 2, 0.5]], dtype)
    o = np.array([[0.5, 0.5, -5], [10.5, 1.5, -5], [10.5, 0.25, -5], [10.5, 0.25, 5]], dtype)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]], dtype)
    rays = orc.make_rays(o, d, dtype)
    for flatten_first in (True, False):
        one = eng.Bvh.from_aabbs(box, ctx)
        if flatten_first:
            one.flatten_in_place()
        bad = new.copy(); bad[0, 4] = np.nan
        one.refit(bad)                                             # a single shape is accepted as it is, as the builders accept it
        one.refit(new)
        flat = one.flatten()
        on = orc.build(new)
        assert one.nodes.tobytes() == on.nodes.tobytes() and flat.nodes.tobytes() == orc.flatten(on.nodes).tobytes()
        off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))       # the single AABB is what traversal tests
        ooff, oidx, _, _ = orc.traverse_flat(orc.flatten(on.nodes), new, rays)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and off.tolist() == [0, 0, 1, 2, 3]
        s_, d_ = flat.knearest_batch(np.array([[10.5, 5, 0.25]], dtype), 1)
        assert s_.tolist() == [[0]] and d_.tolist() == [[3.0]]     # ... and what the point queries measure
        one.close()
    empty.close()


# ---- 3. the input contract ----------------------------------------------------------------------------------------------------
BAD_VALUES = [(np.nan, 1), (np.nan, 4), (np.inf, 5), (-np.inf, 0), (np.inf, 2), (-np.inf, 3)]   # (value, component): NaN in a min and in a max component, ±inf


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("n", [2, 65, 3000])
def test_nonfinite_input_is_refused_and_changes_nothing(eng, orc, dtype, mem, n):
    """Refit takes the builders' input contract: for n >= 2 any NaN or ±inf component makes the call itself return INVALID_ARG, and the
    BvhNode array, the FlatNode array, a ray batch and a k-nearest batch (which reads the tree's own copy of the shape AABBs) are byte for
    byte what they were.  (Its joins are defined on NaN-free floats only: before, a NaN vanished from every ancestor box without an error,
    and the oracle's refit of the same input is not even consistent.)"""
    from bvh_amd import Context
    from bvh_amd._lib import INVALID_ARG, BvhGpuError
    rng = np.random.default_rng(n)
    lo = rng.uniform(-100, 100, size=(n, 3)).astype(dtype)
    a0 = np.ascontiguousarray(np.concatenate([lo, lo + rng.uniform(0, 10, size=(n, 3)).astype(dtype)], axis=1))
    a1, _ = moved("", a0, 1.0, dtype, 1)
    a2, _ = moved("", a0, 1.0, dtype, 2)
    built = orc.build(a0).nodes
    ctx = Context(0)
    bvh = eng.Bvh.from_aabbs(a0, ctx)
    flat = bvh.flatten()
    give = (lambda a: _device(a)) if mem == "device" else (lambda a: a)
    keep = give(a1)
    bvh.refit(keep)
    on1 = orc.refit(built, a1)
    assert bvh.nodes.tobytes() == on1.tobytes()
    rays = _rays(orc, a1, 1.0, 400, dtype, 3)
    pts = _points(a1, 1.0, 50, dtype, 4)

    def state():
        off, idx, ts, _ = flat.traverse_batch(_rb(eng, rays), want_t=True)
        s_, d_ = flat.knearest_batch(pts, min(3, n))
        return [x.tobytes() for x in (bvh.nodes, flat.nodes, off, idx, ts, s_, d_)]

    before = state()
    ooff, oidx, _, _ = orc.traverse_flat(orc.flatten(on1), a1, rays)
    assert before[2] == ooff.tobytes() and before[3] == oidx.tobytes() and len(oidx) > 0
    for value, comp in BAD_VALUES:
        for shape in (0, n // 2, n - 1):
            bad = a2.copy()
            bad[shape, comp] = value
            keep = give(bad)
            with pytest.raises(BvhGpuError) as e:
                bvh.refit(keep)
            assert e.value.status == INVALID_ARG and "NaN or infinity" in str(e.value), (value, comp, shape)
            assert state() == before, (value, comp, shape)
    keep = give(a2)
    bvh.refit(keep)                                                 # a valid refit afterwards
    on2 = orc.refit(built, a2)
    assert bvh.nodes.tobytes() == on2.tobytes() and orc.check_tree(on2, a2) == 0
    assert flat.nodes.tobytes() == orc.flatten(on2).tobytes()
    s_, d_ = flat.knearest_batch(pts, min(3, n))
    want = kr.knearest(orc.flatten(on2), a2, pts, (min(3, n),))[min(3, n)]
    assert np.array_equal(s_, want[0]) and kr.same(d_, want[1])
    bvh.close()
