"""AABB / point / ball query batches on the MI355X (bvhgpu_query_*, Bvh / FlatBvh .traverse / .query_batch / .self_overlaps):
byte-equal CSR against the CPU checker (tests/query_ref.py, a lockstep walk of the oracle's FlatNode array) for every walk, tree
shape and memory kind, and the reference's own known answers (tests/golden/query_known_answers.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import query_ref as qr  # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "query_known_answers.json")))
KINDS = {"aabb": qr.AABB, "point": qr.POINT, "ball": qr.BALL}
KNOB = 22   # BVHGPU_TUNE_QUERY_VARIANT


@pytest.fixture(scope="module")
def ctx():
    from bvh_amd import Context
    c = Context(0)
    yield c
    c.set_tuning(KNOB, -1)


def _scene(n_cubes, dtype):
    from bvh_amd import testbase as tb
    return tb.create_n_cubes(n_cubes)[1].astype(dtype)


def _tree(ctx, aabbs):
    from bvh_amd import Bvh
    bvh = Bvh.from_aabbs(aabbs, ctx)
    bvh.flatten_in_place()
    return bvh


def _queries(kind, n, aabbs, dtype, seed, scale=0.02):
    """half of the queries anywhere in the scene's bounds, half near a random shape's centre (the cubes fill little of the volume)"""
    rng = np.random.default_rng(seed)
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    c = rng.uniform(lo, hi, size=(n, 3))
    near = rng.integers(0, len(aabbs), size=n // 2)
    b = aabbs[near].astype(np.float64)
    c[:n // 2] = (b[:, :3] + b[:, 3:]) * 0.5 + rng.normal(size=(n // 2, 3)) * (b[:, 3:] - b[:, :3])
    if kind == qr.POINT:
        return c.astype(dtype)
    e = rng.uniform(0.0, 1.0, size=(n, 3)) * (hi - lo) * scale
    if kind == qr.AABB:
        return np.concatenate([c - e, c + e], axis=1).astype(dtype)
    return np.concatenate([c, e[:, :1]], axis=1).astype(dtype)


def _edge_rows(kind, aabbs, dtype):
    """NaN per component, inverted and infinite boxes, touching faces, ±0, r = 0, r < 0, r*r = inf, a centre on a face"""
    nan, inf = np.nan, np.inf
    b = aabbs[0].astype(np.float64)
    mn, mx = b[:3], b[3:]
    rows = []
    if kind == qr.AABB:
        for k in range(6):
            r = np.concatenate([mn, mx]); r[k] = nan; rows.append(r)
        rows += [np.concatenate([mx, mn]), [-inf, -inf, -inf, inf, inf, inf], [-inf, mn[1], mn[2], mn[0], mx[1], mx[2]],
                 np.concatenate([mx, mx + 1.0]), np.concatenate([mn - 1.0, mn]), [-0.0, -0.0, -0.0, 0.0, 0.0, 0.0], [nan] * 6]
    elif kind == qr.POINT:
        for k in range(3):
            r = mn.copy(); r[k] = nan; rows.append(r)
        rows += [mn, mx, [-0.0, 0.0, -0.0], [inf, mn[1], mn[2]], (mn + mx) * 0.5]
    else:
        c = (mn + mx) * 0.5
        for k in range(4):
            r = np.concatenate([c, [1.0]]); r[k] = nan; rows.append(r)
        rows += [np.concatenate([c, [0.0]]), np.concatenate([c, [-0.5]]), np.concatenate([c, [1e30 if dtype == np.float32 else 1e300]]),
                 np.concatenate([[mx[0]], c[1:], [0.0]]), np.concatenate([mx, [0.0]]), [-0.0, 0.0, 0.0, 0.0], np.concatenate([c, [inf]])]
    return np.asarray(rows, dtype=np.float64).astype(dtype)


def _check(bvh_or_flat, flat_ref, aabbs, kind, q):
    off, idx = bvh_or_flat.query_batch(kind, q)
    ooff, oidx = qr.walk(flat_ref, aabbs, kind, q)
    assert off.tobytes() == ooff.tobytes(), "offsets differ from the checker"
    assert idx.tobytes() == oidx.tobytes(), "indices differ from the checker"
    return off, idx


# ---- 1. the reference's known answers through traverse ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_answers_through_traverse(ctx, dtype):
    from bvh_amd import Aabb, Sphere, testbase as tb
    boxes = tb.generate_aligned_boxes_aabbs().astype(dtype)
    g = GOLD["aligned_boxes"]
    ids = g["ids"]
    bvh = _tree(ctx, boxes)
    flat = bvh.flatten()
    shapes = list(range(len(boxes)))
    for case in g["queries"]:
        q = case["query"]
        kind = KINDS[case["kind"]]
        obj = {qr.AABB: lambda: Aabb(q[:3], q[3:], dtype), qr.POINT: lambda: q, qr.BALL: lambda: Sphere(q[:3], q[3], dtype)}[kind]()
        _, want = qr.walk(qr.reference_lists(boxes, kind, [q])[2], boxes, kind, np.asarray([q], dtype=dtype))
        for h in (bvh, flat):
            got = h.traverse(obj, shapes)
            assert sorted(ids[i] for i in got) == sorted(case["hit_ids"]), case
            assert got == want.tolist(), case
    for case in GOLD["doc_tests"]:
        b = _tree(ctx, np.asarray([case["box"]], dtype=dtype))
        kind = KINDS[case["kind"]]
        off, idx = b.query_batch(kind, np.asarray([case["query"]], dtype=dtype))
        assert (idx.tolist() == [0]) == case["hit"], case
        b.close()
    bvh.close()


# ---- 2. parity with the checker: dtypes x kinds x scenes x walks ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_cubes", [100, 10_000])
def test_parity_with_checker(ctx, dtype, n_cubes):
    from oracle import orc
    aabbs = _scene(n_cubes, dtype)
    bvh = _tree(ctx, aabbs)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    for kind in (qr.AABB, qr.POINT, qr.BALL):
        n = 20_000 if n_cubes == 100 else 3_000     # 1 200 triangles: a batch above the wide walk's default threshold
        q = _queries(kind, n, aabbs, dtype, seed=11 * kind + n_cubes)
        if n_cubes == 100:
            q = np.concatenate([_edge_rows(kind, aabbs, dtype), q])
        ooff, oidx = qr.walk(oflat, aabbs, kind, q)
        kernels = []
        for knob in (0, 1, -1):
            ctx.set_tuning(KNOB, knob)
            off, idx = bvh.query_batch(kind, q)
            assert off.tobytes() == ooff.tobytes(), (kind, knob)
            assert idx.tobytes() == oidx.tobytes(), (kind, knob)
            kernels.append(bvh.query_kernel())
        ctx.set_tuning(KNOB, -1)
        assert kernels[0].startswith("bvhgpu::k_query<") and kernels[1].startswith("bvhgpu::k_query_wide<"), kernels
        assert len(oidx) > 0
    bvh.close()


# ---- 3. self-overlap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_self_overlaps_equals_explicit_boxes(ctx, dtype):
    aabbs = _scene(1000, dtype)
    bvh = _tree(ctx, aabbs)
    off, idx = bvh.self_overlaps()
    off2, idx2 = bvh.query_batch("aabb", aabbs)
    assert off.tobytes() == off2.tobytes() and idx.tobytes() == idx2.tobytes()
    for i in range(len(aabbs)):
        assert i in idx[off[i]:off[i + 1]]
    from bvh_amd import _lib
    h = C.c_void_p()
    rc = getattr(_lib.load(), f"bvhgpu_query_{bvh.sfx}")(bvh._t, _lib.QUERY_POINT, None, len(aabbs), _lib.HOST, 0, C.byref(h))
    assert rc == _lib.INVALID_ARG
    rc = getattr(_lib.load(), f"bvhgpu_query_{bvh.sfx}")(bvh._t, _lib.QUERY_AABB, None, len(aabbs) - 1, _lib.HOST, 0, C.byref(h))
    assert rc == _lib.INVALID_ARG
    _lib.load().bvhgpu_hits_destroy(h)
    bvh.close()


# ---- 4. tree shapes ------------------------------------------------------------------------------------------------------------
def _no_winner_scene(dtype, n=400, seed=5):
    rng = np.random.default_rng(seed)
    big = dtype(1e19 if dtype == np.float32 else 1e154)
    lo = (rng.uniform(-1, 1, size=(n, 3)) * big).astype(dtype)
    return np.concatenate([lo, lo + big * dtype(0.01)], axis=1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tree_shapes(ctx, dtype):
    from bvh_amd import FlatBvh
    from oracle import orc
    scenes = {"empty": np.zeros((0, 6), dtype=dtype), "one": _scene(1, dtype)[:1], "cubes": _scene(300, dtype)}
    for name, aabbs in scenes.items():
        bvh = _tree(ctx, aabbs)
        from bvh_amd import _lib
        oflat = orc.flatten(orc.build(aabbs).nodes) if len(aabbs) else np.zeros(0, dtype=_lib.FLAT_F32 if dtype == np.float32 else _lib.FLAT_F64)
        src = aabbs if len(aabbs) else np.asarray([[0, 0, 0, 1, 1, 1]], dtype=dtype)
        for kind in (qr.AABB, qr.POINT, qr.BALL):
            q = np.concatenate([_queries(kind, 500, src, dtype, seed=3 + kind, scale=0.2), _edge_rows(kind, src, dtype)])
            for knob in (0, 1):
                ctx.set_tuning(KNOB, knob)
                _check(bvh, oflat, aabbs, kind, q)
        ctx.set_tuning(KNOB, -1)
        if name == "cubes":
            # refitted tree (the shapes moved, same topology)
            moved = aabbs.copy()
            moved[:, [0, 3]] += dtype(0.25)
            moved[::7, 3:] += dtype(0.5)
            bvh.refit(moved)
            rflat = orc.flatten(orc.refit(orc.build(aabbs).nodes, moved))
            for kind in (qr.AABB, qr.BALL):
                q = _queries(kind, 2000, moved, dtype, seed=21, scale=0.1)
                for knob in (0, 1):
                    ctx.set_tuning(KNOB, knob)
                    _check(bvh, rflat, moved, kind, q)
            ctx.set_tuning(KNOB, -1)
            # tree_from_flat (an uploaded FlatBvh: binary walk) and an imported scene blob
            up = FlatBvh.from_flat_nodes(oflat, aabbs, ctx)
            src_tree = _tree(ctx, aabbs)
            src_flat = src_tree.flatten()
            nb = src_flat.scene_nbytes()
            blob = np.zeros(nb, dtype=np.uint8)
            src_flat.scene_export(blob)
            imp = FlatBvh.scene_import(blob, nb, ctx)
            src_tree.close()
            for t in (up, imp):
                for kind in (qr.AABB, qr.POINT, qr.BALL):
                    q = _queries(kind, 2000, aabbs, dtype, seed=31 + kind, scale=0.1)
                    for knob in (0, 1):
                        ctx.set_tuning(KNOB, knob)
                        _check(t, oflat, aabbs, kind, q)
                ctx.set_tuning(KNOB, -1)
            up.close(); imp.close()
        bvh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_bounds_tree_takes_the_binary_walk(ctx, dtype):
    from oracle import orc
    aabbs = _no_winner_scene(dtype)
    bvh = _tree(ctx, aabbs)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    for kind in (qr.AABB, qr.POINT, qr.BALL):
        q = np.concatenate([_queries(kind, 20_000, aabbs, dtype, seed=41 + kind, scale=0.3), _edge_rows(kind, aabbs, dtype)])
        if kind == qr.AABB:
            q = np.concatenate([q, np.asarray([np.concatenate([lo, hi]), [np.nan] * 6], dtype=dtype)])
        for knob in (1, -1):
            ctx.set_tuning(KNOB, knob)
            _check(bvh, oflat, aabbs, kind, q)
            assert bvh.query_kernel().startswith("bvhgpu::k_query<"), bvh.query_kernel()
    ctx.set_tuning(KNOB, -1)
    bvh.close()


def test_deep_tree_overflows_the_wide_stack_and_replays(ctx):
    from oracle import orc
    x = 2.0 ** np.arange(400)
    aabbs = np.stack([x, np.zeros_like(x), np.zeros_like(x), x * 1.25, np.ones_like(x), np.ones_like(x)], 1).astype(np.float64)
    bvh = _tree(ctx, aabbs)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    q = np.asarray([[-1.0, -1.0, -1.0, 1e300, 2.0, 2.0]] * 64 + [[0.0, 0.0, 0.0, 10.0, 1.0, 1.0]] * 64, dtype=np.float64)
    ctx.set_tuning(KNOB, 1)
    off, idx = _check(bvh, oflat, aabbs, qr.AABB, q)
    assert off[1] == len(aabbs)
    assert bvh.query_kernel().startswith("bvhgpu::k_query<"), bvh.query_kernel()   # replayed with the binary walk
    ctx.set_tuning(KNOB, -1)
    bvh.close()


# ---- 5. a hit-heavy batch that overflows the first pool ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hit_heavy_batch_grows_the_pool(ctx, dtype):
    from oracle import orc
    aabbs = _scene(100, dtype)
    bvh = _tree(ctx, aabbs)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    q = np.repeat(np.concatenate([lo - 1, hi + 1])[None, :], 300, axis=0).astype(dtype)
    q[::2, 3] = (lo[0] + hi[0]) * dtype(0.5)
    for knob in (0, 1):
        ctx.set_tuning(KNOB, knob)
        off, idx = _check(bvh, oflat, aabbs, qr.AABB, q)
        assert int(off[-1]) > 65536 and int(off[-1]) == len(idx)
    ctx.set_tuning(KNOB, -1)
    bvh.close()


# ---- 6. one result object: rays, queries, rays -------------------------------------------------------------------------------
def test_result_object_reused_across_ray_and_query_batches(ctx):
    from bvh_amd import BvhGpuError, RayBatch, _lib
    from oracle import orc
    aabbs = _scene(100, np.float32)
    rays = orc.create_rays(0, 20_000)
    q = _queries(qr.BALL, 5000, aabbs, np.float32, seed=2, scale=0.05)
    keep = [_tree(ctx, aabbs) for _ in range(3)]
    a, fr, fq = (t.flatten() for t in keep)
    r1 = a.traverse_batch(RayBatch(len(rays), np.float32, host=rays))[:2]
    q1 = a.query_batch("ball", q)
    r2 = a.traverse_batch(RayBatch(len(rays), np.float32, host=rays))[:2]
    fresh_r = fr.traverse_batch(RayBatch(len(rays), np.float32, host=rays))[:2]
    fresh_q = fq.query_batch("ball", q)
    for x, y in ((r1, fresh_r), (r2, fresh_r), (q1, fresh_q)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    a.query_batch("point", q[:, :3])
    with pytest.raises(BvhGpuError) as e:
        a._hits.fetch_triangles()
    assert e.value.status == _lib.INVALID_ARG
    with pytest.raises(BvhGpuError) as e:
        a._hits.fetch_closest(len(q))
    assert e.value.status == _lib.INVALID_ARG
    for t in keep:
        t.close()


# ---- 7. memory kinds, empty batches, errors, the walk's name -----------------------------------------------------------------
def test_memory_kinds_errors_and_walk_names(ctx):
    import torch
    from bvh_amd import _lib
    from oracle import orc
    lib = _lib.load()
    aabbs = _scene(1000, np.float32)
    bvh = _tree(ctx, aabbs)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    q = _queries(qr.POINT, 30_000, aabbs, np.float32, seed=9)
    ooff, oidx = qr.walk(oflat, aabbs, qr.POINT, q)
    # HOST and DEVICE queries; HOST and DEVICE fetch
    off, idx = bvh.query_batch("point", q)
    assert off.tobytes() == ooff.tobytes() and idx.tobytes() == oidx.tobytes()
    assert bvh.query_kernel() == "bvhgpu::k_query_wide<float, 2>", bvh.query_kernel()   # large batch, normal tree: wide by default
    assert bvh._hits.walk_flags() & _lib.WALK_WIDE
    tq = torch.from_numpy(q).cuda()
    bvh.query_batch("point", tq, fetch=False)
    doff = torch.zeros(len(q) + 1, dtype=torch.int32, device="cuda")
    didx = torch.zeros(max(len(oidx), 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.bvhgpu_hits_fetch(bvh._hits.h, _lib.ptr(doff.data_ptr()), _lib.ptr(didx.data_ptr()), None, _lib.DEVICE), ctx._h)
    torch.cuda.synchronize()
    assert doff.cpu().numpy().view(np.uint32).tobytes() == ooff.tobytes()
    assert didx.cpu().numpy().view(np.uint32)[:len(oidx)].tobytes() == oidx.tobytes()
    # an empty batch
    off, idx = bvh.query_batch("point", np.zeros((0, 3), dtype=np.float32))
    assert off.tolist() == [0] and len(idx) == 0
    # error codes
    h = C.c_void_p()
    assert lib.bvhgpu_query_f64(bvh._t, _lib.QUERY_AABB, _lib.ptr(q.astype(np.float64)), 1, _lib.HOST, 0, C.byref(h)) == _lib.DTYPE_MISMATCH
    assert lib.bvhgpu_query_f32(bvh._t, 7, _lib.ptr(q), 1, _lib.HOST, 0, C.byref(h)) == _lib.INVALID_ARG
    assert lib.bvhgpu_query_f32(bvh._t, _lib.QUERY_AABB, _lib.ptr(q), 1, _lib.HOST, 1, C.byref(h)) == _lib.INVALID_ARG
    t = C.c_void_p()
    _lib.check(lib.bvhgpu_build_f32(ctx._h, _lib.ptr(aabbs), len(aabbs), _lib.HOST, C.byref(t)), ctx._h)
    assert lib.bvhgpu_query_f32(t, _lib.QUERY_AABB, _lib.ptr(q), 1, _lib.HOST, 0, C.byref(h)) == _lib.NOT_FLATTENED
    lib.bvhgpu_tree_destroy(t)
    if h.value:
        lib.bvhgpu_hits_destroy(h)
    # the binary walk on a tree with empty child bounds, even for a large batch
    e = _tree(ctx, _no_winner_scene(np.float32))
    e.query_batch("point", q)
    assert e.query_kernel() == "bvhgpu::k_query<float, 2, 1>", e.query_kernel()
    e.close()
    bvh.close()


# ---- 8. determinism ------------------------------------------------------------------------------------------------------------
def test_same_batch_twice_is_identical(ctx):
    aabbs = _scene(1000, np.float64)
    bvh = _tree(ctx, aabbs)
    q = _queries(qr.BALL, 40_000, aabbs, np.float64, seed=4, scale=0.05)
    a = bvh.query_batch("ball", q)
    b = bvh.query_batch("ball", q)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    bvh.close()
