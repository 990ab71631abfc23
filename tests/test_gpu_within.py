"""Radius-search point queries on the GPU (bvhgpu_within_*): row i is every shape within max_dist[i] of point i — the loop of nearest_to
with a fixed limit, every comparison <= — in a stable ascending sort by distance, in the loop's order with BVHGPU_WITHIN_LIST_ORDER, or
counted only with BVHGPU_WITHIN_COUNT_ONLY, as a CSR without padding.  Every check compares offsets, shapes and distance bits byte for
byte against the definition restated over the oracle's FlatNode array (tests/within_ref.py); tests/test_within_cpu.py shows on the oracle
alone that the scenes used here have the row lengths, the ties and the reversed lists that cross every tier of bvh_amd/csrc/within.hip."""
import ctypes as C

import numpy as np
import pytest

import knn_ref as kr
import test_fp_extremes_queries_cpu as q
import within_ref as wr
from test_knn_cpu import cube_scene
from test_within_cpu import cloud_case, cube_case, far_scene, lengths, line_case, ties_case

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]


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


def _tree(eng, ctx, aabbs, tris=None):
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    if tris is not None:
        flat.set_triangles(tris)
    return flat


def _call(tree, pts, m, kind, sort=True, count_only=False, device=False):
    """within_batch → (offsets u32, shape u32, dist) as numpy, whichever memory the points are in"""
    if not device:
        o, s, d = tree.within_batch(pts, m, triangles=bool(kind), sort=sort, count_only=count_only)
        assert o.dtype == np.uint32 and s.dtype == np.uint32 and d.dtype == pts.dtype
        return o, s, d
    import torch
    tp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    tm = m if np.ndim(m) == 0 else torch.from_numpy(np.ascontiguousarray(m)).cuda()
    o, s, d = tree.within_batch(tp, tm, triangles=bool(kind), sort=sort, count_only=count_only)
    assert o.is_cuda and s.is_cuda and d.is_cuda and o.dtype == torch.int64 and s.dtype == torch.int32 and d.dtype == tp.dtype
    on = o.cpu().numpy()
    assert on.min(initial=0) >= 0
    return on.astype(np.uint32), s.cpu().numpy().view(np.uint32), d.cpu().numpy()


def _same(got, want, label):
    o, s, d = got
    assert o.shape == want[0].shape and o.tobytes() == want[0].tobytes(), (label, "offsets", np.nonzero(o != want[0])[0][:5])
    assert s.shape == want[1].shape and d.shape == want[2].shape and d.dtype == want[2].dtype, label
    bad = np.nonzero(s != want[1])[0]
    assert len(bad) == 0, (label, "shapes differ at", bad[:5], "row", np.searchsorted(o, bad[:5], side="right") - 1, s[bad[:5]], want[1][bad[:5]])
    assert d.tobytes() == want[2].tobytes(), (label, "distances", np.nonzero(d != want[2])[0][:5])


def _check(tree, pts, m, kind, list_rows, mems=(False, True), orders=(True, False), count=True, label=None):
    """sorted, list order and count-only, in host and device memory, against the rows of the definition"""
    dtype = pts.dtype.type
    for sort in orders:
        want = wr.csr(list_rows, dtype, sort)
        for device in mems:
            _same(_call(tree, pts, m, kind, sort, False, device), want, (label, kind, "sorted" if sort else "list order", "device" if device else "host"))
    if count:
        want = wr.csr(list_rows, dtype, False)
        for device in mems:
            o, s, d = _call(tree, pts, m, kind, True, True, device)
            assert o.tobytes() == want[0].tobytes() and s.shape == (0,) and d.shape == (0,), (label, kind, "count only")
            info = tree._hits.info()
            assert info["total"] == info["hits"] == len(want[1]), (label, info)


# ---- 1. the cube scene -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_cube_scene(eng, ctx, dtype):
    """1 200 triangles, about 2 000 points with NaN, infinite, max-finite and subnormal ones among them; a scalar limit and a per-point mix
    holding 0, negative, NaN and +inf; both shape distances, both memory spaces, all three outputs"""
    c = cube_case(dtype)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    t = "float" if dtype == np.float32 else "double"
    for kind in (0, 1):
        for name in ("scalar", "mixed"):
            _check(flat, c["pts"], c["limits"][name], kind, c["rows"][kind, name], label=name)
        tri = "true" if kind else "false"
        assert flat._hits.walk_kernel() == f"bvhgpu::k_within_count<{t}, {tri}, false>"
        _call(flat, c["pts"], c["limits"]["mixed"], kind, sort=False)
        assert flat._hits.walk_kernel() == f"bvhgpu::k_within_fill<{t}, {tri}, false, false>"
        info = flat._hits.info()
        assert info["visited"] == info["leaf_visits"] == info["device_steps"] == info["wave_steps"] == 0 and flat._hits.walk_flags() == 0
    # a Bvh flattens in place first
    bvh = eng.Bvh.from_aabbs(c["aabbs"], ctx)
    _same(bvh.within_batch(c["pts"], c["limits"]["scalar"]), wr.csr(c["rows"][0, "scalar"], dtype), "Bvh")


# ---- 2. row lengths across every tier ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_row_lengths(eng, ctx, dtype, reverse):
    """one batch whose rows have every length 0..300, 2^j - 1 / 2^j / 2^j + 1 up to 4096 and both thresholds +-1: the lane tier, the LDS
    tier and the global tier of the sort in one launch; the reverse rows come in descending distance, a full permutation in every tier"""
    c = line_case(dtype, reverse)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    for kind in (0, 1):
        o, _, _ = _call(flat, c["pts"], c["limits"], kind)
        assert np.array_equal(np.diff(o.astype(np.int64)), c["lengths"])
        _check(flat, c["pts"], c["limits"], kind, c["rows"][kind], mems=(False, True) if kind == 0 else (False,), label=("line", reverse))


# ---- 3. ties in every tier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_ties_in_every_tier(eng, ctx, dtype):
    """three shapes per position: equal distances must come out in leaf pre-order in the lane, the LDS and the global tier"""
    c = ties_case(dtype)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    for kind in (0, 1):
        _check(flat, c["pts"], c["limits"], kind, c["rows"][kind], label="ties")


# ---- 4. point counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_point_counts(eng, ctx, dtype):
    c = cube_case(dtype)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    m = c["limits"]["mixed"]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        for kind in (0, 1):
            _check(flat, c["pts"][:n], m[:n], kind, c["rows"][kind, "mixed"][:n], mems=(False, True) if n in (0, 1, 257, 1025) else (False,),
                   orders=(True,), label=n)
    o, s, d = flat.within_batch(c["pts"][:0], dtype(1))
    assert o.tolist() == [0] and s.shape == (0,) and d.shape == (0,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_scan_second_round(eng, orc, ctx, dtype):
    """256 * 1024 + 1 points: 257 scan blocks, so the one-workgroup scan of the block sums runs a second round.  A small tree with short
    rows; the batch repeats 64 distinct points, so the definition is computed for 64 rows"""
    boxes = orc.aligned_boxes().astype(dtype)
    oflat = orc.flatten(orc.build(boxes).nodes)
    rng = np.random.default_rng(43)
    base = np.concatenate([rng.uniform(-12, 12, size=(64, 1)), rng.uniform(-1, 1, size=(64, 2))], axis=1).astype(dtype)
    bm = np.asarray([0, 0.5, 1.0, 2.5, -1, np.nan, 0.25, 1.5], dtype=dtype)[np.arange(64) % 8]
    rows64 = wr.rows(oflat, boxes, base, bm)
    reps, n = 4096, 64 * 4096 + 1
    assert n == 256 * 1024 + 1
    pts, m = np.concatenate([np.tile(base, (reps, 1)), base[:1]]), np.concatenate([np.tile(bm, reps), bm[:1]])
    flat = _tree(eng, ctx, boxes)
    for sort in (True, False):
        bo, bs, bd = wr.csr(rows64, dtype, sort)
        first = int(bo[1])
        lens = np.concatenate([np.tile(np.diff(bo.astype(np.int64)), reps), [first]])
        want_o = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        want = (want_o, np.concatenate([np.tile(bs, reps), bs[:first]]), np.concatenate([np.tile(bd, reps), bd[:first]]))
        assert 0 < lens.max() <= wr.LANE_MAX and len(want_o) == n + 1
        _same(_call(flat, pts, m, 0, sort, False, device=sort), want, ("second round", sort))
    o, s, d = _call(flat, pts, m, 0, True, True)
    assert o.tobytes() == want[0].tobytes() and len(s) == 0


# ---- 5. tree kinds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_tree_kinds(eng, orc, ctx, dtype):
    import torch
    from bvh_amd import FlatBvh
    c = cube_case(dtype)
    tris, aabbs, nodes, oflat = c["tris"], c["aabbs"], c["nodes"], c["oflat"]
    pts, m = c["pts"][::5], c["limits"]["mixed"][::5]
    rng = np.random.default_rng(44)
    shift = rng.uniform(-0.4, 0.4, size=(len(aabbs), 1, 3)).astype(dtype)
    tris_moved = (tris + shift).astype(dtype)
    moved = np.concatenate([tris_moved.min(axis=1), tris_moved.max(axis=1)], axis=1).astype(dtype)

    def both(tree, flat_nodes, boxes, triangles, label):
        for kind in ((0, 1) if triangles is not None else (0,)):
            rows = wr.rows(flat_nodes, boxes, pts, m, triangles if kind else None)
            assert lengths(rows).max() > wr.LANE_MAX
            _check(tree, pts, m, kind, rows, label=label)

    both(_tree(eng, ctx, aabbs, tris), oflat, aabbs, tris, "built")
    up = FlatBvh.from_flat_nodes(oflat, moved, ctx)                          # an uploaded FlatBvh: stale navigator boxes, current shapes
    up.set_triangles(tris_moved)
    both(up, oflat, moved, tris_moved, "uploaded")
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)                                     # refitted
    bvh.refit(moved)
    refitted = bvh.flatten()
    refitted.set_triangles(tris_moved)
    both(refitted, orc.flatten(orc.refit(nodes, moved)), moved, tris_moved, "refitted")
    built = _tree(eng, ctx, aabbs)
    blob = np.zeros(built.scene_nbytes(), dtype=np.uint8)                    # scene-imported
    built.scene_export(blob)
    both(FlatBvh.scene_import(blob, len(blob), ctx), oflat, aabbs, None, "imported")
    # a tree that is still building when the call arrives: the call settles the build first
    again = eng.Bvh.from_aabbs(aabbs[:300], ctx)
    view = again.flatten()                                                   # (a FlatBvh view: its within_batch goes straight to the C call)
    dev = torch.from_numpy(moved).cuda()
    rows = wr.rows(orc.flatten(orc.build(moved).nodes), moved, pts, m)
    again.rebuild_async(dev)
    _same(view.within_batch(pts, m), wr.csr(rows, dtype), "still building")
    # one shape: a single (leaf) entry, no navigator
    one = _tree(eng, ctx, aabbs[:1], tris[:1])
    oflat1 = orc.flatten(orc.build(aabbs[:1]).nodes)
    far = np.where(np.isfinite(m) & (m > 0), dtype(4e5), m).astype(dtype)    # large enough to reach the one shape from anywhere
    for kind in (0, 1):
        rows = wr.rows(oflat1, aabbs[:1], pts, far, tris[:1] if kind else None)
        assert 0 < lengths(rows).sum() < len(pts)
        _check(one, pts, far, kind, rows, label="one shape")
    t = "float" if dtype == np.float32 else "double"
    assert one._hits.walk_kernel() == f"bvhgpu::k_within_count<{t}, true, true>"
    # no shapes: all offsets 0
    empty = _tree(eng, ctx, np.zeros((0, 6), dtype), np.zeros((0, 3, 3), dtype))
    for kind in (0, 1):
        _check(empty, pts, m, kind, [([], [])] * len(pts), label="empty")


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_tree_with_empty_child_bounds(eng, orc, ctx, dtype):
    """boxes so far apart that no bucket wins a split: both children get EMPTY bounds, a leaf's navigator box is then not its shape's box,
    and the engine walks an unfolded mirror of the FlatNode array"""
    far, tris, pts, m = far_scene(dtype)
    oflat = orc.flatten(orc.build(far).nodes)
    assert q.has_empty_child_bounds(oflat)
    flat = _tree(eng, ctx, far, tris)
    for kind in (0, 1):                                                      # (kind 1: candidates whose own box is beyond the limit, test_within_cpu)
        rows = wr.rows(oflat, far, pts, m, tris if kind else None)
        n = lengths(rows)
        assert (n > 0).sum() > 50 and n.max() > wr.LANE_MAX
        _check(flat, pts, m, kind, rows, label="empty child bounds")


# ---- 6. cross-checks on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_against_ball_query_and_knearest(eng, ctx, dtype):
    """GPU against GPU on the integer cloud, where every operation is exact: list-order kind-0 rows are query_batch("ball")'s CSR rows; the
    heads of sorted rows are knearest_batch's rows cut at the limit; for rows no longer than 64, knearest_tree_batch(64, max_dist) has
    bit-equal distances and the same shapes per group of equal distance"""
    c = cloud_case(dtype)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    pts, m = c["pts"], c["limits"]
    o, s, d = flat.within_batch(pts, m, sort=False)
    balls = np.concatenate([pts, m[:, None]], axis=1).astype(dtype)
    bo, bi = flat.query_batch("ball", balls)
    assert o.tobytes() == np.asarray(bo, dtype=np.uint32).tobytes() and s.tobytes() == np.asarray(bi, dtype=np.uint32).tobytes()
    n = np.diff(o.astype(np.int64))
    assert (n > 64).any() and ((n > 0) & (n <= 64)).sum() > 20
    for kind in (0, 1):
        o, s, d = flat.within_batch(pts, m, triangles=bool(kind))
        n = np.diff(o.astype(np.int64))
        for k in (1, 7, 64):
            hs, hd = wr.head_rows(o, s, d, k)
            ks, kd = flat.knearest_batch(pts, k, triangles=bool(kind))
            inside = kd <= m[:, None]                                        # (exact data: d <= m is d2 <= m * m)
            assert np.array_equal(inside.sum(axis=1), np.minimum(n, k)), (kind, k)
            assert np.array_equal(np.where(inside, ks, NONE), hs) and kr.same(np.where(inside, kd, np.inf).astype(dtype), hd), (kind, k)
        ts, td = flat.knearest_tree_batch(pts, 64, triangles=bool(kind), max_dist=m)
        for i in np.nonzero(n <= 64)[0]:
            b, e = int(o[i]), int(o[i + 1])
            assert (ts[i, e - b:] == NONE).all() and td[i, :e - b].tobytes() == d[b:e].tobytes(), (kind, i)
            assert sorted(zip(td[i, :e - b].tolist(), ts[i, :e - b].tolist())) == sorted(zip(d[b:e].tolist(), s[b:e].tolist())), (kind, i)


# ---- 7. floating-point extremes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", q.sweep_params(q.QUERY_SCALES))
def test_within_scale_sweep(eng, dtype, k):
    """the cube scene scaled from all-subnormal to overflowing, with the scalar limit and the limit vector of the k-nearest sweep (0,
    smallest subnormal, max finite, +inf, NaN, -1 and the reference's own neighbour distances, where the rounding of m * m decides)"""
    from bvh_amd import Context
    case = q.point_case(dtype, k)
    flat = eng.Bvh.from_aabbs(case["aabbs"], Context(0)).flatten()
    assert flat.nodes.tobytes() == case["oflat"].tobytes()
    flat.set_triangles(case["tris"])
    for kind in (0, 1):
        lims = case["limits"][kind]
        scalar, vector = wr.rows_multi(case["oflat"], case["aabbs"], case["pts"], [lims["scalar"], lims["vector"]], case["tris"] if kind else None)
        _check(flat, case["pts"], lims["scalar"], kind, scalar, mems=(False,), label=(q.tname(dtype), k, "scalar"))
        _check(flat, case["pts"], lims["vector"], kind, vector, mems=(False,), label=(q.tname(dtype), k, "vector"))


# ---- 8. one result object through every kind of batch ----------------------------------------------------------------------------------
def test_within_result_object_reuse(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    c = cube_case(dtype)
    flat = _tree(eng, ctx, c["aabbs"], c["tris"])
    pts, m = np.ascontiguousarray(c["pts"]), np.ascontiguousarray(c["limits"]["mixed"])
    n, n2 = len(pts), 300
    rays = np.ascontiguousarray(orc.create_rays(0, 2000))
    off, idx, ts, _ = orc.traverse_flat(c["oflat"], c["aabbs"], rays, want_t=True)
    h = C.c_void_p()
    total, nr = C.c_uint64(), C.c_size_t()
    big = max(len(idx), 200000)
    scratch_o, scratch_s, scratch_v = np.zeros(max(n, len(rays)) + 1, np.uint32), np.zeros(big, np.uint32), np.zeros((big, 3), dtype)

    def info():
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(total), None) == OK
        return nr.value, total.value

    def wrong_kind_fetches_refused(within):
        fetches = [lambda: lib.bvhgpu_hits_fetch(h, ptr(scratch_o), ptr(scratch_s), None, HOST),
                   lambda: lib.bvhgpu_hits_fetch_triangles(h, ptr(scratch_v), HOST),
                   lambda: lib.bvhgpu_hits_fetch_closest(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_any(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_box(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_sphere(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_allhits(h, ptr(scratch_o), ptr(scratch_s), ptr(scratch_v), HOST),
                   lambda: lib.bvhgpu_hits_device(h, None, None, None)]
        if within:
            for f in fetches:
                assert f() == INVALID_ARG
                assert "bvhgpu_hits_fetch_within" in lib.bvhgpu_last_error(ctx._h).decode()
        else:
            assert lib.bvhgpu_hits_fetch_within(h, ptr(scratch_o), ptr(scratch_s), ptr(scratch_v), HOST) == INVALID_ARG
            assert "bvhgpu_within" in lib.bvhgpu_last_error(ctx._h).decode()

    def fetch_within(npts, want, count_only=False):
        assert info() == (npts, len(want[1]))
        rows = 0 if count_only else len(want[1])
        o, s, d = np.zeros(npts + 1, np.uint32), np.full(len(want[1]) + 1, 0xABCD1234, np.uint32), np.full(len(want[1]) + 1, -77.5, dtype)
        assert lib.bvhgpu_hits_fetch_within(h, ptr(o), ptr(s), ptr(d), HOST) == OK
        assert o.tobytes() == want[0].tobytes() and s[:rows].tobytes() == want[1][:rows].tobytes() and d[:rows].tobytes() == want[2][:rows].tobytes()
        assert (s[rows:] == 0xABCD1234).all() and (d[rows:] == -77.5).all()          # nothing beyond the rows is written
        assert lib.bvhgpu_hits_fetch_within(h, None, None, None, HOST) == OK        # each may be NULL
        assert lib.bvhgpu_hits_wait(h) == OK
        wrong_kind_fetches_refused(True)

    def fetch_csr():
        assert info() == (len(rays), len(idx))
        o, s, t = np.zeros(len(rays) + 1, np.uint32), np.zeros(len(idx), np.uint32), np.zeros((len(idx), 2), dtype)
        assert lib.bvhgpu_hits_fetch(h, ptr(o), ptr(s), ptr(t), HOST) == OK
        assert o.tobytes() == off.tobytes() and s.tobytes() == idx.tobytes() and t.tobytes() == ts.tobytes()
        wrong_kind_fetches_refused(False)

    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), len(rays), HOST, 1, C.byref(h)) == OK              # traverse (T_SLICE)
    fetch_csr()
    first = h.value
    assert lib.bvhgpu_within_f32(flat._t, ptr(pts), ptr(m), n, HOST, 1, 0, C.byref(h)) == OK              # within, triangles, sorted
    assert h.value == first
    fetch_within(n, wr.csr(c["rows"][1, "mixed"], dtype, True))
    assert lib.bvhgpu_traverse_allhits_f32(flat._t, ptr(rays), None, len(rays), HOST, 0, 0, C.byref(h)) == OK   # all hits
    assert lib.bvhgpu_hits_fetch_allhits(h, ptr(scratch_o), ptr(scratch_s), ptr(scratch_v), HOST) == OK
    wrong_kind_fetches_refused(False)
    assert lib.bvhgpu_within_f32(flat._t, ptr(pts[:n2]), ptr(m[:n2]), n2, HOST, 0, 1, C.byref(h)) == OK   # a shorter batch, list order
    fetch_within(n2, wr.csr(c["rows"][0, "mixed"][:n2], dtype, False))
    assert lib.bvhgpu_within_f32(flat._t, ptr(pts), ptr(m), n, HOST, 0, 2, C.byref(h)) == OK              # count only
    fetch_within(n, wr.csr(c["rows"][0, "mixed"], dtype, False), count_only=True)
    assert lib.bvhgpu_query_f32(flat._t, 2, ptr(pts[:n2]), n2, HOST, 0, C.byref(h)) == OK                 # a point query
    wrong_kind_fetches_refused(False)
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), len(rays), HOST, 1, C.byref(h)) == OK              # traverse again
    fetch_csr()
    assert h.value == first
    lib.bvhgpu_hits_destroy(h)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_within_refusals(eng, orc):
    from bvh_amd import BvhGpuError, Context, _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, OVERFLOW, ptr
    import torch
    lib = _lib.load()
    ctx = Context(0)
    tris, aabbs = cube_scene(2, np.float32)
    pts = np.ascontiguousarray(tris[:4, 0])
    pts64 = pts.astype(np.float64)
    m, m64 = np.full(4, 2.0, np.float32), np.full(4, 2.0, np.float64)
    rays = np.ascontiguousarray(orc.create_rays(0, 4))
    f32, f64 = lib.bvhgpu_within_f32, lib.bvhgpu_within_f64
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    # the result object holds a box batch: a refused call leaves it, and what it answers, as they were
    other = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    h = C.c_void_p()
    assert lib.bvhgpu_traverse_box_f32(other._t, ptr(rays), None, 4, HOST, 0, C.byref(h)) == OK
    held = h.value
    sl0, sh0 = np.zeros((4, 2), np.float32), np.zeros(4, np.uint32)
    assert lib.bvhgpu_hits_fetch_box(h, ptr(sl0), ptr(sh0), HOST) == OK
    SENT = 0xABCD1234
    out_o, out_s, out_d = np.full(5, SENT, np.uint32), np.full(64, SENT, np.uint32), np.full(64, -77.5, np.float32)

    def refused(rc, status, word, handle=ctx._h):
        assert rc == status, (rc, status, word)
        msg = lib.bvhgpu_last_error(handle).decode()
        assert word in msg, (word, msg)
        assert h.value == held                                                     # *hits as it was
        sl, sh = np.zeros((4, 2), np.float32), np.zeros(4, np.uint32)
        assert lib.bvhgpu_hits_fetch_box(h, ptr(sl), ptr(sh), HOST) == OK and sl.tobytes() == sl0.tobytes() and sh.tobytes() == sh0.tobytes()
        assert lib.bvhgpu_hits_fetch_within(h, ptr(out_o), ptr(out_s), ptr(out_d), HOST) == INVALID_ARG
        assert np.all(out_o == SENT) and np.all(out_s == SENT) and np.all(out_d == -77.5), word

    refused(f32(None, ptr(pts), ptr(m), 4, HOST, 0, 0, C.byref(h)), INVALID_ARG, "NULL tree", None)
    refused(f64(bvh._t, ptr(pts64), ptr(m64), 4, HOST, 0, 0, C.byref(h)), DTYPE_MISMATCH, "dtype")
    refused(f32(bvh._t, ptr(pts), ptr(m), 4, HOST, 0, 0, C.byref(h)), NOT_FLATTENED, "bvhgpu_flatten")
    flat = bvh.flatten()
    refused(f32(flat._t, ptr(pts), ptr(m), 4, HOST, 0, 0, None), INVALID_ARG, "hits is NULL")
    refused(f32(flat._t, None, ptr(m), 4, HOST, 0, 0, C.byref(h)), INVALID_ARG, "points is NULL")
    refused(f32(flat._t, ptr(pts), None, 4, HOST, 0, 0, C.byref(h)), INVALID_ARG, "max_dist is NULL")
    refused(f32(flat._t, ptr(pts), ptr(m), 4, 7, 0, 0, C.byref(h)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    for kind in (2, -1, 1 << 20):
        refused(f32(flat._t, ptr(pts), ptr(m), 4, HOST, kind, 0, C.byref(h)), INVALID_ARG, "shape kind")
    for flags in (4, 7, 16, 1 << 27, 1 << 28, 1 << 31):
        refused(f32(flat._t, ptr(pts), ptr(m), 4, HOST, 0, flags, C.byref(h)), INVALID_ARG, "BVHGPU_WITHIN_LIST_ORDER")
    refused(f32(flat._t, ptr(pts), ptr(m), 4, HOST, 1, 0, C.byref(h)), INVALID_ARG, "bvhgpu_tree_set_triangles")
    refused(f32(flat._t, ptr(pts), ptr(m), 0xFFFFFFFF, HOST, 0, 0, C.byref(h)), OVERFLOW, "points")
    # the order of the checks: the first broken rule names itself
    refused(f32(flat._t, None, None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "points is NULL")
    refused(f32(flat._t, ptr(pts), None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "max_dist is NULL")
    refused(f32(flat._t, ptr(pts), ptr(m), 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    refused(f32(flat._t, ptr(pts), ptr(m), 0xFFFFFFFF, HOST, 9, 8, C.byref(h)), INVALID_ARG, "shape kind")
    refused(f32(flat._t, ptr(pts), ptr(m), 0xFFFFFFFF, HOST, 1, 8, C.byref(h)), INVALID_ARG, "BVHGPU_WITHIN_LIST_ORDER")
    refused(f32(flat._t, ptr(pts), ptr(m), 0xFFFFFFFF, HOST, 1, 3, C.byref(h)), INVALID_ARG, "bvhgpu_tree_set_triangles")
    # a result object that still holds an asynchronous batch
    rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    ha = C.c_void_p()
    assert lib.bvhgpu_traverse_async_f32(flat._t, ptr(rays_dev.data_ptr()), 4, _lib.DEVICE, 0, C.byref(ha)) == OK
    assert f64(flat._t, None, None, 4, 7, 9, 8, C.byref(ha)) == INVALID_ARG and "bvhgpu_hits_wait" in lib.bvhgpu_last_error(ctx._h).decode()
    assert lib.bvhgpu_hits_wait(ha) == OK
    lib.bvhgpu_hits_destroy(ha)
    # a tree whose asynchronous build failed: the settle's answer comes before everything else
    j = np.arange(1000, dtype=np.float32)
    chain = np.stack([j, 0 * j, 0 * j, j + 0.5, 0 * j + 1, 0 * j + 1], axis=1).astype(np.float32)
    nan_tree = eng.Bvh.from_aabbs(chain, ctx)
    chain[77, 3] = np.nan
    bad = torch.from_numpy(chain).cuda()
    nan_tree.rebuild_async(bad)
    refused(f64(nan_tree._t, None, None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "NaN")
    # the Python surface
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_triangles"):
        flat.within_batch(pts, 1.0, triangles=True)
    with pytest.raises(BvhGpuError) as e:
        flat.within_batch(pts64, 1.0)
    assert e.value.status == DTYPE_MISMATCH
    with pytest.raises(BvhGpuError):
        flat.within_batch(pts, m[:-1])
    with pytest.raises(BvhGpuError):
        flat.within_batch(pts, m64)
    with pytest.raises(BvhGpuError):
        flat.within_batch(pts, None)
    with pytest.raises(BvhGpuError):
        flat.within_batch(torch.from_numpy(pts).cuda(), m)                        # limits in host memory, points in HBM
    # ... and a valid call after all that works: an empty batch with NULL pointers on a fresh result object, then rows
    h2 = C.c_void_p()
    assert f32(flat._t, None, None, 0, HOST, 0, 0, C.byref(h2)) == OK and h2.value
    one = np.full(1, SENT, np.uint32)
    assert lib.bvhgpu_hits_fetch_within(h2, ptr(one), None, None, HOST) == OK and one.tolist() == [0]
    lib.bvhgpu_hits_destroy(h2)
    flat.set_triangles(tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    for kind in (0, 1):
        rows = wr.rows(oflat, aabbs, pts, m, tris if kind else None)
        assert lengths(rows).min() > 0
        _check(flat, pts, m, kind, rows, label="after the refusals")
    lib.bvhgpu_hits_destroy(h)
