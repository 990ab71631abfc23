"""Visibility masks for the point and region queries over instanced scenes on the GPU (bvhgpu_instances_within_masked_*,
_knearest_masked_*, _knearest_tree_masked_*, _region_masked_*): everything byte for byte, f32 and f64, HOST and HBM inputs.  The scenes and
masks tests/test_instances_point_masks_cpu.py shows to be worth running, against tests/instances_point_masks_ref.py; the anchor that does
not pass through the new reference (the engine's own unmasked rows of the same run filtered in numpy); the all-ones identity with every
unmasked entry; the edges; the masks' lifetime over update, an uncommitted and a stale set; the refusals of the eight symbols.
Nothing here provokes a fault: every refusal is made on the host before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import instances_point_masks_ref as ipm
import instances_region_ref as irr
import instances_within_ref as iwr
import knn_ref as kr
from test_instances_cpu import SIZES, member_trees, transforms
from test_instances_knn_cpu import cluster
from test_instances_masks_cpu import ALL, HIGH, PAL, inst_masks
from test_instances_point_masks_cpu import KS, LINE_N, limits_of, line_case, point_masks, region_masks, region_want, within_want

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
N_KNN = 200             # the cluster points the k-nearest forms are run on (the figures of the CPU file are read on these)
COMBOS = ("plain", "classify", "count_only", "instances_only", "instances_only_classify", "instances_only_count_only")
LIMIT_RUNS = (("none", KS), ("scalar", (3,)), ("drawn", (3, 64)), ("special", (3,)))


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


def _built_trees(eng, ctx, trees):
    """members with a BvhNode array (the tree form walks it)"""
    out = []
    for aabbs, tris in trees:
        b = eng.Bvh.from_aabbs(aabbs, ctx)
        b.flatten_in_place()
        b.set_triangles(tris)
        out.append(b)
    return out


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_mask(mask):
    import torch
    if mask is None or np.ndim(mask) == 0:
        return mask
    return torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint32).view(np.int32).copy()).cuda()


def _side(v, device):
    return _dev(v) if device and isinstance(v, np.ndarray) else v


def _np(x, index=False):
    if isinstance(x, np.ndarray):
        return x
    x = x.cpu().numpy()
    return x.view(np.uint32) if index else x


def _off(o):
    return o if isinstance(o, np.ndarray) else o.cpu().numpy().astype(np.uint32)


def _within(got):
    if set(got) == {"offsets"}:
        return (_off(got["offsets"]),)
    return _off(got["offsets"]), _np(got["instance"], True), _np(got["shape"], True), _np(got["dist"])


def _tuple_same(got, want, label):
    """byte for byte; two NaN distances are equal whatever their sign and payload (knn_ref.same: the far scenes' distances overflow)"""
    assert len(got) == len(want), label
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and kr.same(a, b), (label, k)


def _padded(got):
    return _np(got[0], True), _np(got[1], True), _np(got[2])


def _region(r):
    """a region result → (offsets u32, instance u32, shape u32 | None, inside u8 | None) as numpy"""
    return (_off(r["offsets"]), _np(r["instance"], True), _np(r["shape"], True) if "shape" in r else None, _np(r["inside"]) if "inside" in r else None)


def _region_kw(combo):
    return dict(classify="classify" in combo, count_only="count_only" in combo, instances_only=combo.startswith("instances_only"))


def _region_want(w, combo):
    off, inst, shape, ins = w["full"]
    toff, tidx, tins = w["top"]
    none = np.zeros(0, dtype=np.uint32)
    return dict(plain=(off, inst, shape, None), classify=(off, inst, shape, ins), count_only=(off, none, none, None),
                instances_only=(toff, tidx, None, None), instances_only_classify=(toff, tidx, None, tins),
                instances_only_count_only=(toff, none, None, None))[combo]


def _region_same(got, want, label):
    for name, g, w in zip(("offsets", "instance", "shape", "inside"), got, want):
        assert (g is None) == (w is None), (label, name)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes(), (label, name)


def _filter_rows(got, M, P, n):
    """the engine's own unmasked CSR (offsets, instance, *columns) with the pairs of invisible instances taken out, in numpy"""
    off, inst = got[0], got[1]
    row = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    keep = (M[inst.astype(np.int64)] & ipm.row_masks(P, n)[row]) != 0
    new_off = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.uint32)
    return (new_off,) + tuple(None if c is None else np.ascontiguousarray(c[keep]) for c in got[1:])


# ---- 1. within -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_within_against_the_reference(eng, orc, ctx, dtype, n):
    """sorted, list order and count only; rows on both sides of INST_WITHIN_LANE_ROW_MAX; and every masked row is the unmasked row of the
    same run filtered in numpy"""
    c, pts, m, _, masked, M, P = within_want(orc, dtype, n)
    lane_max, _ = iwr.engine_thresholds(ROOT)
    lens = np.array([len(r) for r in masked])
    if n == 37:
        assert ((lens > 0) & (lens <= lane_max)).sum() >= 20 and (lens > lane_max).sum() >= 20
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        inst.set_masks(M)
        for device in (False, True):
            p, md, pm = (_dev(pts), _dev(m), _dev_mask(P)) if device else (pts, m, P)
            for sort in (True, False):
                want = iwr.csr(masked, dtype, sort)
                got = _within(inst.within_masked_batch(p, md, pm, sort=sort))
                _tuple_same(got, want, (n, device, sort))
                free = _within(inst.within_batch(p, md, sort=sort))
                _tuple_same(got, _filter_rows(free, M, P, len(pts)), (n, device, sort, "anchor"))
            got = _within(inst.within_masked_batch(p, md, pm, count_only=True))
            _tuple_same(got, (iwr.csr(masked, dtype)[0],), (n, device, "count only"))
        t = "float" if dtype == np.float32 else "double"
        inst.within_masked_batch(pts, m, P)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_within_fill<{t}, true, true>"
        inst.within_batch(pts, m)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_within_fill<{t}, true>"


# ---- 2. knearest and the tree form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_knearest_against_the_reference(eng, orc, ctx, dtype, n):
    """k = 1, 3, 9, 17, 64: every block size of the list kernel.  The anchor: the distances of a masked row are those of the first k of the
    filtered sorted within_batch(+inf) row of the same run"""
    c, pts, cache = cluster(orc, dtype, n)
    pts = np.ascontiguousarray(pts[:N_KNN])
    M, P = inst_masks(n), point_masks(n, N_KNN)
    trees = _gpu_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        inst.set_masks(M)
        everything = _filter_rows(_within(inst.within_batch(pts, np.inf)), M, P, N_KNN)
        pd, Pd = _dev(pts), _dev_mask(P)
        for k in KS:
            want = ipm.padded(ipm.knn_rows(c["scene"], pts, k, M, P, cache), k, dtype)
            got = _padded(inst.knearest_masked_batch(pts, k, P))
            _tuple_same(got, want, (n, k, "host"))
            _tuple_same(_padded(inst.knearest_masked_batch(pd, k, Pd)), want, (n, k, "device"))
            off, dist = everything[0].astype(np.int64), everything[3]
            for j in range(N_KNN):
                head = dist[off[j]:off[j + 1]][:k]
                assert got[2][j, :len(head)].tobytes() == head.tobytes() and np.isposinf(got[2][j, len(head):]).all(), (n, k, j)
        ni, ns, nd = inst.nearest_masked_batch(pts, P)
        w1 = ipm.padded(ipm.knn_rows(c["scene"], pts, 1, M, P, cache), 1, dtype)
        _tuple_same((ni, ns, nd), tuple(x[:, 0] for x in w1), (n, "nearest"))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_knearest_tree_against_the_reference(eng, orc, ctx, dtype, n):
    """every k without a limit; a scalar limit, per-point limits and special_limits at k = 3 (per-point limits at k = 64 too)"""
    c, pts, cache = cluster(orc, dtype, n)
    pts = np.ascontiguousarray(pts[:N_KNN])
    M, P = inst_masks(n), point_masks(n, N_KNN)
    trees = _built_trees(eng, ctx, c["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst:
        inst.set_masks(M)
        pd, Pd = _dev(pts), _dev_mask(P)
        padding = 0
        for kind, ks in LIMIT_RUNS:
            lim = limits_of(kind, dtype, n, N_KNN)
            for k in ks:
                rows = ipm.knn_tree_rows(c["scene"], pts, k, M, P, lim, cache)
                want = ipm.padded(rows, k, dtype)
                _tuple_same(_padded(inst.knearest_tree_masked_batch(pts, k, P, lim)), want, (n, kind, k, "host"))
                _tuple_same(_padded(inst.knearest_tree_masked_batch(pd, k, Pd, _side(lim, True))), want, (n, kind, k, "device"))
                if kind == "none":                            # the distances are the flat form's, pairs aside
                    flat = _padded(inst.knearest_masked_batch(pts, k, P))
                    assert flat[2].tobytes() == want[2].tobytes(), (n, k)
                padding += sum(1 for r in rows if not r) if kind == "drawn" else 0
        assert n != 37 or padding >= 20
        lim = limits_of("drawn", dtype, n, N_KNN)
        w1 = ipm.padded(ipm.knn_tree_rows(c["scene"], pts, 1, M, P, lim, cache), 1, dtype)
        _tuple_same(inst.nearest_tree_masked_batch(pts, P, lim), tuple(x[:, 0] for x in w1), (n, "nearest"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene_ties_at_the_cut(eng, orc, ctx, dtype):
    """the row mask HIGH sees instance 0 and not its coincident copy 64: a cut through the twin keeps the visible pair, in both forms"""
    L = line_case(dtype)
    sc, pts, M, P = L["scene"], L["points"], L["M"], L["P"]
    trees = _built_trees(eng, ctx, L["trees"])
    with eng.Instances(trees, L["tree_of"], L["x"], ctx) as inst:
        inst.set_masks(M)
        for k in (1, 2, 3, 4, 7, 64):
            want = ipm.padded(ipm.knn_rows(sc, pts, k, M, P, L["cache"]), k, dtype)
            _tuple_same(_padded(inst.knearest_masked_batch(pts, k, P)), want, ("flat", k))
            assert (want[0][0::2] != 64).all() and (want[0][0::2, 0] == 0).all()
            want = ipm.padded(ipm.knn_tree_rows(sc, pts, k, M, P, None, L["cache"]), k, dtype)
            _tuple_same(_padded(inst.knearest_tree_masked_batch(_dev(pts), k, _dev_mask(P))), want, ("tree", k))
        lim = np.full(LINE_N, 3.0, dtype=dtype)
        rows = ipm.within_filter(iwr.rows(sc, pts, lim), M, P)
        for sort in (True, False):
            _tuple_same(_within(inst.within_masked_batch(pts, lim, P, sort=sort)), iwr.csr(rows, dtype, sort), ("within", sort))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("member", "top"))
def test_empty_child_bounds(eng, orc, ctx, dtype, which):
    import instances_knn_tree_ref as iktr
    sc, member, x, pts = iktr.far_member_scene(dtype) if which == "member" else iktr.coincident_scene(dtype)
    M = inst_masks(len(x))
    P = PAL[np.random.default_rng(770).integers(0, 10, len(pts))]
    trees = _built_trees(eng, ctx, [member])
    cache = {}
    with eng.Instances(trees, [0] * len(x), x, ctx) as inst:
        inst.set_masks(M)
        for k in (1, 7):
            want = ipm.padded(ipm.knn_tree_rows(sc, pts, k, M, P, None, cache), k, dtype)
            _tuple_same(_padded(inst.knearest_tree_masked_batch(pts, k, P)), want, (which, k, "tree"))
            want = ipm.padded(ipm.knn_rows(sc, pts, k, M, P, cache), k, dtype)
            _tuple_same(_padded(inst.knearest_masked_batch(pts, k, P)), want, (which, k, "flat"))


# ---- 3. region -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_under_every_flag_combination(eng, orc, ctx, dtype):
    """the main scene's 52 regions under every combination of classify / count_only / instances_only, HOST and HBM; every masked row is the
    unmasked row of the same run filtered in numpy; one region given as (m, 4); a scalar mask"""
    m, M, P, w = region_want(dtype)
    planes, nq = m["planes"], len(m["planes"])
    trees = _gpu_trees(eng, ctx, m["trees"])
    with eng.Instances(trees, m["tree_of"], m["x"], ctx) as inst:
        inst.set_masks(M)
        for device in (False, True):
            pl, pm = (_dev(planes), _dev_mask(P)) if device else (planes, P)
            for combo in COMBOS:
                got = _region(inst.region_masked_batch(pl, pm, **_region_kw(combo)))
                _region_same(got, _region_want(w, combo), (combo, device))
                if "count_only" not in combo:
                    free = _region(inst.region_batch(pl, **_region_kw(combo)))
                    _region_same(got, _filter_rows(free, M, P, nq), (combo, device, "anchor"))
        t = "float" if dtype == np.float32 else "double"
        inst.region_masked_batch(planes, P, classify=True)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_region_walk<{t}, false, false, true>"      # (the count walk: the one launch that looks at the masks)
        inst.region_batch(planes, classify=True)
        assert inst._hits.walk_kernel() == f"bvhgpu::k_instances_region_walk<{t}, true, true>"
        q = int(np.argmax(np.diff(w["full"][0].astype(np.int64))))
        one = ipm.region_filter(irr.reference(m["scene"], planes[q]), M, int(P[q]))
        assert one["full"][0][-1] >= 20
        for combo in ("classify", "instances_only_classify"):
            _region_same(_region(inst.region_masked_batch(planes[q], int(P[q]), **_region_kw(combo))), _region_want(one, combo), ("one region", combo))
        sc = ipm.region_filter(m["ref"], M, 0xC)
        _region_same(_region(inst.region_masked_batch(_dev(planes), 0xC, classify=True)), _region_want(sc, "classify"), "scalar")


# ---- 4. identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_ones_is_the_unmasked_entry(eng, orc, ctx, dtype):
    """mask=None and all ones equal every unmasked entry — on a fresh set, under real instance masks with set_masks(None) following them"""
    n = 37
    c, pts, cache = cluster(orc, dtype, n)
    pts = np.ascontiguousarray(pts[:N_KNN])
    md = limits_of("drawn", dtype, n, N_KNN)
    mr = irr.main_scene(dtype)
    ones_p, ones_q = np.full(N_KNN, ALL, np.uint32), np.full(len(mr["planes"]), ALL, np.uint32)

    def check(inst, rinst, label):
        for device in (False, True):
            p, d = (_dev(pts), _dev(md)) if device else (pts, md)
            for pm in (None, ALL, _dev_mask(ones_p) if device else ones_p):
                for kw in (dict(sort=True), dict(sort=False), dict(count_only=True)):
                    _tuple_same(_within(inst.within_masked_batch(p, d, pm, **kw)), _within(inst.within_batch(p, d, **kw)), (label, "within", kw))
                for k in (1, 9, 64):
                    _tuple_same(_padded(inst.knearest_masked_batch(p, k, pm)), _padded(inst.knearest_batch(p, k)), (label, "knn", k))
                    for lim in (None, d):
                        _tuple_same(_padded(inst.knearest_tree_masked_batch(p, k, pm, lim)), _padded(inst.knearest_tree_batch(p, k, lim)), (label, "tree", k))
            pl = _dev(mr["planes"]) if device else mr["planes"]
            for qm in (None, ALL, _dev_mask(ones_q) if device else ones_q):
                for combo in COMBOS:
                    _region_same(_region(rinst.region_masked_batch(pl, qm, **_region_kw(combo))), _region(rinst.region_batch(pl, **_region_kw(combo))),
                                 (label, combo))

    trees, rtrees = _built_trees(eng, ctx, c["trees"]), _gpu_trees(eng, ctx, mr["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances(rtrees, mr["tree_of"], mr["x"], ctx) as rinst:
        check(inst, rinst, "fresh")
        inst.set_masks(inst_masks(n)); rinst.set_masks(inst_masks(len(mr["x"])))
        got = _within(inst.within_masked_batch(pts, md, None))
        assert got[0][-1] < _within(inst.within_batch(pts, md))[0][-1]                  # (the real masks hide something)
        inst.set_masks(None); rinst.set_masks(None)
        check(inst, rinst, "after set_masks(None)")


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges(eng, orc, ctx, dtype):
    """all instance masks 0; all row masks 0; the one-instance set hidden; no instances; no rows; a scalar mask"""
    n, k = 37, 5
    c, pts, cache = cluster(orc, dtype, n)
    pts = np.ascontiguousarray(pts[:64])
    md = np.full(64, 3.0, dtype=dtype)
    mr = irr.main_scene(dtype)
    planes = mr["planes"]
    pad = (np.full((64, k), NONE, np.uint32), np.full((64, k), NONE, np.uint32), np.full((64, k), np.inf, dtype))
    zero = np.zeros(65, np.uint32)

    def all_hidden(inst, rinst, pm, qm, label):
        for device in (False, True):
            p, d, pl = (_dev(pts), _dev(md), _dev(planes)) if device else (pts, md, planes)
            pmd, qmd = (_dev_mask(pm), _dev_mask(qm)) if device else (pm, qm)
            got = _within(inst.within_masked_batch(p, d, pmd))
            assert got[0].tobytes() == zero.tobytes() and all(len(x) == 0 for x in got[1:]), label
            assert _within(inst.within_masked_batch(p, d, pmd, count_only=True))[0].tobytes() == zero.tobytes()
            _tuple_same(_padded(inst.knearest_masked_batch(p, k, pmd)), pad, (label, "knn"))
            _tuple_same(_padded(inst.knearest_tree_masked_batch(p, k, pmd, d)), pad, (label, "tree"))
            for combo in COMBOS:
                got = _region(rinst.region_masked_batch(pl, qmd, **_region_kw(combo)))
                assert not got[0].any() and len(got[0]) == len(planes) + 1 and len(got[1]) == 0, (label, combo)

    trees, rtrees = _built_trees(eng, ctx, c["trees"]), _gpu_trees(eng, ctx, mr["trees"])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances(rtrees, mr["tree_of"], mr["x"], ctx) as rinst:
        assert _within(inst.within_batch(pts, md))[0][-1] >= 20
        all_hidden(inst, rinst, np.zeros(64, np.uint32), np.zeros(len(planes), np.uint32), "row masks 0")
        all_hidden(inst, rinst, 0, 0, "scalar 0")
        inst.set_masks(np.zeros(n, np.uint32)); rinst.set_masks(np.zeros(len(mr["x"]), np.uint32))
        all_hidden(inst, rinst, None, None, "instance masks 0")
        all_hidden(inst, rinst, point_masks(n, 64), region_masks(len(planes)), "instance masks 0, drawn rows")
        # a scalar mask is that mask on every row
        M = inst_masks(n)
        inst.set_masks(M)
        rows = ipm.within_filter(iwr.rows(c["scene"], pts, md), M, 3)
        assert 0 < sum(len(r) for r in rows) < _within(inst.within_batch(pts, md))[0][-1]
        _tuple_same(_within(inst.within_masked_batch(pts, md, 3)), iwr.csr(rows, dtype), "scalar 3")
        _tuple_same(_within(inst.within_masked_batch(_dev(pts), 3.0, 3)), iwr.csr(rows, dtype), "scalar 3, device")
        _tuple_same(_padded(inst.knearest_masked_batch(_dev(pts), k, HIGH)), ipm.padded(ipm.knn_rows(c["scene"], pts, k, M, HIGH, {}), k, dtype), "scalar HIGH")
        _tuple_same(_padded(inst.knearest_tree_masked_batch(pts, k, HIGH)), ipm.padded(ipm.knn_tree_rows(c["scene"], pts, k, M, HIGH, None, {}), k, dtype),
                    "scalar HIGH, tree")
        # no rows
        for p, pm in ((np.zeros((0, 3), dtype), np.zeros(0, np.uint32)), (np.zeros((0, 3), dtype), None)):
            got = _within(inst.within_masked_batch(p, np.zeros(0, dtype), pm))
            assert got[0].tolist() == [0] and len(got[1]) == 0
            assert all(x.shape == (0, k) for x in _padded(inst.knearest_masked_batch(p, k, pm)))
            assert all(x.shape == (0, k) for x in _padded(inst.knearest_tree_masked_batch(p, k, pm)))
        got = _region(rinst.region_masked_batch(np.zeros((0, 6, 4), dtype), None, classify=True))
        assert got[0].tolist() == [0] and len(got[1]) == 0
    # the one-instance set, hidden and seen
    c1, p1, _ = cluster(orc, dtype, 1)
    p1 = np.ascontiguousarray(p1[:64])
    t1 = _built_trees(eng, ctx, c1["trees"])
    with eng.Instances(t1, c1["tree_of"], c1["x"], ctx) as one:
        one.set_masks(np.array([4], np.uint32))
        _tuple_same(_padded(one.knearest_masked_batch(p1, k, 3)), pad, "one hidden")
        _tuple_same(_padded(one.knearest_tree_masked_batch(p1, k, 3)), pad, "one hidden, tree")
        assert _within(one.within_masked_batch(p1, np.inf, 3))[0][-1] == 0
        assert _region(one.region_masked_batch(np.zeros((1, 0, 4), dtype), 3))[0].tolist() == [0, 0]
        _tuple_same(_padded(one.knearest_masked_batch(p1, k, 6)), _padded(one.knearest_batch(p1, k)), "one seen")
        _tuple_same(_padded(one.knearest_tree_masked_batch(p1, k, 6)), _padded(one.knearest_tree_batch(p1, k)), "one seen, tree")
        assert _region(one.region_masked_batch(np.zeros((1, 0, 4), dtype), 6, instances_only=True))[1].tolist() == [0]
    # no instances
    with eng.Instances(t1, np.zeros(0, dtype=np.uint32), np.zeros((0, 3, 4), dtype=dtype), ctx) as empty:
        P = point_masks(37, 64)
        _tuple_same(_padded(empty.knearest_masked_batch(p1, k, P)), pad, "empty")
        _tuple_same(_padded(empty.knearest_tree_masked_batch(_dev(p1), k, _dev_mask(P))), pad, "empty, tree")
        assert _within(empty.within_masked_batch(p1, 1.0, P))[0].tobytes() == zero.tobytes()
        for combo in COMBOS:
            assert not _region(empty.region_masked_batch(planes, None, **_region_kw(combo)))[0].any()


# ---- 6. lifetime ---------------------------------------------------------------------------------------------------------------------------
def test_masks_survive_update_and_stale_sets_refuse(eng, orc, ctx):
    import instances_ref as ir
    from bvh_amd._lib import INVALID_ARG, BvhGpuError
    dtype, ni, k = np.float32, 12, 4
    b_aabbs, b_tris = member_trees(orc, dtype)[1]
    member = eng.Bvh.from_aabbs(b_aabbs, ctx)
    member.flatten_in_place()
    member.set_triangles(b_tris)
    x, x2 = transforms(ni, dtype, 990), transforms(ni, dtype, 991)
    rng = np.random.default_rng(992)
    pts = rng.uniform(-9, 9, size=(80, 3)).astype(dtype)
    md = np.full(80, 2.5, dtype=dtype)
    M, P = inst_masks(ni), PAL[rng.integers(0, 10, 80)]
    planes = irr.rr.random_regions(ir.Scene([(b_aabbs, b_tris)], [0] * ni, x2, dtype).w, 8, 993)
    Q = PAL[[0, 1, 4, 6, 7, 8, 9, 2]]
    with eng.Instances([member], [0] * ni, x, ctx) as inst:
        inst.set_masks(M)
        inst.update(x2)
        assert inst.masks.tobytes() == M.tobytes()
        sc = ir.Scene([(b_aabbs, b_tris)], [0] * ni, x2, dtype)
        rows = ipm.within_filter(iwr.rows(sc, pts, md), M, P)
        assert 20 <= sum(len(r) for r in rows) < sum(len(r) for r in iwr.rows(sc, pts, md))
        _tuple_same(_within(inst.within_masked_batch(pts, md, P)), iwr.csr(rows, dtype), "re-posed within")
        _tuple_same(_padded(inst.knearest_masked_batch(pts, k, P)), ipm.padded(ipm.knn_rows(sc, pts, k, M, P, {}), k, dtype), "re-posed knn")
        _tuple_same(_padded(inst.knearest_tree_masked_batch(pts, k, P, md)), ipm.padded(ipm.knn_tree_rows(sc, pts, k, M, P, md, {}), k, dtype), "re-posed tree")
        w = ipm.region_filter(irr.reference(sc, planes), M, Q)
        _region_same(_region(inst.region_masked_batch(planes, Q, classify=True)), _region_want(w, "classify"), "re-posed region")
        calls = (lambda: inst.within_masked_batch(pts, md, P), lambda: inst.knearest_masked_batch(pts, k, P),
                 lambda: inst.knearest_tree_masked_batch(pts, k, P), lambda: inst.region_masked_batch(planes, Q),
                 lambda: inst.region_masked_batch(planes, Q, instances_only=True))
        bad = x.copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(BvhGpuError):
            inst.update(bad)
        for call in calls:
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == INVALID_ARG and "not committed" in str(e.value)
        inst.update(x2)
        member.rebuild(b_aabbs[:100], flatten=True)
        for call in calls + (lambda: inst.within_batch(pts, md),):
            with pytest.raises(BvhGpuError) as e:
                call()
            assert e.value.status == INVALID_ARG and "instances are stale: call bvhgpu_instances_update" in str(e.value)
        member.set_triangles(b_tris[:100])
        inst.update(x2)
        assert inst.masks.tobytes() == M.tobytes()
        sc3 = ir.Scene([(b_aabbs[:100], b_tris[:100])], [0] * ni, x2, dtype)
        _tuple_same(_padded(inst.knearest_masked_batch(pts, k, P)), ipm.padded(ipm.knn_rows(sc3, pts, k, M, P, {}), k, dtype), "the new generation")


# ---- 7. the refusals of the raw C ABI ------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(eng, orc, ctx):
    """each of the eight symbols against its counterpart: the same status and, word for word, the same message; sentinels untouched; *hits as
    it was"""
    from bvh_amd import _lib
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, OK, OVERFLOW, ptr
    lib = _lib.load()
    dtype, k, n = np.float32, 5, 64
    c, pts, cache = cluster(orc, dtype, 37)
    pts = np.ascontiguousarray(pts[:n])
    pts64 = pts.astype(np.float64)
    md, md64 = np.full(n, 2.5, dtype), np.full(n, 2.5, np.float64)
    mr = irr.main_scene(dtype)
    planes = np.ascontiguousarray(mr["planes"][:8])
    planes64 = planes.astype(np.float64)
    mp = planes.shape[1]
    M, P = inst_masks(37), point_masks(37, n)
    SENT = 0xABABABAB
    oi, os_, od, od64 = np.full((n, 64), SENT, np.uint32), np.full((n, 64), SENT, np.uint32), np.full((n, 64), 7.0, dtype), np.full((n, 64), 7.0, np.float64)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def untouched():
        assert (oi == SENT).all() and (os_ == SENT).all() and (od == 7.0).all() and (od64 == 7.0).all()

    trees = _built_trees(eng, ctx, c["trees"])
    uploaded = eng.FlatBvh.from_flat_nodes(c["scene"].flats[0], c["trees"][0][0], ctx)       # no BvhNode array: the tree form refuses it
    uploaded.set_triangles(c["trees"][0][1])
    member = eng.Bvh.from_aabbs(c["trees"][0][0], ctx)
    member.flatten_in_place()
    member.set_triangles(c["trees"][0][1])
    with eng.Instances(trees, c["tree_of"], c["x"], ctx) as inst, eng.Instances([member], [0] * 37, c["x"], ctx) as stale, \
            eng.Instances(trees, c["tree_of"], c["x"], ctx) as broken, eng.Instances([uploaded], [0] * 37, c["x"], ctx) as flat_only:
        member.rebuild(c["trees"][1][0][:100], flatten=True)
        bad = c["x"].copy()
        bad[1, 0, 0] = np.nan
        with pytest.raises(_lib.BvhGpuError):
            broken.update(bad)
        inst.set_masks(M)
        s, S, B, U = inst._s, stale._s, broken._s, flat_only._s
        Pp, P64, Dp, D64, Mp, I, Sh, Dd, Dd64 = ptr(pts), ptr(pts64), ptr(md), ptr(md64), ptr(P), ptr(oi), ptr(os_), ptr(od), ptr(od64)
        Lp, L64 = ptr(planes), ptr(planes64)
        UNC, STALE = "instances are not committed", "instances are stale: call bvhgpu_instances_update"

        def both(plain, masked, at, args, status, text):
            """the unmasked entry and its masked form (the mask at position `at`) refuse alike: status, message, nothing written"""
            rc0 = plain(*args)
            e0 = err()
            rc1 = masked(*args[:at], Mp, *args[at:])
            assert rc0 == rc1 == status and err() == e0 and text in e0, (rc0, rc1, e0, err())
            assert masked(*args[:at], None, *args[at:]) == status and err() == e0
            untouched()

        # ---- knearest: a NULL set; k; a NULL argument; mem; dtype; uncommitted; stale; the size ----
        k32, k64 = lib.bvhgpu_instances_knearest_f32, lib.bvhgpu_instances_knearest_f64
        km32, km64 = lib.bvhgpu_instances_knearest_masked_f32, lib.bvhgpu_instances_knearest_masked_f64
        assert km32(None, Pp, Mp, n, HOST, k, I, Sh, Dd) == INVALID_ARG == k32(None, Pp, n, HOST, k, I, Sh, Dd)
        untouched()
        for args, status, text in (
                ((s, Pp, n, HOST, 0, I, Sh, Dd), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KNN_MAX_K"),
                ((s, Pp, n, HOST, 65, I, Sh, Dd), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KNN_MAX_K"),
                ((s, None, n, HOST, k, I, Sh, Dd), INVALID_ARG, "NULL argument"), ((s, Pp, n, HOST, k, None, Sh, Dd), INVALID_ARG, "NULL argument"),
                ((s, Pp, n, HOST, k, I, None, Dd), INVALID_ARG, "NULL argument"), ((s, Pp, n, HOST, k, I, Sh, None), INVALID_ARG, "NULL argument"),
                ((s, Pp, n, 7, k, I, Sh, Dd), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                ((B, Pp, n, HOST, k, I, Sh, Dd), INVALID_ARG, UNC), ((S, Pp, n, HOST, k, I, Sh, Dd), INVALID_ARG, STALE),
                ((s, Pp, 1 << 26, HOST, 64, I, Sh, Dd), OVERFLOW, "too many results (points x k)"),
                ((S, None, 0xFFFFFFFF, 7, 0, I, Sh, Dd), INVALID_ARG, "k must be"), ((S, None, 0xFFFFFFFF, 7, k, I, Sh, Dd), INVALID_ARG, "NULL argument"),
                ((S, Pp, 0xFFFFFFFF, 7, k, I, Sh, Dd), INVALID_ARG, "mem must be"), ((B, Pp, 0xFFFFFFFF, HOST, k, I, Sh, Dd), INVALID_ARG, UNC),
                ((S, Pp, 0xFFFFFFFF, HOST, k, I, Sh, Dd), INVALID_ARG, STALE)):
            both(k32, km32, 2, args, status, text)
        both(k64, km64, 2, (s, P64, n, HOST, k, I, Sh, Dd64), DTYPE_MISMATCH, "dtype")
        assert km32(s, None, None, 0, HOST, k, None, None, None) == OK
        # ---- knearest_tree: the same, a member without a BvhNode array besides ----
        t32, t64 = lib.bvhgpu_instances_knearest_tree_f32, lib.bvhgpu_instances_knearest_tree_f64
        tm32, tm64 = lib.bvhgpu_instances_knearest_tree_masked_f32, lib.bvhgpu_instances_knearest_tree_masked_f64
        assert tm32(None, Pp, Mp, n, HOST, k, Dp, I, Sh, Dd) == INVALID_ARG == t32(None, Pp, n, HOST, k, Dp, I, Sh, Dd)
        untouched()
        for args, status, text in (
                ((s, Pp, n, HOST, 0, Dp, I, Sh, Dd), INVALID_ARG, "k must be between 1 and BVHGPU_INSTANCES_KNN_MAX_K"),
                ((s, Pp, n, HOST, 65, None, I, Sh, Dd), INVALID_ARG, "k must be"),
                ((s, None, n, HOST, k, Dp, I, Sh, Dd), INVALID_ARG, "NULL argument"), ((s, Pp, n, HOST, k, Dp, None, Sh, Dd), INVALID_ARG, "NULL argument"),
                ((s, Pp, n, HOST, k, None, I, None, Dd), INVALID_ARG, "NULL argument"), ((s, Pp, n, HOST, k, Dp, I, Sh, None), INVALID_ARG, "NULL argument"),
                ((s, Pp, n, 7, k, Dp, I, Sh, Dd), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                ((B, Pp, n, HOST, k, Dp, I, Sh, Dd), INVALID_ARG, UNC), ((S, Pp, n, HOST, k, Dp, I, Sh, Dd), INVALID_ARG, STALE),
                ((U, Pp, n, HOST, k, Dp, I, Sh, Dd), INVALID_ARG, "the nearest-first descent needs the BvhNode array of every member tree"),
                ((s, Pp, 1 << 26, HOST, 64, Dp, I, Sh, Dd), OVERFLOW, "too many results (points x k)"),
                ((U, None, 0xFFFFFFFF, 7, 0, Dp, I, Sh, Dd), INVALID_ARG, "k must be"), ((U, None, 0xFFFFFFFF, 7, k, Dp, I, Sh, Dd), INVALID_ARG, "NULL argument"),
                ((U, Pp, 0xFFFFFFFF, 7, k, Dp, I, Sh, Dd), INVALID_ARG, "mem must be"), ((U, Pp, 0xFFFFFFFF, HOST, k, Dp, I, Sh, Dd), INVALID_ARG, "BvhNode array")):
            both(t32, tm32, 2, args, status, text)
        both(t64, tm64, 2, (s, P64, n, HOST, k, D64, I, Sh, Dd64), DTYPE_MISMATCH, "dtype")
        assert tm32(s, None, None, 0, HOST, k, None, None, None, None) == OK
        # ---- within: a NULL set; hits; points; max_dist; mem; dtype; flags; uncommitted; stale; the batch size.  *hits stays as it was ----
        w32, w64 = lib.bvhgpu_instances_within_f32, lib.bvhgpu_instances_within_f64
        wm32, wm64 = lib.bvhgpu_instances_within_masked_f32, lib.bvhgpu_instances_within_masked_f64
        r32, r64 = lib.bvhgpu_instances_region_f32, lib.bvhgpu_instances_region_f64
        rm32, rm64 = lib.bvhgpu_instances_region_masked_f32, lib.bvhgpu_instances_region_masked_f64
        h = C.c_void_p()
        assert wm32(None, Pp, Dp, Mp, n, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        assert rm32(None, Lp, Mp, 8, mp, HOST, 0, C.byref(h)) == INVALID_ARG and not h.value
        both(w32, wm32, 3, (s, Pp, Dp, n, HOST, 0, None), INVALID_ARG, "hits is NULL")
        both(r32, rm32, 2, (s, Lp, 8, mp, HOST, 0, None), INVALID_ARG, "hits is NULL")
        for keep in (None, "made"):
            if keep:
                assert wm32(s, Pp, Dp, Mp, n, HOST, 0, C.byref(h)) == OK and h.value
                keep = h.value
            for args, status, text in (
                    ((s, None, Dp, n, HOST, 0, C.byref(h)), INVALID_ARG, "points is NULL"), ((s, Pp, None, n, HOST, 0, C.byref(h)), INVALID_ARG, "max_dist is NULL"),
                    ((s, Pp, Dp, n, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                    ((s, Pp, Dp, n, HOST, 4, C.byref(h)), INVALID_ARG, "instance within flags"),
                    ((B, Pp, Dp, n, HOST, 0, C.byref(h)), INVALID_ARG, UNC), ((S, Pp, Dp, n, HOST, 0, C.byref(h)), INVALID_ARG, STALE),
                    ((s, Pp, Dp, 0xFFFFFFFF, HOST, 0, C.byref(h)), OVERFLOW, "points"),
                    ((S, None, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "points is NULL"), ((S, Pp, None, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "max_dist is NULL"),
                    ((S, Pp, Dp, 0xFFFFFFFF, 7, 8, C.byref(h)), INVALID_ARG, "mem must be"), ((S, Pp, Dp, 0xFFFFFFFF, HOST, 8, C.byref(h)), INVALID_ARG, "instance within flags"),
                    ((B, Pp, Dp, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, UNC), ((S, Pp, Dp, 0xFFFFFFFF, HOST, 3, C.byref(h)), INVALID_ARG, STALE)):
                both(w32, wm32, 3, args, status, text)
                assert h.value == keep
            both(w64, wm64, 3, (s, P64, D64, n, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "dtype")
            # ---- region: planes; m; mem; dtype; flags; uncommitted; stale; the batch size ----
            for args, status, text in (
                    ((s, None, 8, mp, HOST, 0, C.byref(h)), INVALID_ARG, "planes is NULL"), ((s, Lp, 8, 33, HOST, 0, C.byref(h)), INVALID_ARG, "more than BVHGPU_REGION_MAX_PLANES planes per region"),
                    ((s, Lp, 8, mp, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE"),
                    ((s, Lp, 8, mp, HOST, 8, C.byref(h)), INVALID_ARG, "instance region flags"),
                    ((B, Lp, 8, mp, HOST, 0, C.byref(h)), INVALID_ARG, UNC), ((S, Lp, 8, mp, HOST, 0, C.byref(h)), INVALID_ARG, STALE),
                    ((B, Lp, 8, mp, HOST, 4, C.byref(h)), INVALID_ARG, UNC), ((S, Lp, 8, mp, HOST, 5, C.byref(h)), INVALID_ARG, STALE),
                    ((s, Lp, 0xFFFFFFFF, mp, HOST, 0, C.byref(h)), OVERFLOW, "regions"),
                    ((S, None, 0xFFFFFFFF, 33, 7, 8, C.byref(h)), INVALID_ARG, "planes per region"), ((S, Lp, 0xFFFFFFFF, mp, 7, 8, C.byref(h)), INVALID_ARG, "mem must be"),
                    ((S, Lp, 0xFFFFFFFF, mp, HOST, 8, C.byref(h)), INVALID_ARG, "instance region flags"), ((S, Lp, 0xFFFFFFFF, mp, HOST, 7, C.byref(h)), INVALID_ARG, STALE)):
                both(r32, rm32, 2, args, status, text)
                assert h.value == keep
            both(r64, rm64, 2, (s, L64, 8, mp, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "dtype")
            assert h.value == keep
        # the result object the refused batches left alone still holds the masked within batch made before: read by the unmasked family's fetch
        rows = ipm.within_filter(iwr.rows(c["scene"], pts, md), M, P)
        want = iwr.csr(rows, dtype)
        tot = int(want[0][-1])
        assert tot >= 20
        nr, got_tot = C.c_size_t(), C.c_uint64()
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(got_tot), None) == OK and (nr.value, got_tot.value) == (n, tot)
        off, gi, gs, gd = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint32), np.zeros(tot, np.uint32), np.zeros(tot, dtype)
        assert lib.bvhgpu_hits_fetch_instances_within(h, ptr(off), ptr(gi), ptr(gs), ptr(gd), HOST) == OK
        _tuple_same((off, gi, gs, gd), want, "fetched by the unmasked family's entry")
        assert lib.bvhgpu_hits_fetch_within(h, ptr(off), ptr(gs), ptr(gd), HOST) == INVALID_ARG
        # ... and the same object takes a masked region batch, read by bvhgpu_hits_fetch_instances_region
        Q = region_masks(8)
        Q[1] = ALL
        assert rm32(s, Lp, ptr(Q), 8, mp, HOST, 4, C.byref(h)) == OK
        wr_ = ipm.region_filter(irr.reference(c["scene"], planes), M, Q)["top"]
        off8, gi = np.zeros(9, np.uint32), np.zeros(int(wr_[0][-1]), np.uint32)
        assert lib.bvhgpu_hits_fetch_instances_region(h, ptr(off8), ptr(gi), None, None, HOST) == OK
        assert off8.tobytes() == wr_[0].tobytes() and gi.tobytes() == wr_[1].tobytes()
        lib.bvhgpu_hits_destroy(h)
        untouched()
        # a later valid call still answers, on the set that refused
        gi, gs, gd = np.zeros((n, k), np.uint32), np.zeros((n, k), np.uint32), np.zeros((n, k), dtype)
        assert km32(s, Pp, Mp, n, HOST, k, ptr(gi), ptr(gs), ptr(gd)) == OK
        _tuple_same((gi, gs, gd), ipm.padded(ipm.knn_rows(c["scene"], pts, k, M, P, {}), k, dtype), "after the refusals")
