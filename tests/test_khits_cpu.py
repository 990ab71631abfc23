"""Multi-hit ray queries on the CPU: the new entry points are declared, exported and bound in every layer; the definition the GPU tests
pin (tests/khits_ref.py; include/bvh_mi355x.h, bvhgpu_traverse_khits_*) is checked on hand-made rows and, at k = 1, against the closest
queries' definitions; and the scenes of tests/test_gpu_khits.py are shown — on the oracle alone — to truncate, tie and reverse, so that the
GPU tests cannot pass vacuously."""
import os
import re
import subprocess

import numpy as np
import pytest

import khits_ref as kr
from sphere_ref import cluster_rays, cluster_scene, list_hits, sphere_match
from test_box_hit_cpu import box_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_traverse_khits_f32", "bvhgpu_traverse_khits_f64"]
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
INF = np.inf


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


# ---- 1. every layer --------------------------------------------------------------------------------------------------------
def test_new_functions_in_every_layer():
    raw = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    h = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), f"{name} is not declared in the header"
    for name, value in (("BVHGPU_KHITS_MAX_K", "64u"), ("BVHGPU_LEAF_BOX", "0"), ("BVHGPU_LEAF_TRIANGLE", "1"), ("BVHGPU_LEAF_SPHERE", "2")):
        assert re.search(r"#define %s %s\b" % (name, value), h), name
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define BVHGPU_KHITS_MAX_K", raw, flags=re.S)
    assert m, "bvhgpu_traverse_khits_* has no comment in front of it"
    text = " ".join(m.group(1).split())
    for word in ("BVHGPU_NONE", "+inf", "stable", "strict", "BVHGPU_KHITS_MAX_K", "Padding", "No pruning"):
        assert word in text, word
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in bound, f"{name} missing from _lib.SYMBOLS"
        assert hasattr(lib, name) and re.search(r" T %s\b" % name, nm), f"{name} not exported"
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"k_ray_khits" in blob and b"k_khits_fill" in blob
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} missing from ffi.rs"
        assert name in lib_rs, f"{name} is no impl_gpu_scalar! entry"
    for const in ("BVHGPU_KHITS_MAX_K: u32 = 64", "BVHGPU_LEAF_BOX: c_int = 0", "BVHGPU_LEAF_TRIANGLE: c_int = 1", "BVHGPU_LEAF_SPHERE: c_int = 2"):
        assert "pub const " + const in ffi, const
    assert "pub fn traverse_khits(" in lib_rs
    from bvh_amd.api import Bvh, _TreeBase
    assert callable(getattr(_TreeBase, "khits_batch", None)) and "khits_batch" in Bvh.__dict__
    assert _lib.KHITS_MAX_K == 64 and (_lib.LEAF_BOX, _lib.LEAF_TRIANGLE, _lib.LEAF_SPHERE) == (0, 1, 2)
    assert _lib.LEAF_KINDS == {"box": 0, "triangle": 1, "sphere": 2}
    from bvh_amd import build_ext
    assert "khits.hip" in build_ext.SOURCES


# ---- 2. the definition on hand-made rows ------------------------------------------------------------------------------------
def _rows(dtype, w=2):
    """four rays: [5, 3, 3, inf, 1, 3] (shapes 10..15), [], [2, 2] (shapes 7, 4), [inf] (shape 9); the second scalar is 100 + shape"""
    off = np.array([0, 6, 6, 8, 9], dtype=np.uint32)
    idx = np.array([10, 11, 12, 13, 14, 15, 7, 4, 9], dtype=np.uint32)
    rec = np.zeros((9, w), dtype=dtype)
    rec[:, 0] = [5, 3, 3, INF, 1, 3, 2, 2, INF]
    rec[:, 1] = 100 + idx
    if w == 3:
        rec[:, 2] = 200 + idx
    return off, idx, rec


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [2, 3])
def test_khits_match_on_hand_made_rows(dtype, w):
    off, idx, rec = _rows(dtype, w)
    pad = [INF, 0] + [0] * (w - 2)

    def record(s):
        return [float(rec[list(idx).index(s), 0]), 100 + s] + ([200 + s] if w == 3 else [])

    # k larger than any row: the whole sorted rows, ties (3, 3, 3: shapes 11, 12, 15; 2, 2: shapes 7, 4) in list order, then padding
    vals, shape = kr.khits_match(off, idx, rec, None, 6)
    assert vals.dtype == dtype and vals.shape == (4, 6, w) and shape.dtype == np.uint32 and shape.shape == (4, 6)
    assert shape.tolist() == [[14, 11, 12, 15, 10, NONE], [NONE] * 6, [7, 4] + [NONE] * 4, [NONE] * 6]
    assert vals[0].tolist() == [record(14), record(11), record(12), record(15), record(10), pad]
    assert vals[1].tolist() == [pad] * 6 and vals[3].tolist() == [pad] * 6            # an empty row, and a row of misses
    assert vals[2].tolist() == [record(7), record(4)] + [pad] * 4
    # truncation at k: inside the tie (k = 3 keeps 11 and 12, drops 15), and k = 1
    vals, shape = kr.khits_match(off, idx, rec, None, 3)
    assert shape.tolist() == [[14, 11, 12], [NONE] * 3, [7, 4, NONE], [NONE] * 3]
    assert vals[0].tolist() == [record(14), record(11), record(12)]
    vals, shape = kr.khits_match(off, idx, rec, None, 1)
    assert shape.tolist() == [[14], [NONE], [7], [NONE]] and vals[2].tolist() == [record(7)]
    # tmax is strict: tmax == distance admits nothing at that distance
    vals, shape = kr.khits_match(off, idx, rec, np.array([3, 3, 2, INF], dtype=dtype), 4)
    assert shape.tolist() == [[14, NONE, NONE, NONE], [NONE] * 4, [NONE] * 4, [NONE] * 4]
    assert vals[0].tolist() == [record(14), pad, pad, pad] and vals[2].tolist() == [pad] * 4
    above = np.nextafter(dtype(3), dtype(4))
    vals, shape = kr.khits_match(off, idx, rec, np.array([above, 0, above, 1], dtype=dtype), 4)
    assert shape.tolist() == [[14, 11, 12, 15], [NONE] * 4, [7, 4, NONE, NONE], [NONE] * 4]
    # NaN, zero and negative tmax admit nothing; +inf admits every hit but no miss
    for t in (np.nan, 0.0, -0.0, -1.0, -INF):
        vals, shape = kr.khits_match(off, idx, rec, np.full(4, t, dtype=dtype), 2)
        assert np.all(shape == NONE) and vals.tolist() == [[pad] * 2] * 4, t
    vals, shape = kr.khits_match(off, idx, rec, np.full(4, INF, dtype=dtype), 6)
    assert shape[0].tolist() == [14, 11, 12, 15, 10, NONE] and np.all(shape[3] == NONE)
    assert kr.candidate_counts(off, rec).tolist() == [5, 0, 2, 0]
    assert kr.candidate_counts(off, rec, np.array([3, 3, 2.5, INF], dtype=dtype)).tolist() == [1, 0, 2, 0]
    # no rays at all
    vals, shape = kr.khits_match(np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, w), dtype), None, 5)
    assert vals.shape == (0, 5, w) and shape.shape == (0, 5)


def test_khits_match_equals_the_incremental_form():
    """the list the kernel runs — enter while not full; a full list accepts d iff d < L[k-1] and drops L[k-1]; d goes in front of the
    first e with d < e — gives the stable sort cut to k, on rows of few distinct values (many ties)"""
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 40, size=200)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    total = int(off[-1])
    idx = rng.permutation(total).astype(np.uint32)
    rec = np.zeros((total, 2), dtype=np.float32)
    rec[:, 0] = rng.choice([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, INF], size=total)
    rec[:, 1] = idx
    tmax = rng.choice([0.0, 1.0, 2.0, 3.0, INF, np.nan], size=200).astype(np.float32)
    for k in (1, 2, 5, 64):
        vals, shape = kr.khits_match(off, idx, rec, tmax, k)
        for r in range(200):
            L = []
            for m in range(off[r], off[r + 1]):
                d = rec[m, 0]
                if not d < tmax[r]:
                    continue
                if len(L) == k:
                    if not d < L[-1][0]:
                        continue
                    L.pop()
                pos = next((j for j, e in enumerate(L) if d < e[0]), len(L))
                L.insert(pos, (d, int(idx[m])))
            assert shape[r, :len(L)].tolist() == [s for _, s in L] and np.all(shape[r, len(L):] == NONE), (k, r)
            assert vals[r, :len(L), 0].tolist() == [d for d, _ in L] and np.all(np.isposinf(vals[r, len(L):, 0]))


# ---- the scenes of the GPU tests, on the oracle ---------------------------------------------------------------------------------
_CACHE = {}


def cluster_case(orc, dtype):
    """the cluster scene's CSR and records, computed once per dtype: dict(spheres, aabbs, rays, rng, off, idx, box, sphere)"""
    key = ("cluster", np.dtype(dtype).name)
    if key not in _CACHE:
        from bvh_amd import spheres_aabbs
        centres, spheres = cluster_scene(dtype)
        rays, rng = cluster_rays(orc, centres, 20000, dtype, seed=9)
        aabbs = spheres_aabbs(spheres)
        oflat = orc.flatten(orc.build(aabbs).nodes)
        off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
        _CACHE[key] = dict(spheres=spheres, aabbs=aabbs, rays=rays, rng=rng, off=off, idx=idx, box=ts, sphere=list_hits(off, idx, rays, spheres))
    return _CACHE[key]


def pair_row_case(orc, dtype):
    key = ("pairs", np.dtype(dtype).name)
    if key not in _CACHE:
        spheres, aabbs = kr.nested_pair_row(dtype)
        rays = kr.row_rays(orc, dtype)
        oflat = orc.flatten(orc.build(aabbs).nodes)
        off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True)
        _CACHE[key] = dict(spheres=spheres, aabbs=aabbs, rays=rays, oflat=oflat, off=off, idx=idx, box=ts, sphere=list_hits(off, idx, rays, spheres))
    return _CACHE[key]


def triangle_row_case(orc, dtype, alternate):
    key = ("tris", np.dtype(dtype).name, alternate)
    if key not in _CACHE:
        tris, aabbs = kr.triangle_row(dtype, alternate)
        rays = kr.row_rays(orc, dtype, z=-0.5)
        oflat = orc.flatten(orc.build(aabbs).nodes)
        off, idx, _, _ = orc.traverse_flat(oflat, aabbs, rays)
        isect, closest, prim = orc.triangle_stage(tris, rays, off, idx)
        _CACHE[key] = dict(tris=tris, aabbs=aabbs, rays=rays, off=off, idx=idx, triangle=isect, closest=closest, prim=prim)
    return _CACHE[key]


def cube_case(orc, dtype, rays_kind):
    """orc.create_n_cubes(1000) (12 000 triangles) with 20 000 rays: "stream" = orc.create_rays, "aimed" = rays aimed at the cubes"""
    key = ("cubes", np.dtype(dtype).name, rays_kind)
    if key not in _CACHE:
        tris32, aabbs32 = orc.create_n_cubes(1000)
        tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
        if rays_kind == "stream":
            rays = orc.create_rays(0, 20000, dtype=dtype)
        else:
            from test_gpu_any_hit import _aimed_rays
            rays, _ = _aimed_rays(orc, tris, 20000, dtype, seed=5)
        off, idx, _, _ = orc.traverse_flat(orc.flatten(orc.build(aabbs).nodes), aabbs, rays, threads=orc.max_threads())
        isect, closest, prim = orc.triangle_stage(tris, rays, off, idx)
        _CACHE[key] = dict(tris=tris, aabbs=aabbs, rays=rays, off=off, idx=idx, triangle=isect, closest=closest, prim=prim)
    return _CACHE[key]


def _tie_pairs(off, idx, vals, shape, r, upto=64):
    """adjacent equal finite distances among the first `upto` slots of row r → (pairs, pairs whose later member has the lower shape index);
    asserts that each pair stands in list order"""
    lst = idx[off[r]:off[r + 1]].tolist()
    pairs = lower = 0
    for j in range(min(upto, shape.shape[1]) - 1):
        if np.isfinite(vals[r, j, 0]) and vals[r, j, 0] == vals[r, j + 1, 0]:
            assert lst.index(shape[r, j]) < lst.index(shape[r, j + 1]), (r, j)
            pairs += 1
            lower += int(shape[r, j + 1] < shape[r, j])
    return pairs, lower


# ---- 3. k = 1 is the closest queries' definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_k1_equals_the_closest_definitions(orc, dtype):
    for case in (cluster_case(orc, dtype), pair_row_case(orc, dtype)):
        off, idx, rays = case["off"], case["idx"], case["rays"]
        nearest = sphere_match(off, idx, rays, case["spheres"], None, False)
        rng = np.random.default_rng(2)
        from sphere_ref import tmax_draw
        for tmax in (None, tmax_draw(rng, nearest[0][:, 0], dtype)):
            want = sphere_match(off, idx, rays, case["spheres"], tmax, False)
            vals, shape = kr.khits_match(off, idx, case["sphere"], tmax, 1)
            assert vals[:, 0].tobytes() == want[0].tobytes() and np.array_equal(shape[:, 0], want[1])
            want = box_match(off, idx, case["box"], tmax, False)
            vals, shape = kr.khits_match(off, idx, case["box"], tmax, 1)
            assert vals[:, 0].tobytes() == want[0].tobytes() and np.array_equal(shape[:, 0], want[1])
    for alternate in (False, True):
        case = triangle_row_case(orc, dtype, alternate)
        vals, shape = kr.khits_match(case["off"], case["idx"], case["triangle"], None, 1)
        assert vals[:, 0].tobytes() == case["closest"].tobytes() and np.array_equal(shape[:, 0], case["prim"])
    for name in ("stream", "aimed"):
        case = cube_case(orc, dtype, name)
        vals, shape = kr.khits_match(case["off"], case["idx"], case["triangle"], None, 1)
        assert vals[:, 0].tobytes() == case["closest"].tobytes() and np.array_equal(shape[:, 0], case["prim"])
    # the bench stream's rays pass 1 000 boxes of this scene and hit no triangle: only the aimed rays put triangle candidates into rows
    assert len(cube_case(orc, dtype, "stream")["idx"]) >= 500 and (cube_case(orc, dtype, "stream")["prim"] != NONE).sum() == 0
    assert (cube_case(orc, dtype, "aimed")["prim"] != NONE).mean() > 0.5


# ---- 4. what the scenes exercise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_truncates_at_4_and_never_at_16(orc, dtype):
    """measured with the oracle, f32 and f64 alike: 0.46 (box) and 0.12 (sphere) of the rays have more than 4 candidates; the most per ray
    are 14 (box) and 10 (sphere)"""
    case = cluster_case(orc, dtype)
    assert case["spheres"].shape == (36000, 4) and len(case["rays"]) == 20000
    for leaf in ("box", "sphere"):
        c = kr.candidate_counts(case["off"], case[leaf])
        assert (c > 4).mean() >= 0.10, (leaf, (c > 4).mean())
        assert 4 < c.max() < 16, (leaf, c.max())
        v4, s4 = kr.khits_match(case["off"], case["idx"], case[leaf], None, 4)
        v16, s16 = kr.khits_match(case["off"], case["idx"], case[leaf], None, 16)
        assert np.array_equal(s4, s16[:, :4]) and np.all(s16[:, 15] == NONE)
        assert np.array_equal((s16 != NONE).sum(axis=1), c)
        assert np.all(v16[:, 1:, 0] >= v16[:, :-1, 0])                    # rows ascend (+inf padding last)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nested_pair_row_ties_and_reversed_lists(orc, dtype):
    case = pair_row_case(orc, dtype)
    off, idx = case["off"], case["idx"]
    assert np.all(np.diff(off.astype(np.int64)) == 200)
    for leaf in ("box", "sphere"):
        rec = case[leaf]
        assert np.all(kr.candidate_counts(off, rec) == 200)
        vals, shape = kr.khits_match(off, idx, rec, None, 64)
        total = 0
        for r in range(32):                                               # +x rays: 32 tie pairs among the first 64, the later member has the lower index
            pairs, lower = _tie_pairs(off, idx, vals, shape, r)
            assert pairs == 32 and lower == 32, (leaf, r, pairs, lower)
            total += lower
        assert total == 1024
        by_index = np.lexsort((idx[off[0]:off[1]], rec[off[0]:off[1], 0]))[:64]   # a tie-break by shape index gives another row
        assert idx[off[0]:off[1]][by_index].tolist() != shape[0].tolist()
        for r in range(32, 64):                                           # -x rays: the list comes in descending distance
            d = rec[off[r]:off[r + 1], 0]
            assert np.all(np.diff(d) <= 0) and d[0] > d[-1], (leaf, r)
            assert shape[r].tolist() != idx[off[r]:off[r] + 64].tolist()
    # ray 0 (from x = -10): the pair at p = 0 at distance 10, the pair at p = 8 at 18, ... the smaller sphere (odd index) first
    vals, shape = kr.khits_match(off, idx, case["sphere"], None, 4)
    assert shape[0].tolist() == [1, 0, 3, 2] and vals[0].tolist() == [[10, 12], [10, 16], [18, 20], [18, 24]]
    vals, shape = kr.khits_match(off, idx, case["box"], None, 4)
    assert shape[0].tolist() == [1, 0, 3, 2] and vals[0].tolist() == [[10, 12], [10, 16], [18, 20], [18, 24]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_triangle_rows_ties_culling_and_reversed_lists(orc, dtype):
    # uniform winding: +x rays 200 candidates with 32 tie pairs among the first 64; -x rays visit 200 members and keep none (back faces)
    case = triangle_row_case(orc, dtype, False)
    off, idx, rec = case["off"], case["idx"], case["triangle"]
    assert np.all(np.diff(off.astype(np.int64)) == 200)
    c = kr.candidate_counts(off, rec)
    assert np.all(c[:32] == 200) and np.all(c[32:] == 0)
    vals, shape = kr.khits_match(off, idx, rec, None, 64)
    total = 0
    for r in range(32):
        pairs, lower = _tie_pairs(off, idx, vals, shape, r)
        assert pairs == 32 and lower == 32, (r, pairs, lower)
        total += lower
    assert total == 1024
    assert np.all(shape[32:] == NONE) and np.all(np.isposinf(vals[32:, :, 0])) and not vals[32:, :, 1:].any()
    assert shape[0, :4].tolist() == [1, 0, 3, 2]
    assert vals[0, :3].tolist() == [[10, 0.375, 0.375], [10, 0.21875, 0.46875], [18, 0.375, 0.375]]
    # alternating winding: even positions face -x, odd ones +x — every ray has 100 candidates, 50 pairs; -x rays meet them in descending order
    case = triangle_row_case(orc, dtype, True)
    off, idx, rec = case["off"], case["idx"], case["triangle"]
    assert np.all(np.diff(off.astype(np.int64)) == 200)
    assert np.all(kr.candidate_counts(off, rec) == 100)
    vals, shape = kr.khits_match(off, idx, rec, None, 64)
    for r in range(64):
        pairs, lower = _tie_pairs(off, idx, vals, shape, r)
        assert pairs == 32, (r, pairs)
        if r < 32:
            assert lower == 32, (r, lower)
        assert np.all(((shape[r] // 2) % 2) == (0 if r < 32 else 1))      # the positions that face the ray
    for r in range(32, 64):
        d = rec[off[r]:off[r + 1], 0]
        d = d[np.isfinite(d)]
        assert len(d) == 100 and np.all(np.diff(d) <= 0) and d[0] > d[-1], r
    assert shape[0, :4].tolist() == [1, 0, 5, 4] and vals[0, :3, 0].tolist() == [10, 10, 26]
    assert shape[40, :4].tolist() == [199, 198, 195, 194] and vals[40, :2].tolist() == [[116, 0.375, 0.375], [116, 0.46875, 0.21875]]
