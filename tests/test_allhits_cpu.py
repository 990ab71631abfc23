"""All-hits ray queries on the CPU: the new entry points are declared, exported and bound in every layer; the definition the GPU tests pin
(tests/allhits_ref.py; include/bvh_mi355x.h, bvhgpu_traverse_allhits_*) is checked on hand-made rows and, row head by row head, against
khits_ref.khits_match; and the scenes of tests/test_gpu_allhits.py are shown — on the oracle alone — to have the row lengths, the ties and
the reversed lists the GPU tests rely on, so that those cannot pass vacuously."""
import os
import re
import subprocess

import numpy as np
import pytest

import allhits_ref as ar
import khits_ref as kr
from sphere_ref import list_hits, tmax_draw
from test_khits_cpu import cluster_case, cube_case, pair_row_case, triangle_row_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_traverse_allhits_f32", "bvhgpu_traverse_allhits_f64", "bvhgpu_hits_fetch_allhits"]
DTYPES = [np.float32, np.float64]
INF = np.inf
P_LONG = 4096


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
    assert re.search(r"#define BVHGPU_ALLHITS_LIST_ORDER 1u\b", h)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define BVHGPU_ALLHITS_LIST_ORDER", raw, flags=re.S)
    assert m, "bvhgpu_traverse_allhits_* has no comment in front of it"
    text = " ".join(m.group(1).split())
    for word in ("stable", "strict", "no padding", "LIST_ORDER", "BVHGPU_OVERFLOW"):
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
    for kern in (b"k_allhits_count", b"k_allhits_fill", b"k_allhits_sort_row", b"k_rows_scan_final"):
        assert kern in blob, kern
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} missing from ffi.rs"
        assert name in lib_rs, f"{name} is not used by the shim"
    assert "pub const BVHGPU_ALLHITS_LIST_ORDER: c_uint = 1" in ffi
    assert "pub fn traverse_allhits(" in lib_rs
    from bvh_amd.api import Bvh, _Hits, _TreeBase
    assert callable(getattr(_TreeBase, "allhits_batch", None)) and "allhits_batch" in Bvh.__dict__ and callable(getattr(_Hits, "fetch_allhits", None))
    assert _lib.ALLHITS_LIST_ORDER == 1
    from bvh_amd import build_ext
    assert "allhits.hip" in build_ext.SOURCES
    lane_max, lds_max = ar.engine_thresholds(ROOT)
    assert 0 < lane_max < lds_max <= P_LONG // 2          # the long-row test crosses both with rows of at most P_LONG members


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
def test_allhits_match_on_hand_made_rows(dtype, w):
    off, idx, rec = _rows(dtype, w)

    def record(s):
        return [float(rec[list(idx).index(s), 0]), 100 + s] + ([200 + s] if w == 3 else [])

    # sorted: ties (3, 3, 3: shapes 11, 12, 15; 2, 2: shapes 7, 4) in list order; the empty row and the row of misses have no entries
    o, s, v = ar.allhits_match(off, idx, rec, None, True)
    assert o.dtype == np.uint32 and s.dtype == np.uint32 and v.dtype == dtype and v.shape == (7, w)
    assert o.tolist() == [0, 5, 5, 7, 7] and s.tolist() == [14, 11, 12, 15, 10, 7, 4]
    assert v.tolist() == [record(x) for x in (14, 11, 12, 15, 10, 7, 4)]
    # list order: the candidates as the list has them, the miss (shape 13) dropped
    o, s, v = ar.allhits_match(off, idx, rec, None, False)
    assert o.tolist() == [0, 5, 5, 7, 7] and s.tolist() == [10, 11, 12, 14, 15, 7, 4]
    assert v.tolist() == [record(x) for x in (10, 11, 12, 14, 15, 7, 4)]
    # tmax is strict: tmax == distance admits nothing at that distance
    for sort in (True, False):
        o, s, v = ar.allhits_match(off, idx, rec, np.array([3, 3, 2, INF], dtype=dtype), sort)
        assert o.tolist() == [0, 1, 1, 1, 1] and s.tolist() == [14] and v.tolist() == [record(14)]
    above = np.nextafter(dtype(3), dtype(4))
    o, s, _ = ar.allhits_match(off, idx, rec, np.array([above, 0, above, 1], dtype=dtype), True)
    assert o.tolist() == [0, 4, 4, 6, 6] and s.tolist() == [14, 11, 12, 15, 7, 4]
    o, s, _ = ar.allhits_match(off, idx, rec, np.array([above, 0, above, 1], dtype=dtype), False)
    assert o.tolist() == [0, 4, 4, 6, 6] and s.tolist() == [11, 12, 14, 15, 7, 4]
    # NaN, zero and negative tmax admit nothing; +inf admits every hit but no miss
    for t in (np.nan, 0.0, -0.0, -1.0, -INF):
        for sort in (True, False):
            o, s, v = ar.allhits_match(off, idx, rec, np.full(4, t, dtype=dtype), sort)
            assert o.tolist() == [0] * 5 and len(s) == 0 and v.shape == (0, w), t
    o, s, _ = ar.allhits_match(off, idx, rec, np.full(4, INF, dtype=dtype), True)
    assert o.tolist() == [0, 5, 5, 7, 7]
    # no rays at all
    o, s, v = ar.allhits_match(np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, w), dtype), None, True)
    assert o.tolist() == [0] and len(s) == 0 and v.shape == (0, w)
    # head_rows is khits' layout
    hv, hs = ar.head_rows(*ar.allhits_match(off, idx, rec, None, True), 3)
    want = kr.khits_match(off, idx, rec, None, 3)
    assert hv.tobytes() == want[0].tobytes() and hs.tobytes() == want[1].tobytes()


# ---- 3. row heads are khits' rows ---------------------------------------------------------------------------------------------------
def _existing_cases(orc, dtype):
    """(label, off, idx, records, drawn tmax) of every scene of tests/test_khits_cpu.py"""
    out = []
    case = cluster_case(orc, dtype)
    nearest = kr.khits_match(case["off"], case["idx"], case["sphere"], None, 1)[0][:, 0, 0]
    tm = tmax_draw(np.random.default_rng(2), nearest, dtype)
    out += [("cluster box", case["off"], case["idx"], case["box"], tm), ("cluster sphere", case["off"], case["idx"], case["sphere"], tm)]
    case = pair_row_case(orc, dtype)
    i = np.arange(64)
    tm = np.where(i % 2 == 0, 100.0, np.where(i < 32, 18.0 + i, 110.0 + (i - 32))).astype(dtype)
    out += [("pairs box", case["off"], case["idx"], case["box"], tm), ("pairs sphere", case["off"], case["idx"], case["sphere"], tm)]
    for alternate in (False, True):
        case = triangle_row_case(orc, dtype, alternate)
        out.append((f"triangle row {alternate}", case["off"], case["idx"], case["triangle"], tm))
    for name in ("stream", "aimed"):
        case = cube_case(orc, dtype, name)
        c = case["closest"][:, 0].astype(np.float64)
        tmc = np.where(np.isfinite(c), c * np.random.default_rng(4).uniform(0.3, 1.7, size=len(c)), 4e5).astype(dtype)
        out.append((f"cubes {name}", case["off"], case["idx"], case["triangle"], tmc))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_sorted_row_heads_are_the_khits_rows(orc, dtype):
    for label, off, idx, rec, drawn in _existing_cases(orc, dtype):
        for tm in (None, drawn):
            o, s, v = ar.allhits_match(off, idx, rec, tm, True)
            assert np.array_equal(np.diff(o.astype(np.int64)), kr.candidate_counts(off, rec, tm)), label
            ol, sl, vl = ar.allhits_match(off, idx, rec, tm, False)
            assert np.array_equal(ol, o) and np.array_equal(np.sort(sl), np.sort(s)), label
            for k in (1, 4, 64):
                hv, hs = ar.head_rows(o, s, v, k)
                want = kr.khits_match(off, idx, rec, tm, k)
                assert hv.tobytes() == want[0].tobytes() and hs.tobytes() == want[1].tobytes(), (label, k)


# ---- 4. the scenes of the GPU tests, on the oracle ----------------------------------------------------------------------------------
_CACHE = {}


def single_row_case(orc, dtype, reverse):
    """single_row(P_LONG) with the tier lengths: dict(scene arrays, rays, tmax, lengths, off, idx, box, sphere, triangle), once per dtype"""
    key = ("single", np.dtype(dtype).name, reverse)
    if key not in _CACHE:
        scene = ar.single_row(dtype, P_LONG, reverse)
        lengths = ar.tier_lengths(*ar.engine_thresholds(ROOT), P=P_LONG)
        rays, tmax = ar.length_rays(orc, dtype, lengths, reverse, P_LONG)
        aabbs = scene["aabbs"]
        off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(aabbs).nodes), aabbs, rays, want_t=True, threads=orc.max_threads())
        isect, _, _ = orc.triangle_stage(scene["tris"], rays, off, idx)
        _CACHE[key] = dict(scene, rays=rays, tmax=tmax, lengths=lengths, off=off, idx=idx, box=ts, sphere=list_hits(off, idx, rays, scene["spheres"]),
                           triangle=isect)
    return _CACHE[key]


def long_pair_case(orc, dtype):
    key = ("long pairs", np.dtype(dtype).name)
    if key not in _CACHE:
        spheres, aabbs = ar.pair_row(dtype, P_LONG)
        rays = ar.pair_row_rays(orc, dtype, P_LONG)
        off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(aabbs).nodes), aabbs, rays, want_t=True, threads=orc.max_threads())
        _CACHE[key] = dict(spheres=spheres, aabbs=aabbs, rays=rays, off=off, idx=idx, box=ts, sphere=list_hits(off, idx, rays, spheres))
    return _CACHE[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reverse", [False, True])
def test_length_rays_give_exactly_the_requested_lengths(orc, dtype, reverse):
    case = single_row_case(orc, dtype, reverse)
    lengths = case["lengths"]
    lane_max, lds_max = ar.engine_thresholds(ROOT)
    for m in list(range(301)) + [511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, lane_max, lane_max + 1, lds_max, lds_max + 1]:
        assert m in lengths, m
    assert 64 <= len(lengths) <= 700
    assert np.all(np.diff(case["off"].astype(np.int64)) == P_LONG)              # every ray's list holds every position
    for leaf in ("box", "sphere", "triangle"):
        assert np.all(kr.candidate_counts(case["off"], case[leaf]) == P_LONG), leaf   # ... and every position is a hit
        assert np.array_equal(kr.candidate_counts(case["off"], case[leaf], case["tmax"]), lengths), leaf
        d = case[leaf][:, 0].reshape(len(lengths), P_LONG)
        if reverse:
            assert np.all(np.diff(d, axis=1) < 0), leaf                        # the list comes in strictly descending distance
            o, s, _ = ar.allhits_match(case["off"], case["idx"], case[leaf], case["tmax"], True)
            r = int(np.nonzero(lengths == 300)[0][0])
            lst = case["idx"][case["off"][r]:case["off"][r + 1]]
            assert s[o[r]:o[r + 1]].tolist() == lst[-300:][::-1].tolist()        # the last 300 members of the list, nearest first
        else:
            assert np.all(np.diff(d, axis=1) > 0), leaf


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_pair_row_ties(orc, dtype):
    case = long_pair_case(orc, dtype)
    off, idx = case["off"].astype(np.int64), case["idx"]
    assert np.all(np.diff(off) == 2 * P_LONG)
    for leaf in ("box", "sphere"):
        rec = case[leaf]
        assert np.all(kr.candidate_counts(case["off"], rec) == 2 * P_LONG), leaf
        o, s, v = ar.allhits_match(case["off"], idx, rec, None, True)
        for r in (0, 31):                                                     # +x rays: P_LONG tie pairs, each in list order
            row_s, row_d = s[o[r]:o[r + 1]], v[o[r]:o[r + 1], 0]
            ties = np.nonzero(row_d[1:] == row_d[:-1])[0]
            assert len(ties) == P_LONG, (leaf, r, len(ties))
            place = np.empty(2 * P_LONG, dtype=np.int64)
            place[idx[off[r]:off[r + 1]]] = np.arange(2 * P_LONG)
            assert np.all(place[row_s[ties]] < place[row_s[ties + 1]]), (leaf, r)
            assert (row_s[ties + 1] < row_s[ties]).sum() >= P_LONG // 2        # a tie-break by shape index would give another row


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_and_cube_scenes_cover_the_short_rows(orc, dtype):
    case = cluster_case(orc, dtype)
    for leaf in ("box", "sphere"):
        c = kr.candidate_counts(case["off"], case[leaf])
        assert (c == 0).sum() > 100 and (c == 1).sum() > 100 and (c > 4).sum() > 100, (leaf, np.bincount(c)[:6])
    assert np.isfinite(case["box"][:, 0]).all()                               # every enter is finite: LIST_ORDER rows are traverse_batch's CSR
    stream = cube_case(orc, dtype, "stream")
    members = np.diff(stream["off"].astype(np.int64))
    cand = kr.candidate_counts(stream["off"], stream["triangle"])
    # the bench stream passes boxes on one ray in forty (0.025, f32 and f64 alike) and hits no triangle at all: every ray that has a list has a
    # row that is empty after a full walk
    share = ((members > 0) & (cand == 0)).mean()
    assert 0.02 < share < 0.03 and (members > 0).sum() >= 400, (share, (members > 0).sum())
    assert cand.sum() == 0 and members.sum() >= 500
