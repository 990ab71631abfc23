"""Convex-region (plane-set) queries, on the CPU alone: the definition restated three ways (tests/region_ref.py: the lockstep walk, the
entry-by-entry walk, the brute-force set), the kernel's schedule restated on the CPU against them (bvh_amd/csrc/region.hip: chunks, windows,
the exclusive prefix maximum, the ancestor table and the deep-path descent), hand cases with known answers, the host-side plane builders,
the conditions that make the main scene of tests/test_gpu_region.py worth running, and the wiring of the new family through every layer."""
import os
import re

import numpy as np
import pytest

import fuzz_scenes as fz
import query_ref as qr
import region_ref as rr
from test_within_cpu import far_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
CHUNK_MIN = 1024      # bvh_amd/csrc/region.hip REGION_CHUNK_MIN: the kernel's smallest chunk_entries
SMALL = (1, 2, 3, 70)


def _cubes(n, dtype):
    from oracle import orc
    _, a = orc.create_n_cubes(n)
    return np.ascontiguousarray(a.astype(dtype))


def _rows(off, idx):
    return [idx[off[q]:off[q + 1]].tolist() for q in range(len(off) - 1)]


# ---- 1. the three statements of the definition, and the schedule ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_walks_agree_and_equal_brute_force_and_the_scan(dtype):
    """oracle trees of 1, 2, 3 and 70 cubes, 40 regions of 1 - 6 random planes: walk == walk_one, the row as a set == brute force, and the
    kernel's schedule gives the row for windows of 4 and 64, chunks of 8, 128 and 1024, over the FlatNode array and over the folded one,
    with the ancestor table and (table of 2 entries) with the serial descent"""
    for n in SMALL:
        a = _cubes(n, dtype)
        flat = rr.oracle_tree(a)
        assert not fz.has_empty_child_bounds(flat)
        pl = rr.random_regions(a, 40, 5)
        off, idx, ins = rr.walk(flat, a, pl)
        rows = _rows(off, idx)
        assert sum(1 for r in rows if r) >= 10 and (n < 70 or sum(1 for r in rows if not r) >= 1), n   # (a plane through a single cube's middle never misses it)
        ents = [rr.entries(flat, a, False), rr.entries(flat, a, True)]
        assert len(ents[1]["exit"]) == max(2 * len(a) - 2, 1) and len(ents[0]["exit"]) == 3 * len(a) - 2
        for q, row in enumerate(rows):
            if n <= 3 or q < 8:
                assert row == rr.walk_one(flat, a, pl[q]), (n, q)
            assert sorted(row) == rr.brute(a, pl[q], dtype).tolist(), (n, q)
            b = a[row]
            assert ins[off[q]:off[q + 1]].tolist() == rr.inside(np.repeat(pl[q:q + 1], len(b), axis=0), b[:, :3], b[:, 3:]).astype(int).tolist()
            for ent in ents:
                for window, chunk in ((4, 8), (64, 128), (4, 128), (64, 1024)):
                    assert rr.scan(ent, pl[q], window, chunk) == row, (n, q, window, chunk)
                assert rr.scan(ent, pl[q], 4, 8, anc_max=2) == row, (n, q, "serial descent")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_regions_make_every_one_of_32_planes_decide(dtype):
    """the batch tests/test_gpu_region.py runs for m = 32 without padding (70 cubes, BALL_REGIONS regions of 32 tangent planes): most rows
    are non-empty, and for EVERY plane index 0 .. 31 some region has a shape that fails that plane and no other — so a kernel that read a
    high plane index wrongly, or stopped its loop early, gives another row.  (No empty child bounds: the row is the brute-force set.)"""
    a = _cubes(70, dtype)
    pl = rr.ball_regions(a, rr.BALL_REGIONS, rr.BALL_SEED)
    assert pl.shape == (rr.BALL_REGIONS, 32, 4) and (pl[:, :, :3] != 0).all()
    lo, hi = a[:, :3], a[:, 3:]
    decided = np.zeros(32, dtype=np.int64)
    nonempty = 0
    for q in range(len(pl)):
        with np.errstate(invalid="ignore"):
            ok = rr._sums(np.repeat(pl[q:q + 1], len(a), axis=0), lo, hi, True) >= 0          # (shape, plane)
        nonempty += bool(ok.all(axis=1).any())
        only = np.nonzero((~ok).sum(axis=1) == 1)[0]
        decided += np.bincount(np.argmin(ok[only], axis=1), minlength=32) > 0
    assert nonempty >= 200 and (decided >= 2).all(), (nonempty, decided.tolist())
    off, idx, _ = rr.walk(rr.oracle_tree(a), a, pl[:20])
    for q in range(20):
        assert sorted(idx[off[q]:off[q + 1]].tolist()) == rr.brute(a, pl[q], dtype).tolist(), q


def test_scan_takes_the_deep_path_on_a_chain():
    """a right-leaning chain of 100 shapes: the last chunks' ancestor paths are longer than the 64-entry table, so the walk descends itself"""
    for dtype in DTYPES:
        a = _cubes(9, dtype)[:100]
        flat = rr.chain_flat(a)
        pl = rr.random_regions(a, 20, 7)
        off, idx, _ = rr.walk(flat, a, pl)
        rows = _rows(off, idx)
        assert sum(1 for r in rows if r) >= 5
        ent = rr.entries(flat, a, False)
        assert len(rr.ancestors(ent, len(flat) - 1)) == 99
        deep = 0
        for q, row in enumerate(rows):
            assert row == rr.walk_one(flat, a, pl[q])
            units = []
            assert rr.scan(ent, pl[q], 64, 64, units=units) == row
            deep += sum(u["deep"] for u in units)
        assert deep >= 20


# ---- 2. hand cases ---------------------------------------------------------------------------------------------------------------------
def _grid(dtype):
    """4 x 4 x 4 unit boxes at even integer corners: box (i, j, k) = [2i, 2i + 1] x ..."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) * 2.0
    return np.concatenate([g, g + 1], axis=1).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_space_through_a_grid(dtype):
    a = _grid(dtype)
    flat = rr.oracle_tree(a)
    # x >= 2.5: the boxes with max x >= 2.5 (i >= 1) pass; wholly inside are those with min x >= 2.5 (i >= 2)
    off, idx, ins = rr.walk(flat, a, np.array([[1, 0, 0, -2.5]], dtype))
    assert sorted(idx.tolist()) == np.nonzero(a[:, 3] >= 2.5)[0].tolist() and len(idx) == 48
    assert sorted(idx[ins == 1].tolist()) == np.nonzero(a[:, 0] >= 2.5)[0].tolist() and (ins == 1).sum() == 32
    # the plane on a box face: s == 0 passes (x <= 2 keeps the boxes that start at 2)
    off, idx, ins = rr.walk(flat, a, np.array([[-1, 0, 0, 2.0]], dtype))
    assert sorted(idx.tolist()) == np.nonzero(a[:, 0] <= 2)[0].tolist() and len(idx) == 32
    assert sorted(idx[ins == 1].tolist()) == np.nonzero(a[:, 3] <= 2)[0].tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_aabb_planes_give_the_aabb_query_rows(dtype):
    """aabb_planes(mn, mx) against query_ref's AABB rows: the sums are hi - mn and mx - lo, whose sign is exact for finite coordinates, so
    the rows are identical — list order included — on boxes with integer and half-integer corners (no sum rounds at all)"""
    from bvh_amd.region import aabb_planes
    a = _cubes(70, dtype)
    a = np.round(a * 2) / 2                                     # half-integer corners, far below 2^24
    flat = rr.oracle_tree(a)
    rng = np.random.default_rng(3)
    c = a[rng.integers(0, len(a), 30), :3]
    half = rng.integers(1, 400000, size=(30, 3)) / 2
    boxes = np.concatenate([c - half, c + half], axis=1).astype(dtype)
    planes = np.stack([aabb_planes(b[:3], b[3:], dtype) for b in boxes])
    assert planes.shape == (30, 6, 4) and planes.dtype == dtype
    off, idx, _ = rr.walk(flat, a, planes)
    qoff, qidx = qr.walk(flat, a, qr.AABB, boxes)
    assert off.tobytes() == qoff.tobytes() and idx.tobytes() == qidx.tobytes()
    n = np.diff(off.astype(np.int64))
    assert (n > 0).sum() >= 20 and n.max() > 100 and n.min() <= 24


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_planes_nan_plane_padding_plane_and_inverted_box(dtype):
    a = _grid(dtype)
    a[5] = [3.0, 3.0, 3.0, 2.0, 2.0, 2.0]                       # an inverted shape box: max < min on every axis
    flat = rr.oracle_tree(a)
    assert not fz.has_empty_child_bounds(flat)
    every = [int(s) for s in flat["shape"][flat["entry"] == rr.NONE]]
    # m = 0 passes every box, wholly
    off, idx, ins = rr.walk(flat, a, np.zeros((1, 0, 4), dtype))
    assert idx.tolist() == every and ins.all()
    # the padding plane passes every finite box, and mixes plane counts in one batch
    off, idx, ins = rr.walk(flat, a, np.zeros((1, 3, 4), dtype))
    assert idx.tolist() == every and ins.all()
    one = np.array([[[1, 0, 0, -2.5]]], dtype)
    padded = np.concatenate([one, np.zeros((1, 5, 4), dtype)], axis=1)
    assert [x.tobytes() for x in rr.walk(flat, a, one)] == [x.tobytes() for x in rr.walk(flat, a, padded)]
    # a NaN d is a NaN sum: a miss, at the root's children already
    off, idx, _ = rr.walk(flat, a, np.array([[[1, 0, 0, np.nan]]], dtype))
    assert len(idx) == 0
    # a NaN normal component takes lo and makes the sum NaN
    off, idx, _ = rr.walk(flat, a, np.array([[[np.nan, 0, 0, 1e9]]], dtype))
    assert len(idx) == 0
    # -0 takes hi like +0: (−0, 0, 0, d) is a padding plane with d
    neg0 = np.array([[[-0.0, 0, 0, 0.0]]], dtype)
    assert rr.walk(flat, a, neg0)[1].tolist() == every
    # the inverted box: x >= 2.5 takes its "hi" = 2 → a miss, although its min corner (3) is inside; x <= 2.5 takes its "lo" = 3 → a miss:
    # the row is still the brute-force set (fact 1 holds for inverted shape boxes)
    for pl in (np.array([[1, 0, 0, -2.5]], dtype), np.array([[-1, 0, 0, 2.5]], dtype), np.array([[1, 0, 0, -1.5]], dtype)):
        off, idx, _ = rr.walk(flat, a, pl)
        assert sorted(idx.tolist()) == rr.brute(a, pl, dtype).tolist()
    assert 5 not in rr.walk(flat, a, np.array([[1, 0, 0, -2.5]], dtype))[1] and 5 in rr.walk(flat, a, np.array([[1, 0, 0, -1.5]], dtype))[1]


def test_walk_defines_the_row_on_trees_with_empty_child_bounds():
    """a fuzz_scenes draw from the band where surface areas overflow (splits without SAH winner): the empty navigator boxes give -inf or
    NaN sums and are never entered, so the walk reports fewer shapes than pass on their own — and with m = 0 it reports all of them"""
    for dtype, k_scale in ((np.float32, 70), (np.float64, 520)):
        sc = fz.draw(2, dtype, 0, k_scale, n_pin=300)
        a = sc["aabbs"]
        flat = rr.oracle_tree(a)
        assert fz.has_empty_child_bounds(flat)
        pl = rr.random_regions(a, 20, 9)
        off, idx, _ = rr.walk(flat, a, pl)
        differ = 0
        for q, row in enumerate(_rows(off, idx)):
            want = rr.brute(a, pl[q], dtype).tolist()
            assert set(row) <= set(want)
            assert row == rr.walk_one(flat, a, pl[q])
            assert rr.scan(rr.entries(flat, a, False), pl[q], 64, 128) == row      # (the engine walks the unfolded mirror of such a tree)
            differ += sorted(row) != want
        assert differ >= 5
        assert len(rr.walk(flat, a, np.zeros((1, 0, 4), dtype))[1]) == len(a)
    far = far_scene(np.float32)[0]                                                # the scene tests/test_gpu_region.py builds on the GPU
    flat = rr.oracle_tree(far)
    assert fz.has_empty_child_bounds(flat)
    pl = rr.random_regions(far, 20, 9)
    off, idx, _ = rr.walk(flat, far, pl)
    assert sum(sorted(r) != rr.brute(far, pl[q], np.float32).tolist() for q, r in enumerate(_rows(off, idx))) >= 5


# ---- 3. the host-side plane builders ---------------------------------------------------------------------------------------------------
def test_frustum_planes_contain_what_the_camera_rays_reach():
    """api.camera's rays are eye + t (forward + sx tan_x right + sy tan_y up), sx, sy in [-1, 1]: every such point at depth near .. far
    (measured along forward) is inside all six planes, and points just beyond each plane are outside that plane alone"""
    from bvh_amd.api import camera
    from bvh_amd.region import frustum_planes
    eye, look, up, fov, aspect, near, far = (3.0, -2.0, 5.0), (10.0, 4.0, -1.0), (0.1, 1.0, 0.0), 50.0, 1.6, 0.5, 80.0
    cam = camera(eye, look, up, fov, aspect).astype(np.float64)
    e, r, u, f, tx, ty = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
    pl = frustum_planes(eye, look, up, fov, aspect, near, far, np.float64)
    assert pl.shape == (6, 4) and frustum_planes(eye, look, up, fov, aspect, near, far, np.float32).dtype == np.float32
    rng = np.random.default_rng(1)
    sx, sy = rng.uniform(-1, 1, 2000), rng.uniform(-1, 1, 2000)
    depth = rng.uniform(near, far, 2000)
    sx[:8], sy[:8] = [-1, 1, -1, 1, -1, 1, -1, 1], [-1, -1, 1, 1, -1, -1, 1, 1]   # the eight corners
    depth[:4], depth[4:8] = near, far
    pts = e + depth[:, None] * (f + (sx * tx)[:, None] * r + (sy * ty)[:, None] * u)
    s = pts @ pl[:, :3].T + pl[:, 3]
    tol = 1e-5 * far                                                              # (the camera's axes are rounded to f32)
    assert (s >= -tol).all()
    inner = (np.abs(sx) < 0.99) & (np.abs(sy) < 0.99) & (depth > near + 0.01) & (depth < far - 0.01)
    assert inner.sum() > 1500 and (s[inner] > 0).all()
    # just outside each plane: that plane alone says so
    for k, (ax, ay, d) in enumerate(((-1.05, 0, 10), (1.05, 0, 10), (0, -1.05, 10), (0, 1.05, 10), (0, 0, near * 0.9), (0, 0, far * 1.1))):
        p = e + d * (f + ax * tx * r + ay * ty * u)
        sp = pl[:, :3] @ p + pl[:, 3]
        assert sp[k] < 0 and (np.delete(sp, k) > 0).all(), k


# ---- 4. the main scene of the GPU test -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_main_scene_is_worth_running(dtype):
    """900 cubes, 10 800 shapes, 21 598 folded entries; 40 regions of 1 - 6 random planes through the middle 80 % of the bounds, and 24
    more whose first plane cuts a shape (region_ref.random_regions: in this scene of unit cubes in +-1e5 a random plane almost never
    does, and the `inside` byte would be 1 everywhere)"""
    m = rr.main_scene(dtype)
    a, flat, planes, off, idx, ins = m["aabbs"], m["flat"], m["planes"], m["off"], m["idx"], m["ins"]
    assert len(a) == 10800 and len(planes) == rr.MAIN_REGIONS + rr.MAIN_CUT and rr.MAIN_REGIONS >= 40
    ent = rr.entries(flat, a, True)
    assert len(ent["exit"]) == 21598 and not fz.has_empty_child_bounds(flat)
    n = np.diff(off.astype(np.int64))
    plain = n[:rr.MAIN_REGIONS]
    assert (plain > 0).sum() >= 10 and (plain == 0).sum() >= 5, ((plain > 0).sum(), (plain == 0).sum())
    # the kernel's schedule at its smallest chunk: the rows again, rows over several chunks, units a failing ancestor kills and units it does not
    spanning, killed, alive = 0, 0, 0
    for q in list(range(0, len(planes), 4)) + list(range(rr.MAIN_REGIONS, len(planes))):
        units = []
        assert rr.scan(ent, planes[q], 64, CHUNK_MIN, units=units) == idx[off[q]:off[q + 1]].tolist(), q
        assert len(units) == 22
        spanning += sum(u["count"] > 0 for u in units) >= 2
        killed += sum(u["killed"] for u in units)
        alive += sum(not u["killed"] for u in units)
    assert spanning >= 10 and killed >= 1 and alive >= 1, (spanning, killed, alive)
    assert rr.scan(ent, planes[1], 4, CHUNK_MIN) == idx[off[1]:off[2]].tolist()
    # both inside values, in at least 10 rows each
    has0 = sum(1 for q in range(len(n)) if n[q] and ins[off[q]:off[q + 1]].min() == 0)
    has1 = sum(1 for q in range(len(n)) if n[q] and ins[off[q]:off[q + 1]].max() == 1)
    assert has0 >= 10 and has1 >= 10, (has0, has1)


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------------
def test_region_is_wired_through_every_layer():
    from bvh_amd import build_ext
    assert "region.hip" in build_ext.SOURCES and "unfold.hpp" in build_ext.HEADERS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    for sym in ("bvhgpu_region_f32", "bvhgpu_region_f64", "bvhgpu_hits_fetch_region", "bvhgpu_hits_region_info"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
    for macro, value in (("BVHGPU_REGION_MAX_PLANES", "32"), ("BVHGPU_REGION_COUNT_ONLY", "1u"), ("BVHGPU_REGION_CLASSIFY", "2u")):
        assert re.search(r"#define %s %s\b" % (macro, value), header), macro
    assert re.search(r"#define BVHGPU_ABI_VERSION 7\b", header)
    import bvh_amd
    from bvh_amd import _lib, api
    assert bvh_amd.region_batch.__module__ == "bvh_amd.region"
    assert bvh_amd.frustum_planes.__module__ == bvh_amd.aabb_planes.__module__ == "bvh_amd.region"
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert {"bvhgpu_region_f32", "bvhgpu_region_f64", "bvhgpu_hits_fetch_region", "bvhgpu_hits_region_info"} <= bound
    assert (_lib.REGION_MAX_PLANES, _lib.REGION_COUNT_ONLY, _lib.REGION_CLASSIFY) == (32, 1, 2) == (rr.MAX_PLANES, 1, 2)
    # the public surface of the six pinned classes is what the call-trace test's golden file lists: nothing about regions reached them
    for cls in (api.Context, api.RayBatch, api._Hits, api._TreeBase, api.FlatBvh, api.Bvh):
        assert not [k for k in vars(cls) if "region" in k or "plane" in k or "frustum" in k], cls
    # the kernel's constants this file restates
    src = open(os.path.join(ROOT, "bvh_amd", "csrc", "region.hip")).read()
    assert re.search(r"REGION_CHUNK_MIN = %d;" % CHUNK_MIN, src) and re.search(r"REGION_ANC_MAX = 64;", src)
