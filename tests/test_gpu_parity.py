"""Parity tests proper: the HIP engine (through the C ABI, via bvh_amd's ctypes mirror) against the
CPU oracle on the same seeded inputs, and against the reference's own known-answer vectors.
Bar: bit-exact for BvhNode / FlatNode arrays, shape->node map, CSR offsets and indices (order
included) and t-slices (two NaNs count as equal).
"""
import json
import os

import numpy as np
import pytest

from test_fp_extremes_cpu import same as same_bytes  # byte equality, two NaNs equal

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_known_answers.json")))


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
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    return eng.RayBatch(len(rays), dt, host=np.ascontiguousarray(rays))


def _full_parity(eng, orc, aabbs, rays):
    bvh = eng.Bvh.from_aabbs(aabbs)
    ot = orc.build(aabbs)
    assert bvh.nodes.tobytes() == ot.nodes.tobytes()
    assert np.array_equal(bvh.shape_nodes, ot.shape_node)
    flat = bvh.flatten()
    oflat = orc.flatten(ot.nodes)
    assert flat.nodes.tobytes() == oflat.tobytes()
    off, idx, ts, st = flat.traverse_batch(_rb(eng, rays), want_t=True, stats=True)
    ooff, oidx, ots, ost = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    assert np.array_equal(off, ooff)
    assert np.array_equal(idx, oidx)
    if len(idx):
        assert same_bytes(ts, ots)
    assert st["hits"] == ost["hits"] and st["visited"] == ost["visited"] and st["leaf_visits"] == ost["leaf_visits"]
    # the same batch without STATS / T_SLICE: the default walk for large batches (the wide walk) must give the same CSR
    off2, idx2, _, _ = flat.traverse_batch(_rb(eng, rays))
    assert np.array_equal(off2, ooff) and np.array_equal(idx2, oidx)
    return bvh, flat, ot, oflat


# ------------------------------------------------------------------ reference known answers
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_golden_hit_sets(eng, dtype):
    """testbase.rs:174-225 through the trait-surface mirror (Bvh::build, build_par, FlatBvh::build)."""
    from bvh_amd import testbase as tb
    g = GOLD["aligned_boxes"]
    for builder in (eng.Bvh.build, eng.Bvh.build_par, eng.FlatBvh.build):
        shapes = tb.generate_aligned_boxes()
        bh = builder(shapes, dtype)
        for case in g["rays"]:
            ray = eng.Ray(case["origin"], case["direction"], dtype)
            hit = bh.traverse(ray, shapes)
            assert sorted(s.id for s in hit) == sorted(case["hit_ids"])
        # set_bh_node_index was called with the leaf that holds each shape (bvh_node.rs:102)
        if isinstance(bh, eng.Bvh):
            nodes = bh.nodes
            for i, s in enumerate(shapes):
                assert nodes[s.bh_node_index()]["shape"] == i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_one_node_and_empty(eng, dtype):
    from bvh_amd import testbase as tb
    for case in GOLD["one_node"]["cases"]:  # bvh_impl.rs:667-690
        boxes = [tb.UnitBox(0, case["box_center"])]
        ray = eng.Ray(case["origin"], case["direction"], dtype)
        bvh = eng.Bvh.build(boxes, dtype)
        assert len(bvh.traverse(ray, boxes)) == case["hits"]
        assert len(bvh.flatten().traverse(ray, boxes)) == case["hits"]
        assert len(bvh.nodes) == 1 and len(bvh.flatten().nodes) == 1
    empty = eng.Bvh.build([], dtype)  # bvh_impl.rs:57-59, flat_bvh.rs:245-248
    assert len(empty.nodes) == 0 and len(empty.flatten().nodes) == 0
    assert empty.traverse(eng.Ray([0, 0, 0], [1, 0, 0], dtype), []) == []


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_slab_edge_cases(eng, dtype):
    """ray_impl.rs:245-299 through Ray.intersects_aabb / intersection_slice_for_aabb (device slab test)."""
    s = GOLD["slab"]

    def ub(c):
        c = np.asarray(c, dtype=dtype)
        return eng.Aabb(c + dtype(-0.5), c + dtype(0.5), dtype)
    z = s["zero_depth"]
    assert eng.Ray(z["origin"], z["direction"], dtype).intersects_aabb(eng.Aabb(z["aabb"][:3], z["aabb"][3:], dtype))
    a = s["slice_accuracy"]
    box = eng.Aabb.empty(dtype).grow(a["grow_points"][0]).grow(a["grow_points"][1])
    tmin, tmax = eng.Ray(a["origin"], a["direction"], dtype).intersection_slice_for_aabb(box)
    assert abs(tmin - a["tmin"]) < a["tol"] and abs(tmax - a["tmax"]) < a["tol"]
    p = s["parallel_miss"]
    assert eng.Ray(p["origin"], p["direction"], dtype).intersection_slice_for_aabb(ub(p["box_center"])) is None
    for c in s["in_plane"]:
        r = eng.Ray(c["origin"], c["direction"], dtype)
        assert r.intersects_aabb(ub(c["box_center"])) is False
        assert r.intersection_slice_for_aabb(ub(c["box_center"])) is None


# ------------------------------------------------------------------ oracle parity, seeded scenes
def test_parity_config0_1200_triangles(eng, orc):
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(100)
    _full_parity(eng, orc, aabbs, orc.create_rays(0, 1000))


def test_parity_config1_120k_triangles(eng, orc):
    """BASELINE.json configs[1] at full size: 120 k triangles, ALL 1 M rays of the seed-0 stream — nodes, flat array,
    CSR (order included), t-slices and visit counters against the oracle (which needs < 1 s for it, multi-threaded)."""
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(10_000)
    bvh, flat, ot, oflat = _full_parity(eng, orc, aabbs, orc.create_rays(0, 1_000_000))
    assert orc.check_tree(bvh.nodes, aabbs) == 0  # assert_consistent + assert_tight + coverage on the GPU tree


def test_parity_config4_f64(eng, orc):
    """BASELINE.json configs[4] at full size: the same scene and ALL 1 M rays in f64 (t-values within 1e-12 relative)."""
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(10_000)
    r32 = orc.create_rays(0, 1_000_000)
    rays = orc.make_rays(r32["o"].astype(np.float64), r32["d"].astype(np.float64), np.float64)
    _full_parity(eng, orc, aabbs.astype(np.float64), rays)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 66, 127, 128, 129, 767, 768, 769, 1000, 1024, 1025, 1536, 1537, 4099])
def test_parity_ragged_sizes(eng, orc, n, dtype):
    """sizes around the wave (64) and tile (1024) boundaries of the two builder tiers."""
    rng = np.random.default_rng(n)
    lo = rng.uniform(-100, 100, size=(n, 3)).astype(dtype)
    ext = rng.uniform(0, 10, size=(n, 3)).astype(dtype)
    aabbs = np.concatenate([lo, lo + ext], axis=1)
    o = rng.uniform(-120, 120, size=(300, 3)).astype(dtype)
    d = rng.normal(size=(300, 3)).astype(dtype)
    _full_parity(eng, orc, aabbs, orc.make_rays(o, d, dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_degenerate_and_collisions(eng, orc, dtype):
    """identical centroids (bvh_node.rs:114-124 halving path) at both tiers, zero-thickness boxes,
    shapes sharing one AABB, axis-parallel rays (inf inverse directions) and in-plane rays (NaN → miss)."""
    rng = np.random.default_rng(11)
    n = 3000
    lo = rng.integers(-20, 20, size=(n, 3)).astype(dtype)          # integer grid: many exact ties
    ext = rng.integers(0, 3, size=(n, 3)).astype(dtype)            # zero-thickness boxes included
    lo[500:1400] = lo[500]; ext[500:1400] = ext[500]               # 900 identical boxes (> 64: tier-1 degenerate)
    lo[2000:2040] = lo[2000]; ext[2000:2040] = ext[2000]           # 40 identical boxes (tier-2 degenerate)
    aabbs = np.concatenate([lo, lo + ext], axis=1)
    o = rng.integers(-25, 25, size=(2000, 3)).astype(dtype)
    d = rng.integers(-1, 2, size=(2000, 3)).astype(dtype)          # axis-parallel / diagonal directions
    d[np.all(d == 0, axis=1)] = [1, 0, 0]
    rays = orc.make_rays(o, d, dtype)
    _full_parity(eng, orc, aabbs, rays)
    # all shapes identical: every split is the halving path
    same = np.tile(aabbs[500], (777, 1))
    _full_parity(eng, orc, same, rays[:200])


def test_parity_unbalanced_deep_tree(eng, orc):
    """exponentially spaced boxes: SAH peels a few hundred shapes per level → far more level-synchronous
    passes than the optimistic batch, exercising the host-synchronised continuation of the level loop
    (and re-launches of the workgroup and wave tiers for the items queued late)."""
    n = 12000
    x = np.float32(1.004) ** np.arange(n, dtype=np.float32)
    lo = np.stack([x, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
    aabbs = np.concatenate([lo, lo + np.float32(0.5)], axis=1).astype(np.float32)
    o = np.zeros((64, 3), np.float32); o[:, 1] = 0.25; o[:, 2] = 0.25; o[:, 0] = -1
    d = np.tile(np.array([1, 0, 0], np.float32), (64, 1))
    bvh, *_ = _full_parity(eng, orc, aabbs, orc.make_rays(o, d))
    assert bvh.build_levels >= 5  # optimistic batch for n = 12 000 is 4 passes: the continuation ran


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("launches", [1, 2, (2, 1024), (2, 4096)])
def test_level_tier_schedules_same_tree(eng, orc, launches, dtype):
    """The level tier as one launch per level (k_level: split of level L-1 and binning of level L fused, default) and as two
    (k_bin, k_split) must both reproduce the oracle's node array: balanced scene, the unbalanced deep tree (host-continued
    level loop), sizes around the tier's hand-over, a scene with colliding centroids (degenerate halving in the level tier)."""
    from bvh_amd import Bvh, Context, testbase as tb
    from bvh_amd._lib import TUNE_BUILD_LEVEL_LAUNCHES, TUNE_BUILD_LEVEL_TILE
    ctx = Context(0)
    if isinstance(launches, tuple):   # the two-launch schedule with the tile size it takes on scenes of millions of shapes (a scheduling unit: same tree)
        launches, tile = launches
        ctx.set_tuning(TUNE_BUILD_LEVEL_TILE, tile)
    ctx.set_tuning(TUNE_BUILD_LEVEL_LAUNCHES, launches)
    rng = np.random.default_rng(5)
    scenes = []
    _, cubes = tb.create_n_cubes(2500)
    scenes.append(cubes.astype(dtype))
    n = 12000
    x = np.float32(1.004) ** np.arange(n, dtype=np.float32)
    lo = np.stack([x, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
    scenes.append(np.concatenate([lo, lo + np.float32(0.5)], axis=1).astype(dtype))
    for m in (769, 770, 1537, 1538, 3077, 6000):
        lo = rng.uniform(-50, 50, size=(m, 3))
        scenes.append(np.concatenate([lo, lo + rng.uniform(0, 3, size=(m, 3))], axis=1).astype(dtype))
    same = np.tile(np.array([[1, 2, 3, 4, 5, 6]], dtype), (5000, 1))          # every centroid equal: halving all the way down
    scenes.append(same)
    half = np.concatenate([same[:2500], cubes[:3000].astype(dtype)])           # a degenerate cluster inside a normal scene
    scenes.append(half)
    bvh = None
    for aabbs in scenes:
        ot = orc.build(aabbs)
        bvh = Bvh.from_aabbs(aabbs, ctx) if bvh is None else bvh.rebuild(aabbs)
        assert bvh.nodes.tobytes() == ot.nodes.tobytes(), (launches, len(aabbs))
        assert np.array_equal(bvh.shape_nodes, ot.shape_node)
    # the same tree object rebuilt with a scene it has a level hint for
    bvh.rebuild(scenes[0]); bvh.rebuild(scenes[0])
    assert bvh.nodes.tobytes() == orc.build(scenes[0]).nodes.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("groups_of", [1, 16, 64])
def test_persistent_level_tier_same_tree(eng, orc, groups_of, dtype):
    """BVHGPU_TUNE_BUILD_LEVEL_PERSIST: the level tier's passes below tree level 3 as ONE persistent launch, a workgroup group per
    level-3 subtree synchronising with itself (build.hip k_level_xcd; 1 = 32 workgroups per group, else that many).  The BvhNode array
    (bvh_node.rs:81-279) and the shape → node map must be the oracle's, bit for bit: balanced scenes, sizes around the tier's threshold
    (32 x 769 shapes), an unbalanced chain (one subtree holds nearly everything and runs on for dozens of passes), colliding centroids
    (the halving branch inside the persistent passes), rebuilds of the same tree object, and the wide walk's CSR on the result."""
    from bvh_amd import Bvh, Context, testbase as tb
    from bvh_amd._lib import TUNE_BUILD_LEVEL_PERSIST
    ctx = Context(0)
    ctx.set_tuning(TUNE_BUILD_LEVEL_PERSIST, groups_of)
    rng = np.random.default_rng(11)
    scenes = []
    _, cubes = tb.create_n_cubes(10000)
    scenes.append(cubes.astype(dtype))                                  # configs[1]'s scene
    scenes.append(cubes[:30000].astype(dtype))
    for m in (24607, 24608, 24609, 50001):                              # around 32 x (768 + 1)
        lo = rng.uniform(-500, 500, size=(m, 3))
        scenes.append(np.concatenate([lo, lo + rng.uniform(0, 3, size=(m, 3))], axis=1).astype(dtype))
    n = 40000
    x = np.float32(1.0003) ** np.arange(n, dtype=np.float32)
    lo = np.stack([x, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
    scenes.append(np.concatenate([lo, lo + np.float32(0.5)], axis=1).astype(dtype))        # unbalanced: long chains below level 3
    same = np.tile(np.array([[1, 2, 3, 4, 5, 6]], dtype), (30000, 1))                       # every centroid equal: halving all the way down
    scenes.append(same)
    scenes.append(np.concatenate([same[:12000], cubes[:24000].astype(dtype)]))              # a degenerate cluster inside a scene
    clustered = np.concatenate([cubes[:3000].astype(dtype) * dtype(0.001), cubes[3000:60000].astype(dtype)])   # one level-3 subtree tiny
    scenes.append(clustered)
    bvh = None
    for aabbs in scenes:
        ot = orc.build(aabbs, threads=orc.max_threads(), schedule="fast")
        for _ in range(2):                                              # (the second build of a scene reuses every buffer and counter)
            bvh = Bvh.from_aabbs(aabbs, ctx) if bvh is None else bvh.rebuild(aabbs)
            assert bvh.nodes.tobytes() == ot.nodes.tobytes(), (groups_of, len(aabbs))
            assert np.array_equal(bvh.shape_nodes, ot.shape_node)
    # the asynchronous step on such a tree, and the walk of what it built
    rays = orc.create_rays(0, 50_000, tb.default_bounds(), dtype)
    a = scenes[0]
    ot = orc.build(a, threads=orc.max_threads(), schedule="fast")
    oflat = orc.flatten(ot.nodes)
    ooff, oidx, _, _ = orc.traverse_flat(oflat, a, rays, threads=orc.max_threads())
    import torch
    from bvh_amd import RayBatch
    dev_a = torch.from_numpy(a).cuda()
    dev_r = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    rb = RayBatch.from_device(dev_r, len(rays), dtype)
    for _ in range(3):
        bvh.rebuild_async(dev_a)
        h = bvh.traverse_async(rb)
        h.wait()
        off, idx = h.fetch(len(rays))
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    assert bvh.flatten().nodes.tobytes() == oflat.tobytes()
    # a subtree deeper than the tier's counter slots (f64 only: 1.02^i over 30 000 shapes needs the exponent range; every split peels ≈ 90
    # shapes off the chain, well over a hundred levels with more than 768 shapes): the persistent launch gives up (BUILD_FLAG_PERSIST_GAVE_UP),
    # build_finalize builds the same generation again with a launch per level — same arrays, and the tree object stays with that schedule;
    # an asynchronous batch enqueued on the abandoned build is replayed on the finished tree
    if dtype == np.float64:
        m = 30000
        xs = np.float64(1.02) ** np.arange(m, dtype=np.float64)
        lo = np.stack([xs, np.zeros(m), np.zeros(m)], axis=1)
        deep = np.concatenate([lo, lo + 0.5], axis=1)
        ot = orc.build(deep, threads=orc.max_threads(), schedule="fast")
        deep_tree = Bvh.from_aabbs(deep, ctx)
        assert deep_tree.nodes.tobytes() == ot.nodes.tobytes() and np.array_equal(deep_tree.shape_nodes, ot.shape_node)
        assert deep_tree.build_levels > 92
        oflat = orc.flatten(ot.nodes)
        o = np.stack([xs[::3] + 0.25, np.full(len(xs[::3]), 0.25), np.full(len(xs[::3]), -3.0)], axis=1)
        rays_d = orc.make_rays(np.concatenate([o, o]), np.tile(np.array([[0.0, 0.0, 1.0]]), (2 * len(o), 1)), np.float64)
        ooff, oidx, _, _ = orc.traverse_flat(oflat, deep, rays_d, threads=orc.max_threads())
        fresh = Bvh.from_aabbs(scenes[1], ctx)          # (a tree object that has not given up yet: the asynchronous rebuild below does)
        dev_d = torch.from_numpy(deep).cuda()
        dev_rd = torch.from_numpy(rays_d.view(np.uint8).reshape(-1)).cuda()
        rbd = RayBatch.from_device(dev_rd, len(rays_d), np.float64)
        for _ in range(2):
            fresh.rebuild_async(dev_d)
            h = fresh.traverse_async(rbd)
            h.wait()
            off, idx = h.fetch(len(rays_d))
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and len(idx) > 0
        assert fresh.nodes.tobytes() == ot.nodes.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193, 30000])
def test_parity_mid_tier_boundaries(eng, orc, n, dtype):
    """sizes around MID_MAX = 4096 (workgroup tier) with clustered data so sub-node sizes vary widely."""
    rng = np.random.default_rng(n)
    centres = rng.uniform(-1000, 1000, size=(37, 3))
    which = rng.integers(0, 37, size=n)
    lo = (centres[which] + rng.normal(scale=rng.uniform(0.01, 30, size=(37, 1))[which], size=(n, 3))).astype(dtype)
    ext = rng.uniform(0, 2, size=(n, 3)).astype(dtype)
    aabbs = np.concatenate([lo, lo + ext], axis=1)
    o = rng.uniform(-1100, 1100, size=(500, 3)).astype(dtype)
    d = rng.normal(size=(500, 3)).astype(dtype)
    _full_parity(eng, orc, aabbs, orc.make_rays(o, d, dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lazy_flatten_same_arrays_whoever_asks_first(eng, orc, dtype):
    """BVHGPU_TUNE_FLATTEN_LAZY (default on): the flatten behind a build writes what the wide walk reads; the FlatNode array
    (flat_bvh.rs:60-143), the folded binary array and its LDS slot table follow when something reads them.  Whatever asks
    first — bvhgpu_flat_nodes, a STATS / t-slice (binary) walk, nearest_to, the scene blob, a refit — sees the arrays an eager
    flatten writes, and a wide walk that never asks gives the same CSR."""
    from bvh_amd import Bvh, Context, FlatBvh, testbase as tb
    from bvh_amd._lib import TUNE_FLATTEN_INLINE, TUNE_FLATTEN_LAZY
    _, aabbs = tb.create_n_cubes(1700)
    aabbs = aabbs.astype(dtype)
    ot = orc.build(aabbs)
    oflat = orc.flatten(ot.nodes)
    rays = orc.create_rays(0, 40_000, tb.default_bounds(), dtype)
    ooff, oidx, ots, ost = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    pts = np.random.default_rng(3).uniform(-900, 900, size=(500, 3)).astype(dtype)
    firsts = ["flat_nodes", "stats_walk", "wide_walk_then_flat", "scene_blob", "nearest", "async_step"]
    # lazy 2: the second pass at once, on the side stream beside the walk; 3: the FlatNode array at once, the binary array on first use (bench.py's step);
    # inline 1 (default): the builder's wave tier writes the FLAT / WIDE parts of its own subtrees (BVHGPU_TUNE_FLATTEN_INLINE), 0: the flatten kernel everything
    for lazy, inline in ((1, 1), (0, 1), (2, 1), (3, 1), (1, 0), (0, 0), (3, 0)):
        for first in firsts:
            ctx = Context(0)
            ctx.set_tuning(TUNE_FLATTEN_LAZY, lazy)
            ctx.set_tuning(TUNE_FLATTEN_INLINE, inline)
            bvh = Bvh.from_aabbs(aabbs, ctx)
            flat = bvh.flatten()
            if first == "flat_nodes":
                assert flat.nodes.tobytes() == oflat.tobytes()
            elif first == "stats_walk":
                off, idx, ts, st = flat.traverse_batch(_rb(eng, rays), want_t=True, stats=True)
                assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and st["visited"] == ost["visited"]
            elif first == "wide_walk_then_flat":
                off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
                assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
            elif first == "scene_blob":
                blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
                flat.scene_export(blob)
                peer = FlatBvh.scene_import(blob, len(blob), ctx)
                off, idx, _, st = peer.traverse_batch(_rb(eng, rays), stats=True)
                assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and st["visited"] == ost["visited"]
            elif first == "nearest":
                sh, dist = flat.nearest_batch(pts)
                osh, odist = orc.nearest(oflat, aabbs, pts)
                assert np.array_equal(sh, osh) and dist.tobytes() == odist.tobytes()
            else:   # the asynchronous triple of bench.py's step, twice, then every reader in turn
                import torch
                from bvh_amd import RayBatch
                dev_a = torch.from_numpy(aabbs).cuda()
                dev_r = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
                rb = RayBatch.from_device(dev_r, len(rays), dtype)
                for _ in range(2):
                    bvh.rebuild_async(dev_a)
                    st = bvh.traverse_async(rb).wait()
                    assert st["hits"] == ost["hits"]
            # afterwards everything agrees, in any order
            assert flat.nodes.tobytes() == oflat.tobytes(), (lazy, first)
            off, idx, _, st = flat.traverse_batch(_rb(eng, rays), stats=True)
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and st["leaf_visits"] == ost["leaf_visits"]
            off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
            # a refit to the same boxes re-flattens (lazily again): same arrays
            bvh.refit(aabbs)
            off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
            assert flat.nodes.tobytes() == oflat.tobytes(), (lazy, first, "after refit")


def test_rebuild_and_determinism(eng, orc):
    from bvh_amd import testbase as tb
    _, a1 = tb.create_n_cubes(500)
    _, a2 = tb.create_n_cubes(300)
    bvh = eng.Bvh.from_aabbs(a1)
    n1 = bvh.nodes.copy()
    bvh.rebuild(a2)
    assert bvh.nodes.tobytes() == orc.build(a2).nodes.tobytes()
    bvh.rebuild(a1)
    assert bvh.nodes.tobytes() == n1.tobytes()  # run twice, bit-compare (race / determinism check)


def test_hit_pool_growth_and_order(eng, orc):
    """many hits per ray (ray along a row of overlapping boxes): exercises pool overflow → replay,
    and pins per-ray order = flat-array (DFS) order."""
    n = 4000
    x = np.arange(n, dtype=np.float32) * np.float32(0.25)
    lo = np.stack([x, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
    aabbs = np.concatenate([lo, lo + np.float32(1.0)], axis=1)
    o = np.tile(np.array([-5, 0.5, 0.5], np.float32), (300, 1)); o[:, 1] += np.linspace(0, 0.4, 300, dtype=np.float32)
    d = np.tile(np.array([1, 0, 0], np.float32), (300, 1))
    rays = orc.make_rays(o, d)
    bvh, flat, ot, oflat = _full_parity(eng, orc, aabbs, rays)
    off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
    assert off[-1] == 300 * n  # every ray reports every box: 1.2 M hits from 300 rays


def test_device_ray_stream_matches_reference_generator(eng, orc):
    import torch
    from bvh_amd import testbase as tb
    from bvh_amd._lib import RAY_F32
    ctx = eng.default_context()
    buf = torch.empty(4096 * RAY_F32.itemsize, dtype=torch.uint8, device="cuda")
    eng.RayBatch.generate(999_000, 4096, tb.default_bounds(), buf, np.float32, ctx)
    ctx.synchronize()
    got = buf.cpu().numpy().view(RAY_F32)
    assert got.tobytes() == orc.create_rays(999_000, 4096).tobytes()
    # the f64 twin (BASELINE.json configs[4]): the same f32 points, widened BEFORE Ray::new
    from bvh_amd._lib import RAY_F64
    buf64 = torch.empty(4096 * RAY_F64.itemsize, dtype=torch.uint8, device="cuda")
    eng.RayBatch.generate(999_000, 4096, tb.default_bounds(), buf64, np.float64, ctx)
    ctx.synchronize()
    assert buf64.cpu().numpy().view(RAY_F64).tobytes() == orc.create_rays(999_000, 4096, dtype=np.float64).tobytes()
    # Ray::new on device == oracle Ray::new (sqrt and divides correctly rounded)
    rng = np.random.default_rng(5)
    o = rng.normal(size=(1000, 3)).astype(np.float32) * 1e3
    d = rng.normal(size=(1000, 3)).astype(np.float32)
    assert eng.RayBatch.new(o, d).host.tobytes() == orc.make_rays(o, d).tobytes()
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    assert eng.RayBatch.new(o64, d64, np.float64).host.tobytes() == orc.make_rays(o64, d64, np.float64).tobytes()


def test_uploaded_flatbvh_and_scene_blob(eng, orc):
    """bvhgpu_tree_from_flat (a FlatBvh built elsewhere; shapes MOVED since the build, so the leaf
    re-test of flat_bvh.rs:411-418 matters) and the multi-GPU scene blob round trip."""
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(200)
    ot = orc.build(aabbs)
    oflat = orc.flatten(ot.nodes)
    moved = aabbs.copy()
    moved[::3, [0, 3]] += np.float32(0.75)  # shapes moved after the build: navigator boxes are stale
    rays = orc.create_rays(0, 3000)
    up = eng.FlatBvh.from_flat_nodes(oflat, moved)
    off, idx, _, st = up.traverse_batch(_rb(eng, rays), stats=True)
    ooff, oidx, _, ost = orc.traverse_flat(oflat, moved, rays)
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    assert st["visited"] == ost["visited"] and st["leaf_visits"] == ost["leaf_visits"]
    # scene blob: export → (broadcast) → import gives the same hit lists
    bvh = eng.Bvh.from_aabbs(aabbs)
    flat = bvh.flatten()
    blob = np.zeros(flat.scene_nbytes(), dtype=np.uint8)
    flat.scene_export(blob)
    peer = eng.FlatBvh.scene_import(blob, len(blob))
    a = flat.traverse_batch(_rb(eng, rays))
    b = peer.traverse_batch(_rb(eng, rays))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    peer2 = eng.FlatBvh.scene_import(blob, len(blob), reuse=peer)
    assert peer2 is peer


def test_full_size_properties_1m_rays(eng, orc):
    """BASELINE.json configs[1] at full size (120 k triangles, 1 M rays) through size-independent
    properties: CSR well-formedness, bench-quirk closed form (first 5 000 rays start inside cube 2k and
    return exactly the two triangles of one face; later rays of this stream return nothing),
    recursive-vs-flat agreement on a sample, chunked == whole, device-resident rays == host rays."""
    import torch
    from bvh_amd import testbase as tb
    from bvh_amd._lib import RAY_F32
    _, aabbs = tb.create_n_cubes(10_000)
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    R = 1_000_000
    ctx = eng.default_context()
    buf = torch.empty(R * RAY_F32.itemsize, dtype=torch.uint8, device="cuda")
    rays_dev = eng.RayBatch.generate(0, R, tb.default_bounds(), buf, np.float32, ctx)
    off, idx, _, st = flat.traverse_batch(rays_dev, stats=True)
    assert off[0] == 0 and off[-1] == len(idx) and np.all(np.diff(off.astype(np.int64)) >= 0)
    cnt = np.diff(off.astype(np.int64))
    assert np.all(cnt[:5000] == 2) and np.all(cnt[5000:] == 0)
    pairs = idx.reshape(-1, 2)
    k = np.arange(5000)
    assert np.all(pairs // 12 == (2 * k)[:, None])        # both candidates belong to cube 2k
    assert np.all(pairs[:, 0] // 2 == pairs[:, 1] // 2)   # the two triangles of one face (shared AABB)
    # the same stream, chunked and from host memory: identical CSR pieces
    rays_host = orc.create_rays(0, 20_000)
    o2, i2, _, _ = flat.traverse_batch(_rb(eng, rays_host))
    assert np.array_equal(o2, off[:20_001]) and np.array_equal(i2, idx[:off[20_000]])
    # recursive Bvh::traverse (oracle) == flat traverse (GPU) on a sample: bvh_node.rs:288-319 vs flat_bvh.rs:396-431
    ot = orc.build(aabbs)
    ro, ri = orc.traverse_tree(ot.nodes, aabbs, rays_host[:6000])
    assert np.array_equal(ro, off[:6001]) and np.array_equal(ri, idx[:off[6000]])
    # slab tests per ray: SURVEY §8d re-derived on the device
    assert 60 < st["visited"] / R < 90


# ------------------------------------------------------------------ traversal variants (tuning knobs never change results)
@pytest.mark.parametrize("variant,slots,threads", [(0, 0, 0), (1, 0, 0), (2, 5056, 1024), (2, 2048, 1024), (2, 300, 256),
                                                   (2, 4, 64)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_traversal_variants_same_result(eng, orc, variant, slots, threads, dtype):
    """one ray per lane / persistent waves with refill / LDS-resident top of the tree: identical CSR (order
    included), t-slices and reference-equivalent visit counters on scenes that stress every path: deep and
    shallow walks, many hits per ray (per-wave pool chunks + overflow replay), axis-parallel and in-plane
    rays (non-finite inverse directions → exact NaN-aware slab test), n = 1 and n = 2 trees, an uploaded
    FlatBvh whose shapes moved."""
    from bvh_amd import Context
    from bvh_amd._lib import (TUNE_TRAVERSE_LDS_MIN_RAYS, TUNE_TRAVERSE_LDS_SLOTS, TUNE_TRAVERSE_LDS_THREADS,
                              TUNE_TRAVERSE_VARIANT)
    ctx = Context(0)
    ctx.set_tuning(TUNE_TRAVERSE_VARIANT, variant)
    ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    if variant == 2:
        ctx.set_tuning(TUNE_TRAVERSE_LDS_SLOTS, slots)
        ctx.set_tuning(TUNE_TRAVERSE_LDS_THREADS, threads)
    _variant_suite(eng, orc, ctx, dtype)


@pytest.mark.parametrize("items,stack_lds,wg_per_cu,threads,slots", [(-1, -1, 0, 0, 0), (0, 8, 2, 1024, 0), (1, 8, 2, 1024, 0),
                                                                      (2, 8, 2, 1024, 0), (2, 0, 2, 512, 0), (1, 2, 1, 1024, 0),
                                                                      (0, 3, 4, 256, 1), (2, 32, 1, 64, 5), (1, 6, 2, 512, 341),
                                                                      (2, 3, 2, 256, 21)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wide_walk_same_result(eng, orc, items, stack_lds, wg_per_cu, threads, slots, dtype):
    """The wide walk (four grandchild boxes per step, k_traverse_wide) under every geometry knob: 1 / 4 / 16 items per ray,
    the per-lane stack entirely in LDS / entirely in HBM / split, 1..4 workgroups per CU, 1..341 resident top nodes.
    Same scenes as the other variants: the CSR must equal the oracle's, order included."""
    from bvh_amd import Context
    from bvh_amd._lib import (TUNE_TRAVERSE_LDS_MIN_RAYS, TUNE_TRAVERSE_VARIANT, TUNE_WIDE_ITEMS_LOG4, TUNE_WIDE_SLOTS,
                              TUNE_WIDE_STACK_LDS, TUNE_WIDE_THREADS, TUNE_WIDE_WG_PER_CU)
    ctx = Context(0)
    ctx.set_tuning(TUNE_TRAVERSE_VARIANT, 3)
    ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    ctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, items)
    ctx.set_tuning(TUNE_WIDE_STACK_LDS, stack_lds)
    ctx.set_tuning(TUNE_WIDE_WG_PER_CU, wg_per_cu)
    ctx.set_tuning(TUNE_WIDE_THREADS, threads)
    ctx.set_tuning(TUNE_WIDE_SLOTS, slots)
    _variant_suite(eng, orc, ctx, dtype, deep=True)


def _variant_suite(eng, orc, ctx, dtype, deep=False):
    rng = np.random.default_rng(77)

    def check(aabbs, rays, flat_upload=None, counters=True):
        aabbs = aabbs.astype(dtype)
        if flat_upload is None:
            tree = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
            oflat = orc.flatten(orc.build(aabbs).nodes)
            cur = aabbs
        else:
            oflat, cur = flat_upload
            tree = eng.FlatBvh.from_flat_nodes(oflat, cur, ctx)
        rb = eng.RayBatch(len(rays), dtype, host=np.ascontiguousarray(rays))
        off, idx, ts, st = tree.traverse_batch(rb, want_t=True, stats=True)
        ooff, oidx, ots, ost = orc.traverse_flat(oflat, cur, rays, want_t=True, threads=orc.max_threads())
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        if len(idx):
            assert same_bytes(ts, ots)
        if counters:
            assert (st["hits"], st["visited"], st["leaf_visits"]) == (ost["hits"], ost["visited"], ost["leaf_visits"])
        off2, idx2, _, _ = tree.traverse_batch(rb)          # the NaN-free fast slab test (no t-slice requested)
        assert np.array_equal(off2, ooff) and np.array_equal(idx2, oidx)

    # clustered boxes, generic + axis-parallel + in-plane rays
    n = 20000
    lo = rng.integers(-60, 60, size=(n, 3)).astype(dtype) + rng.uniform(0, 1, size=(n, 3)).round(1).astype(dtype)
    ext = rng.integers(0, 4, size=(n, 3)).astype(dtype)
    aabbs = np.concatenate([lo, lo + ext], axis=1)
    o = rng.uniform(-70, 70, size=(9000, 3)).astype(dtype)
    d = rng.normal(size=(9000, 3)).astype(dtype)
    d[:1500] = rng.integers(-1, 2, size=(1500, 3))
    d[np.all(d == 0, axis=1)] = [0, 1, 0]
    o[:700] = np.round(o[:700])                              # origins on box face planes
    check(aabbs, orc.make_rays(o, d, dtype))
    # many hits per ray
    m = 3000
    x = np.arange(m, dtype=dtype) * dtype(0.25)
    lo2 = np.stack([x, np.zeros(m, dtype), np.zeros(m, dtype)], axis=1)
    row = np.concatenate([lo2, lo2 + dtype(1.0)], axis=1)
    o2 = np.tile(np.array([-5, 0.5, 0.5], dtype), (200, 1)); o2[:, 1] += np.linspace(0, 0.4, 200).astype(dtype)
    check(row, orc.make_rays(o2, np.tile(np.array([1, 0, 0], dtype), (200, 1)), dtype))
    # tiny trees
    for k in (1, 2, 3):
        check(aabbs[:k], orc.make_rays(o[:500], d[:500], dtype))
    # uploaded FlatBvh, shapes moved
    small = aabbs[:3000].astype(dtype)
    oflat = orc.flatten(orc.build(small).nodes)
    moved = small.copy(); moved[::3, [0, 3]] += dtype(0.75)
    check(small, orc.make_rays(o[:4000], d[:4000], dtype), flat_upload=(oflat, moved))
    if deep:
        # a very unbalanced tree (SAH peels a few hundred shapes per level) with rays through ALL boxes: the per-lane stack of
        # the wide walk leaves LDS, then its HBM part; beyond that the batch must be replayed with the stackless binary walk
        nd = 6000
        xs = dtype(1.004) ** np.arange(nd, dtype=dtype)
        lo3 = np.stack([xs, np.zeros(nd, dtype), np.zeros(nd, dtype)], axis=1)
        chain = np.concatenate([lo3, lo3 + dtype(0.5)], axis=1)
        o3 = np.zeros((300, 3), dtype); o3[:, 0] = -1; o3[:, 1] = np.linspace(0.01, 0.49, 300); o3[:, 2] = 0.25
        d3 = np.tile(np.array([1, 0, 0], dtype), (300, 1)); d3[::7] = [1, 0.001, 0]
        check(chain, orc.make_rays(o3, d3, dtype))
        # splits with no SAH winner: boxes so far apart that every surface area overflows to inf make every cost NaN, so
        # min_bucket stays 0 and both children get EMPTY bounds (bvh_node.rs:225-230) — a child box is then not the join of
        # its grandchildren and the engine must keep to the walk that tests every ancestor
        big = dtype(1e19 if dtype == np.float32 else 1e154)
        lo4 = (rng.uniform(-1, 1, size=(500, 3)) * big).astype(dtype)
        far = np.concatenate([lo4, lo4 + big * dtype(0.01)], axis=1)
        o4 = (rng.uniform(-1, 1, size=(600, 3)) * big).astype(dtype)
        # (the visit COUNTERS are not compared here: the engine folds a leaf's navigator and leaf entries into one test of
        # the shape's AABB, which gives the same hits but does not count the leaf-entry visit behind an empty navigator box)
        check(far, orc.make_rays(o4, d[:600], dtype), counters=False)


# ------------------------------------------------------------------ triangle stage
def _pairs_oracle(orc, rays, tris):
    n = len(rays)
    isect, _, _ = orc.triangle_stage(tris, rays, np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    return isect


def _triangle_cases(rng, n, dtype, spread):
    a = rng.uniform(-spread, spread, size=(n, 3)).astype(dtype)
    b = a + rng.normal(scale=spread * 0.1, size=(n, 3)).astype(dtype)
    c = a + rng.normal(scale=spread * 0.1, size=(n, 3)).astype(dtype)
    tris = np.stack([a, b, c], axis=1)
    u = rng.integers(0, 101, size=n)
    v = np.minimum(100 - u, rng.integers(0, 101, size=n))
    p = a + (u[:, None] / 100.0).astype(dtype) * (b - a) + (v[:, None] / 100.0).astype(dtype) * (c - a)
    o = rng.uniform(-spread, spread, size=(n, 3)).astype(dtype)
    d = (p - o).astype(dtype)
    k = n // 8
    d[:k] = rng.normal(size=(k, 3))                         # random directions: mostly misses
    tris[k:2 * k, 2] = tris[k:2 * k, 1]                     # degenerate (zero-area) triangles: det == 0
    o[2 * k:3 * k] = a[2 * k:3 * k]                         # origin on a vertex
    d[2 * k:3 * k] = (b - a)[2 * k:3 * k]                   # ray inside the triangle's plane
    return tris, o, d, (u, v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ray_triangle_pairs_bit_exact(eng, orc, dtype):
    """Ray::intersects_triangle (ray_impl.rs:154-213) on the device == the oracle's restatement, bit for bit,
    for every field of Intersection including the u / v left behind by the early returns."""
    from bvh_amd.api import intersect_triangle_pairs
    rng = np.random.default_rng(2024)
    for spread in (1.0, 1e3, 1e10):
        tris, o, d, _ = _triangle_cases(rng, 20000, dtype, spread)
        rays = orc.make_rays(o, d, dtype)
        got = intersect_triangle_pairs(_rb(eng, rays), tris)
        want = _pairs_oracle(orc, rays, tris)
        assert got.tobytes() == want.tobytes()
        assert np.isfinite(want[:, 0]).sum() > 1000        # the sample does exercise real hits


def test_reference_ray_hits_triangle_property(eng, orc):
    """the reference's proptest test_ray_hits_triangle (ray_impl.rs:361-420) on the device implementation."""
    from bvh_amd.api import intersect_triangle_pairs
    rng = np.random.default_rng(7)
    n = 50000
    f = np.float32
    a, b, c, origin = (rng.uniform(-10e10, 10e10, size=(n, 3)).astype(f) for _ in range(4))
    u16 = rng.integers(0, 65536, size=n); v16 = rng.integers(0, 65536, size=n)
    u = u16 % 101
    v = np.minimum(100 - u, v16 % 101)
    uf = (u.astype(f) / f(100.0)); vf = (v.astype(f) / f(100.0))
    u_vec = b - a; v_vec = c - a
    with np.errstate(all="ignore"):
        normal = np.cross(u_vec, v_vec).astype(f)
        p = a + uf[:, None] * u_vec + vf[:, None] * v_vec
        d = (p - origin).astype(f)
        on_back = (normal * (origin - a)).astype(f).sum(axis=1) <= 0
    rays = orc.make_rays(origin, d, f)
    tris = np.stack([a, b, c], axis=1)
    r = intersect_triangle_pairs(_rb(eng, rays), tris)
    assert r.tobytes() == _pairs_oracle(orc, rays, tris).tobytes()
    dist, ru, rv = r[:, 0], r[:, 1], r[:, 2]
    eps = np.finfo(f).eps
    with np.errstate(all="ignore"):
        uv = ru + rv
        inside = (uv >= 0) & (uv <= 1) & (dist < np.inf)
    border = (np.abs(uf) < eps) | (np.abs(uf - 1) < eps) | (np.abs(vf) < eps) | (np.abs(vf - 1) < eps) | (np.abs(uf + vf - 1) < eps)
    # numpy's sum order differs from nalgebra's dot only in rounding: skip the few cases at the plane itself
    clear = np.abs((normal * (origin - a)).sum(axis=1)) > 1e-3 * np.abs(normal * (origin - a)).sum(axis=1)
    assert np.all(dist[on_back & clear] == np.inf)
    ok = inside | border
    # the reference's own property is only approximately true at |coords| ~ 1e11 in f32 (it is a proptest with
    # regression seeds); require it on the overwhelming majority and identically on the oracle
    assert ok[~on_back & clear].mean() > 0.95


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_triangle_stage_matches_reference_loop(eng, orc, variant, dtype):
    """traverse + intersects_triangle on every candidate (testbase.rs:826-836): per-candidate Intersection in
    CSR order and the closest hit per ray, against the oracle's restatement of that loop."""
    from bvh_amd import Context, testbase as tb
    from bvh_amd._lib import TUNE_TRAVERSE_LDS_MIN_RAYS, TUNE_TRAVERSE_VARIANT
    ctx = Context(0)
    ctx.set_tuning(TUNE_TRAVERSE_VARIANT, variant)
    ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    tris32, aabbs32 = tb.create_n_cubes(3000)
    tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
    rng = np.random.default_rng(3)
    n = 40000
    centres = tris.reshape(3000, 36, 3)[:, :, :].mean(axis=1)          # cube centres
    target = centres[rng.integers(0, 3000, size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3))
    o = rng.uniform(-1e5, 1e5, size=(n, 3)).astype(dtype)
    d = (target - o).astype(dtype)
    d[: n // 10] = rng.normal(size=(n // 10, 3))                        # some rays that hit nothing
    rays = orc.make_rays(o, d, dtype)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    flat = bvh.flatten()
    flat.set_triangles(tris)
    off, idx, isect, st = flat.intersect_triangles(_rb(eng, rays), stats=True)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    ooff, oidx, _, ost = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    oisect, oclosest, oprim = orc.triangle_stage(tris, rays, ooff, oidx)
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    assert isect.tobytes() == oisect.tobytes()
    assert st["visited"] == ost["visited"]
    cl, prim, st2 = flat.closest_hits(_rb(eng, rays), stats=True)
    assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
    assert st2["hits"] == ost["hits"] and st2["visited"] == ost["visited"]
    hit = np.isfinite(oclosest[:, 0])
    assert hit.sum() > n // 2 and (~hit).sum() > n // 20               # both outcomes are exercised
    # the same batch without STATS: the default walk of a batch this size — the wide walk over 16 items per ray, the ray's nearest candidate
    # taken as a minimum over its items (f32: WalkOut::closest_key + k_closest_resolve; f64: (ray, item) slots + k_closest_resolve_slots)
    ctx3 = Context(0)                                                    # default tuning: the wide walk for batches of 16 384 rays and more
    flat3 = eng.Bvh.from_aabbs(aabbs, ctx3).flatten()
    flat3.set_triangles(tris)
    cl2, prim2, st3 = flat3.closest_hits(_rb(eng, rays))
    assert cl2.tobytes() == oclosest.tobytes() and np.array_equal(prim2, oprim)
    # (f64: the candidates filed by (ray, item), k_closest_resolve_slots — walked over the f32 guide boxes, every candidate's box and triangle decided
    #  in f64; with the guide off, the f64 walk)
    assert flat3._hits.walk_kernel().startswith("bvhgpu::k_traverse_wide<float, 3, 2, 1024, 8, %d>" % (0 if dtype == np.float32 else 1))
    if dtype == np.float64:
        from bvh_amd._lib import TUNE_WIDE_F64_GUIDE
        ctx3.set_tuning(TUNE_WIDE_F64_GUIDE, 0)
        cl2b, prim2b, _ = flat3.closest_hits(_rb(eng, rays))
        assert cl2b.tobytes() == oclosest.tobytes() and np.array_equal(prim2b, oprim)
        assert flat3._hits.walk_kernel().startswith("bvhgpu::k_traverse_wide<double, 3, 2,")
        ctx3.set_tuning(TUNE_WIDE_F64_GUIDE, 1)
    # ... and where the minimum is not unique: pairs of overlapping coplanar triangles (planes z = const, a ray along +z meets both at exactly
    # the same distance) whose centroids lie far apart, so that they sit in different subtrees — different ITEMS of the ray.  The reference keeps
    # the candidate its loop meets first (strict <, testbase.rs:831-833): the key's item number must reproduce that order.
    planes = np.arange(-400, 401, 50, dtype=np.float64)
    big = []
    for z in planes:
        big.append([[-2000.0, -600.0, z], [300.0, -600.0, z], [-400.0, 1200.0, z]])   # centroid x = -700
        big.append([[-300.0, -600.0, z], [2000.0, -600.0, z], [400.0, 1200.0, z]])    # centroid x = +700: the root's split parts them; they overlap around x = 0
    big = np.array(big)
    tris_t = np.concatenate([tris.reshape(-1, 3, 3), big.astype(dtype)]).astype(dtype)
    aabbs_t = np.concatenate([tris_t.min(axis=1), tris_t.max(axis=1)], axis=1).astype(dtype)
    m = 30000
    ot_ = rng.uniform(-150, 150, size=(m, 3)); ot_[:, 2] = rng.choice(np.concatenate([planes - 25.0, [-1000.0]]), size=m)
    dt_ = np.tile(np.array([[0.0, 0.0, 1.0]]), (m, 1)); dt_[m // 2:] *= -1.0          # half of them look down: the order of the planes flips
    rays_t = orc.make_rays(ot_.astype(dtype), dt_.astype(dtype), dtype)
    flat_t = eng.Bvh.from_aabbs(aabbs_t, ctx3).flatten()
    flat_t.set_triangles(tris_t)
    oflat_t = orc.flatten(orc.build(aabbs_t).nodes)
    toff, tidx, _, _ = orc.traverse_flat(oflat_t, aabbs_t, rays_t, threads=orc.max_threads())
    tisect, tclosest, tprim = orc.triangle_stage(tris_t, rays_t, toff, tidx)
    d_all = tisect[:, 0]
    ties = sum(1 for r in range(0, m, 7) if np.isfinite(tclosest[r, 0]) and (d_all[toff[r]:toff[r + 1]] == tclosest[r, 0]).sum() > 1)
    assert ties > 300, ties                                              # the scene does produce equal nearest distances (every one of them across subtrees)
    cl3, prim3, _ = flat_t.closest_hits(_rb(eng, rays_t))
    assert cl3.tobytes() == tclosest.tobytes() and np.array_equal(prim3, tprim)
    cl4, prim4, _ = flat_t.closest_hits(_rb(eng, rays_t), stats=True)    # (the binary walk: one lane owns the ray)
    assert cl4.tobytes() == tclosest.tobytes() and np.array_equal(prim4, tprim)
    # flags that cannot be combined / missing triangles fail loudly
    bare = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    with pytest.raises(eng.BvhGpuError):
        bare.closest_hits(_rb(eng, rays[:10]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [48, 700, 6000])
def test_parity_signed_zero_bounds(eng, orc, n, dtype):
    """-0.0 and +0.0 coordinates: every join of the builder (integer keys in the level tier, v_min/v_max in
    the wave tier, LDS atomics in the workgroup tiers) must order -0 < +0 like the oracle, byte for byte."""
    rng = np.random.default_rng(n)
    vals = np.array([-0.0, 0.0, -1.0, 1.0, -0.5, 0.5, 2.0], dtype=dtype)
    lo = vals[rng.integers(0, len(vals), size=(n, 3))]
    hi = vals[rng.integers(0, len(vals), size=(n, 3))]
    mn = np.where(lo <= hi, lo, hi); mx = np.where(lo <= hi, hi, lo)
    # keep the signed zeros that np.where picked: (-0.0 <= 0.0) is True, so min may be -0.0 or +0.0 by position
    aabbs = np.concatenate([mn, mx], axis=1).astype(dtype)
    assert np.signbit(aabbs[aabbs == 0]).any() and (~np.signbit(aabbs[aabbs == 0])).any()
    o = rng.uniform(-3, 3, size=(400, 3)).astype(dtype)
    d = rng.normal(size=(400, 3)).astype(dtype)
    _full_parity(eng, orc, aabbs, orc.make_rays(o, d, dtype))


# ------------------------------------------------------------------ point query (BoundingHierarchy::nearest_to)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nearest_to_reference_doc_example_and_parity(eng, orc, dtype):
    """flat_bvh.rs:440-508 doc example (1000 unit boxes at (i,i,i), query (5.0,5.7,5.3) → id 5) through the
    trait-surface mirror, then shape and distance against the oracle's flat loop, bit for bit: AABB-distance
    shapes (UnitBox) and triangles, built and uploaded trees, n = 1 and the empty hierarchy."""
    from bvh_amd import testbase as tb
    boxes = [tb.UnitBox(i, (float(i), float(i), float(i))) for i in range(1000)]
    for builder in (eng.Bvh.build, eng.FlatBvh.build):
        bh = builder(boxes, dtype)
        got = bh.nearest_to([5.0, 5.7, 5.3], boxes)
        assert got[0].id == 5 and abs(got[1] - 0.2) < 1e-6
    assert eng.Bvh.build([], dtype).nearest_to([0, 0, 0], []) is None
    one = eng.FlatBvh.build(boxes[:1], dtype)
    assert one.nearest_to([3, 0, 0], boxes[:1])[0].id == 0
    rng = np.random.default_rng(21)
    tris32, aabbs32 = tb.create_n_cubes(1500)
    tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
    pts = np.concatenate([rng.uniform(-1e5, 1e5, size=(6000, 3)), tris[rng.integers(0, len(tris), 2000)].mean(axis=1)
                          + rng.normal(scale=2.0, size=(2000, 3)), tris[:500, 0]]).astype(dtype)
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    flat.set_triangles(tris)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    for use_tris in (False, True):
        s, d = flat.nearest_batch(pts, triangles=use_tris)
        os_, od = orc.nearest(oflat, aabbs, pts, tris if use_tris else None)
        assert np.array_equal(s, os_) and d.tobytes() == od.tobytes()
    # uploaded FlatBvh whose shapes moved: stale navigator boxes, current shape distances (flat_bvh.rs:538)
    moved = aabbs.copy(); moved[::3, [0, 3]] += dtype(0.75)
    up = eng.FlatBvh.from_flat_nodes(oflat, moved)
    s, d = up.nearest_batch(pts[:3000])
    os_, od = orc.nearest(oflat, moved, pts[:3000])
    assert np.array_equal(s, os_) and d.tobytes() == od.tobytes()
    with pytest.raises(eng.BvhGpuError):
        up.nearest_batch(pts[:10], triangles=True)      # no triangles were set on this tree


# ------------------------------------------------------------------ ordered traversal
def test_ordered_traversal_reference_known_answers(eng):
    """child_distance_traverse.rs tests: on the 21 aligned boxes the nearest / farthest child iterators return the
    golden hit sets of testbase.rs:174-225, ordered by entry distance ascending / descending."""
    from bvh_amd import testbase as tb
    shapes = tb.generate_aligned_boxes()
    bvh = eng.Bvh.build(shapes)
    flat = bvh.flatten()
    for case in GOLD["aligned_boxes"]["rays"]:
        ray = eng.Ray(case["origin"], case["direction"])
        near = flat.nearest_child_traverse(ray, shapes)
        far = flat.farthest_child_traverse(ray, shapes)
        assert sorted(s.id for s in near) == sorted(case["hit_ids"]) == sorted(s.id for s in far)
        dn = [ray.intersection_slice_for_aabb(s.aabb())[0] for s in near]
        df = [ray.intersection_slice_for_aabb(s.aabb())[0] for s in far]
        assert dn == sorted(dn) and df == sorted(df, reverse=True)
    empty = eng.Bvh.build([]).flatten()
    assert empty.nearest_child_traverse(eng.Ray([0, 0, 0], [1, 0, 0]), []) == []


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ordered_traversal_matches_iterator_restatement(eng, orc, dtype):
    """CSR in the order of Bvh::nearest_child_traverse_iterator / farthest_child_traverse_iterator against the
    oracle's state-for-state restatement: cube scene, clustered boxes with axis-parallel and in-plane rays, tiny
    trees; per-candidate triangle Intersections and the closest hit in that order; a tree deeper than the
    iterator's 32-entry stack is an error (the reference panics)."""
    from bvh_amd import testbase as tb
    rng = np.random.default_rng(31)
    tris32, aabbs32 = tb.create_n_cubes(2000)
    tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
    centres = tris.reshape(2000, 36, 3).mean(axis=1)
    n = 20000
    o = rng.uniform(-1e5, 1e5, size=(n, 3)).astype(dtype)
    d = (centres[rng.integers(0, 2000, size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3)) - o).astype(dtype)
    d[:2000] = rng.normal(size=(2000, 3))
    rays = orc.make_rays(o, d, dtype)
    bvh = eng.Bvh.from_aabbs(aabbs)
    flat = bvh.flatten()
    flat.set_triangles(tris)
    onodes = orc.build(aabbs).nodes
    foff, fidx, _, _ = flat.traverse_batch(_rb(eng, rays))
    for order, asc in (("nearest", True), ("farthest", False)):
        off, idx, _, _ = flat.traverse_batch(_rb(eng, rays), order=order)
        ooff, oidx = orc.traverse_child_ordered(onodes, aabbs, rays, asc)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        assert np.array_equal(off, foff) and not np.array_equal(idx, fidx)      # same sets per ray, another order
        off2, idx2, isect, _ = flat.intersect_triangles(_rb(eng, rays), order=order)
        oisect, oclosest, oprim = orc.triangle_stage(tris, rays, ooff, oidx)
        assert np.array_equal(idx2, oidx) and isect.tobytes() == oisect.tobytes()
        cl, prim, _ = flat.closest_hits(_rb(eng, rays), order=order)
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
    # clustered integer boxes, axis-parallel / in-plane rays (NaN → None in intersection_slice_for_aabb)
    m = 5000
    lo = rng.integers(-30, 30, size=(m, 3)).astype(dtype); ext = rng.integers(0, 4, size=(m, 3)).astype(dtype)
    boxes = np.concatenate([lo, lo + ext], axis=1)
    o2 = np.round(rng.uniform(-35, 35, size=(3000, 3))).astype(dtype)
    d2 = rng.integers(-1, 2, size=(3000, 3)).astype(dtype); d2[np.all(d2 == 0, axis=1)] = [0, 0, 1]
    rays2 = orc.make_rays(o2, d2, dtype)
    for k in (m, 3, 2, 1):
        b = eng.Bvh.from_aabbs(boxes[:k]).flatten()
        on = orc.build(boxes[:k]).nodes
        for order, asc in (("nearest", True), ("farthest", False)):
            off, idx, _, _ = b.traverse_batch(_rb(eng, rays2), order=order)
            ooff, oidx = orc.traverse_child_ordered(on, boxes[:k], rays2, asc)
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    # deeper than 32 levels: the reference's fixed stack overflows (panic) → BVHGPU_OVERFLOW here
    q = 42
    x = 8.0 ** np.arange(q, dtype=np.float64)                  # one shape peeled per level: depth 41 (f64: no overflow in SA)
    deep = np.stack([x, np.zeros(q), np.zeros(q), x * 1.5, np.ones(q), np.ones(q)], axis=1)
    along = orc.make_rays(np.array([[-1, 0.25, 0.25]], np.float64), np.array([[1, 0, 0]], np.float64), np.float64)
    assert orc.tree_stats(orc.build(deep).nodes, deep)["max_depth"] > 33
    db = eng.Bvh.from_aabbs(deep).flatten()
    with pytest.raises(OverflowError):
        orc.traverse_child_ordered(orc.build(deep).nodes, deep, along, True)
    with pytest.raises(eng.BvhGpuError) as e:
        db.traverse_batch(_rb(eng, along), order="nearest")
    assert "32" in str(e.value)


def test_best_first_traversal_reference_known_answers(eng):
    """distance_traverse.rs tests on the engine: golden hit sets of the 21 aligned boxes with monotone entry distances
    (:188-262), the empty tree (:270-281), single-node trees (bvh_impl.rs:667-690), test_overlapping_child_order (:295-322)."""
    from bvh_amd import testbase as tb
    shapes = tb.generate_aligned_boxes()
    flat = eng.Bvh.build(shapes).flatten()
    for case in GOLD["aligned_boxes"]["rays"]:
        ray = eng.Ray(case["origin"], case["direction"])
        near = flat.nearest_traverse(ray, shapes)
        far = flat.farthest_traverse(ray, shapes)
        assert sorted(s.id for s in near) == sorted(case["hit_ids"]) == sorted(s.id for s in far)
        dn = [ray.intersection_slice_for_aabb(s.aabb())[0] for s in near]
        df = [ray.intersection_slice_for_aabb(s.aabb())[0] for s in far]
        assert dn == sorted(dn) and df == sorted(df, reverse=True)
    empty = eng.Bvh.build([]).flatten()
    assert empty.nearest_traverse(eng.Ray([0, 0, 0], [1, 0, 0]), []) == []
    assert empty.farthest_traverse(eng.Ray([0, 0, 0], [1, 0, 0]), []) == []
    one = [tb.UnitBox(0, np.array([0.0, 0.0, 0.0], np.float32))]
    f1 = eng.Bvh.build(one).flatten()
    assert f1.nearest_traverse(eng.Ray([0, 2, 0], [1, 0, 0]), one) == []
    assert len(f1.nearest_traverse(eng.Ray([-5, 0, 0], [1, 0, 0]), one)) == 1
    ov = np.array([[-0.33333334, -5000.3335, -5000.3335, 1.3333334, 0.33333334, 0.33333334],
                   [-5000.3335, -5000.3335, -5000.3335, 0.33333334, 0.33333334, -4998.6665],
                   [-5000.3335, -5000.3335, -5000.3335, 0.33333334, 0.33333334, 5000.3335]], np.float32)
    fo = eng.Bvh.from_aabbs(ov).flatten()
    ray = eng.Ray([-5000.0, -5000.0, -5000.0], [1, 0, 0])
    _, idx, _, _ = fo.traverse_batch(ray._batch, order="nearest_heap")
    assert sorted(idx.tolist()) == [0, 1, 2]
    d = [ray.intersection_slice_for_aabb(eng.Aabb(ov[i, :3], ov[i, 3:]))[0] for i in idx]
    assert d == sorted(d)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_best_first_traversal_matches_iterator_restatement(eng, orc, dtype):
    """CSR in the order of Bvh::nearest_traverse_iterator / farthest_traverse_iterator (DistanceTraverseIterator: the
    std BinaryHeap's sifts decide the order of equal distances) against the oracle's restatement: cube scene (more rays
    than resident lanes: workgroups stride), clustered integer boxes with axis-parallel / in-plane rays (many ties),
    tiny trees, the triangle stage and the closest hit in that order, and a scene whose frontier (1000+ entries)
    outgrows the LDS part of the heap AND the first global workspace (grow + replay)."""
    from bvh_amd import testbase as tb
    rng = np.random.default_rng(37)
    tris32, aabbs32 = tb.create_n_cubes(2000)
    tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
    centres = tris.reshape(2000, 36, 3).mean(axis=1)
    n = 300_000
    o = rng.uniform(-1e5, 1e5, size=(n, 3)).astype(dtype)
    d = (centres[rng.integers(0, 2000, size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3)) - o).astype(dtype)
    d[:2000] = rng.normal(size=(2000, 3))
    rays = orc.make_rays(o, d, dtype)
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    flat.set_triangles(tris)
    onodes = orc.build(aabbs).nodes
    foff, fidx, _, _ = flat.traverse_batch(_rb(eng, rays))
    for order, asc in (("nearest_heap", True), ("farthest_heap", False)):
        off, idx, _, _ = flat.traverse_batch(_rb(eng, rays), order=order)
        ooff, oidx = orc.traverse_distance(onodes, aabbs, rays, asc)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        assert np.array_equal(off, foff) and not np.array_equal(idx, fidx)      # same sets per ray, another order
        off2, idx2, isect, _ = flat.intersect_triangles(_rb(eng, rays), order=order)
        oisect, oclosest, oprim = orc.triangle_stage(tris, rays, ooff, oidx)
        assert np.array_equal(idx2, oidx) and isect.tobytes() == oisect.tobytes()
        cl, prim, _ = flat.closest_hits(_rb(eng, rays), order=order)
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
    m = 5000
    lo = rng.integers(-30, 30, size=(m, 3)).astype(dtype); ext = rng.integers(0, 4, size=(m, 3)).astype(dtype)
    boxes = np.concatenate([lo, lo + ext], axis=1)
    o2 = np.round(rng.uniform(-35, 35, size=(3000, 3))).astype(dtype)
    d2 = rng.integers(-1, 2, size=(3000, 3)).astype(dtype); d2[np.all(d2 == 0, axis=1)] = [0, 0, 1]
    rays2 = orc.make_rays(o2, d2, dtype)
    for k in (m, 3, 2, 1):
        b = eng.Bvh.from_aabbs(boxes[:k]).flatten()
        on = orc.build(boxes[:k]).nodes
        for order, asc in (("nearest_heap", True), ("farthest_heap", False)):
            off, idx, _, _ = b.traverse_batch(_rb(eng, rays2), order=order)
            ooff, oidx = orc.traverse_distance(on, boxes[:k], rays2, asc)
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    # every box contains the origin: all entry distances tie at 0 and the farthest-first frontier passes 1000 entries
    q = 3000
    c = (rng.uniform(-1, 1, size=(q, 3)) * 0.1).astype(dtype)
    hw = rng.uniform(1, 5, size=(q, 1)).astype(dtype)
    nest = np.concatenate([c - hw, c + hw], axis=1).astype(dtype)
    r3 = orc.make_rays(np.zeros((70, 3), dtype), rng.normal(size=(70, 3)).astype(dtype), dtype)
    nb = eng.Bvh.from_aabbs(nest).flatten()
    nn = orc.build(nest).nodes
    for order, asc in (("nearest_heap", True), ("farthest_heap", False)):
        ooff, oidx, peak = orc.traverse_distance(nn, nest, r3, asc, want_peak=True)
        off, idx, _, _ = nb.traverse_batch(_rb(eng, r3), order=order)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        if not asc:
            assert peak > 64
    # the depth that overflows the child iterator's fixed stack is no limit for the heap
    p = 42
    x = 8.0 ** np.arange(p, dtype=np.float64)
    deep = np.stack([x, np.zeros(p), np.zeros(p), x * 1.5, np.ones(p), np.ones(p)], axis=1)
    along = orc.make_rays(np.array([[-1, 0.25, 0.25]], np.float64), np.array([[1, 0, 0]], np.float64), np.float64)
    db = eng.Bvh.from_aabbs(deep).flatten()
    off, idx, _, _ = db.traverse_batch(_rb(eng, along), order="nearest_heap")
    ooff, oidx = orc.traverse_distance(orc.build(deep).nodes, deep, along, True)
    assert np.array_equal(idx, oidx) and len(idx) == p


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refit_moved_shapes(eng, orc, dtype):
    """bvhgpu_refit: the topology stays, every child AABB becomes the exact join of the moved shapes below it
    (fix_aabbs_ascending, optimization.rs:355-391, applied to the whole tree).  Bit-identical to the oracle's bottom-up
    recursion; consistent + tight (the reference's assert_consistent / assert_tight, bvh_impl.rs:424-485); refit with the
    build's own AABBs reproduces the built tree; traversal of the refitted tree == the oracle on the refitted tree and
    returns the same SET per ray as a fresh build of the moved shapes.  Sizes cover 1..3 segment-tree passes."""
    from bvh_amd import testbase as tb
    rng = np.random.default_rng(41)
    for n_cubes in (1, 40, 420, 9000):
        tris32, aabbs32 = tb.create_n_cubes(n_cubes)
        aabbs = aabbs32.astype(dtype)
        for n in sorted({1, 2, 3, len(aabbs)} if n_cubes == 40 else {len(aabbs)}):
            a0 = aabbs[:n].copy()
            bvh = eng.Bvh.from_aabbs(a0)
            ot = orc.build(a0)
            flat = bvh.flatten()
            bvh.refit(a0)                                           # nothing moved: the built tree, bit for bit
            assert bvh.nodes.tobytes() == ot.nodes.tobytes()
            assert flat.nodes.tobytes() == orc.flatten(ot.nodes).tobytes()
            # move every shape (rigidly, by up to a few cube sizes) and give some boxes signed zeros
            shift = rng.uniform(-3, 3, size=(n, 1, 3)).astype(dtype)
            a1 = (a0.reshape(n, 2, 3) + shift).reshape(n, 6)
            a1[::7, 0] = -0.0; a1[::7, 3] = 0.0
            a1[3::11, 1] = 0.0; a1[3::11, 4] = 0.0
            bvh.refit(a1)
            on = orc.refit(ot.nodes, a1)
            assert bvh.nodes.tobytes() == on.tobytes()
            assert orc.check_tree(on, a1) == 0
            oflat = orc.flatten(on)
            assert flat.nodes.tobytes() == oflat.tobytes()
            m = 4000
            o = rng.uniform(-1e5, 1e5, size=(m, 3)).astype(dtype)
            tgt = a1[rng.integers(0, n, m)].reshape(m, 2, 3).mean(axis=1)
            rays = orc.make_rays(o, (tgt - o).astype(dtype), dtype)
            off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
            ooff, oidx, _, _ = orc.traverse_flat(oflat, a1, rays)
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
            fresh = orc.build(a1)
            foff, fidx, _, _ = orc.traverse_flat(orc.flatten(fresh.nodes), a1, rays)
            assert np.array_equal(foff, ooff)
            assert all(sorted(idx[off[i]:off[i + 1]]) == sorted(fidx[foff[i]:foff[i + 1]]) for i in range(m))
            if n >= 2:   # ordered walks read the BvhNode array the refit rewrote
                noff, nidx, _, _ = flat.traverse_batch(_rb(eng, rays), order="nearest_heap")
                qoff, qidx = orc.traverse_distance(on, a1, rays, True)
                assert np.array_equal(noff, qoff) and np.array_equal(nidx, qidx)
            # a rebuild after the refit is an ordinary build again
            bvh.rebuild(a1)
            assert bvh.nodes.tobytes() == fresh.nodes.tobytes()
    # errors: shape count must match, imported scenes have no BvhNode array
    bvh = eng.Bvh.from_aabbs(aabbs[:100])
    with pytest.raises(eng.BvhGpuError):
        bvh.refit(aabbs[:99])


def test_refit_1_2m_triangles_three_passes(eng, orc):
    """1.2 M shapes: n_pad = 2^21, three segment-tree passes; refit == oracle refit, bit for bit."""
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(100_000)
    bvh = eng.Bvh.from_aabbs(aabbs)
    nodes0 = bvh.nodes
    rng = np.random.default_rng(43)
    n = len(aabbs)
    a1 = (aabbs.reshape(n, 2, 3) + rng.uniform(-2, 2, size=(n, 1, 3)).astype(np.float32)).reshape(n, 6)
    bvh.refit(a1)
    assert bvh.nodes.tobytes() == orc.refit(nodes0, a1).tobytes()
    bvh.refit(aabbs)
    assert bvh.nodes.tobytes() == nodes0.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_large_scene_tier_geometry(eng, orc, dtype):
    """above 250 000 shapes the builder hands nodes of up to 1536 (f64: 1024) shapes to 256-thread workgroups instead of
    768 / 384 (build.hip MidSmallScene / MidLargeScene): 300 000 triangles, nodes / flat / CSR byte-identical to the oracle."""
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(25_000)
    aabbs = aabbs.astype(dtype)
    bvh = eng.Bvh.from_aabbs(aabbs)
    ot = orc.build(aabbs, threads=min(8, orc.max_threads()))
    assert bvh.nodes.tobytes() == ot.nodes.tobytes()
    assert np.array_equal(bvh.shape_nodes, ot.shape_node)
    flat = bvh.flatten()
    oflat = orc.flatten(ot.nodes)
    assert flat.nodes.tobytes() == oflat.tobytes()
    rays = orc.create_rays(0, 50_000)
    if dtype == np.float64:
        rays = orc.make_rays(rays["o"], rays["d"], np.float64)
    off, idx, _, _ = flat.traverse_batch(_rb(eng, rays))
    ooff, oidx, _, _ = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)


@pytest.mark.parametrize("launches", [0, 1])
def test_parity_1_2m_triangles(eng, orc, launches):
    """ten times the BASELINE scene (create_n_cubes(100 000) = 1.2 M triangles): more level-synchronous passes,
    many tier-A/B items, multi-chunk tile-offset scans — node, flat and CSR arrays byte-identical to the oracle; with the level
    tier's schedule the library picks at this size (two launches per level) and with one launch per level forced (more tiles
    than workgroups, items of more than 384 tiles)."""
    from bvh_amd import Context, testbase as tb
    from bvh_amd._lib import TUNE_BUILD_LEVEL_LAUNCHES
    _, aabbs = tb.create_n_cubes(100_000)
    rays = orc.create_rays(0, 100_000)
    ctx = Context(0)
    ctx.set_tuning(TUNE_BUILD_LEVEL_LAUNCHES, launches)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    ot = orc.build(aabbs, threads=min(8, orc.max_threads()))
    assert bvh.nodes.tobytes() == ot.nodes.tobytes()
    assert np.array_equal(bvh.shape_nodes, ot.shape_node)
    flat = bvh.flatten()
    oflat = orc.flatten(ot.nodes)
    assert flat.nodes.tobytes() == oflat.tobytes()
    off, idx, _, st = flat.traverse_batch(_rb(eng, rays), stats=True)
    ooff, oidx, _, ost = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and st["visited"] == ost["visited"]


def test_c_abi_from_plain_c(eng, orc, tmp_path):
    """tests/c_abi/abi_roundtrip.c — a C11 program that only includes include/bvh_mi355x.h and links
    libbvh_mi355x.so: FlatBvh::build, Ray::new, traverse, nearest_to; its printout must match the oracle."""
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "abi_roundtrip")
    libdir = os.path.join(root, "bvh_amd")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c_abi", "abi_roundtrip.c"), "-L", libdir, "-lbvh_mi355x",
                           "-Wl,-rpath," + libdir, "-o", exe])
    env = dict(os.environ)
    # the engine must bind to the same HIP runtime the wheel ships (see bvh_amd/_lib.py); for a C program that is
    # whatever libamdhip64.so.7 the loader finds first: point it at torch's copy, like the Python path does
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    banner = ("RCCL version", "HIP version", "ROCm version", "Hostname", "Librccl path")
    out = [ln for ln in subprocess.check_output([exe, "5"], env=env, text=True).strip().splitlines() if not ln.startswith(banner)]
    m = 5
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) * 2
    aabbs = np.concatenate([g + np.float32(-0.5), g + np.float32(0.5)], axis=1)
    ot = orc.build(aabbs)
    oflat = orc.flatten(ot.nodes)
    rays = orc.make_rays(np.array([[-5, 0, 0], [-3, -3, -3]], np.float32), np.array([[1, 0, 0], [1, 1, 1]], np.float32))
    ooff, oidx, _, ost = orc.traverse_flat(oflat, aabbs, rays)
    assert out[0] == f"shapes {m ** 3} nodes {2 * m ** 3 - 1} flat {3 * m ** 3 - 2} dtype 0"
    assert out[1] == f"total {len(oidx)} visited {ost['visited']}"
    for r in range(2):
        want = " ".join(str(int(i)) for i in oidx[ooff[r]:ooff[r + 1]])
        assert out[2 + r] == (f"ray {r}: {want}" if want else f"ray {r}:")
    s, d = orc.nearest(oflat, aabbs, [[2.2, 0.1, 3.9]])
    assert out[4] == f"nearest {int(s[0])} {d[0]:.6f}"
    # the RCCL exchange step through the C ABI (one-rank communicator on this one-GPU box): the tree survives a broadcast
    comm_line = [ln for ln in out if ln.startswith("comm ranks")]   # (RCCL prints its own version banner to stdout)
    ndev = eng.device_count()
    assert comm_line == [f"comm ranks {ndev} first 0 local {ndev}; after bcast total {len(oidx)}"]

    # the sharded step (one ctx per device over real RCCL; then K = 4 ranks sharing device 0 over the tests' stand-in library):
    # rebuild_flat_async on the root, bcast_known, every rank walks its slice of ONE ray stream — concatenation == oracle
    def shard_line(lines):
        return [ln for ln in lines if ln.startswith("shards ")][0].split()

    T = 60000
    bounds = np.array([-3, -3, -3, 2 * m + 1, 2 * m + 1, 2 * m + 1], np.float32)
    soff, sidx, _, _ = orc.traverse_flat(oflat, aabbs, orc.create_rays(0, T, bounds), threads=orc.max_threads())
    csum = 0
    for r in range(T):
        for j in range(int(soff[r]), int(soff[r + 1])):
            csum = (csum * 1000003 + r * 31 + int(sidx[j])) % (1 << 64)

    def check_shards(lines, K):
        f = shard_line(lines)
        assert f[1] == str(K) and f[3] == str(T) and f[5] == str(len(sidx)) and f[7] == str(csum), f
        per = [int(x) for x in f[9:]]
        cuts = [int(soff[(i * T) // K]) for i in range(K + 1)]
        assert per == [cuts[i + 1] - cuts[i] for i in range(K)]

    check_shards(out, ndev)
    fake = os.path.join(root, "tests", "c_abi", "libfakerccl.so")
    src = os.path.join(root, "tests", "c_abi", "fake_rccl.cpp")
    if not os.path.exists(fake) or os.path.getmtime(fake) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "-O1", "-o", fake, src])
    env4 = dict(env, BVHGPU_RCCL_LIB=fake, BVHGPU_RCCL_SHARED_DEVICE="1")
    out4 = subprocess.check_output([exe, "5", "4"], env=env4, text=True).strip().splitlines()
    check_shards(out4, 4)


def _unreached_combos():
    """fuzz_scenes.OTHER_COMBOS on seeds 100..107; from BVH_FUZZ_SEEDS = 32 on all 24 combinations outside the historic map, on seeds 100..123"""
    import fuzz_scenes as fs
    combos = fs.OTHER_COMBOS
    if int(os.environ.get("BVH_FUZZ_SEEDS", "12")) >= 32:
        reached = {(d, k, fs.k_scales(d).index(s)) for d, k, s in map(fs.historic, range(8))}
        rest = [(d, k, si) for d in (np.float32, np.float64) for k in range(4) for si in range(4) if (d, k, si) not in reached and (d, k, si) not in fs.OTHER_COMBOS]
        combos = fs.OTHER_COMBOS + rest
    return [pytest.param(100 + j, d, k, si, id=f"{100 + j}-{'f32' if d == np.float32 else 'f64'}-{fs.KINDS[k]}-{fs.SCALES[si]}") for j, (d, k, si) in enumerate(combos)]


@pytest.mark.parametrize("seed", range(int(os.environ.get("BVH_FUZZ_SEEDS", "12"))))   # BVH_FUZZ_SEEDS=400 for a long soak
def test_fuzz_all_queries(eng, orc, seed):
    """in the spirit of the reference's fuzz.rs ("all traversals agree", fuzz.rs:321-324): random scenes of random
    size and character (spread, clustered, grid-aligned with exact ties, duplicated shapes), random rays and points;
    every query the engine offered when this test was written against the oracle (tests/test_gpu_fuzz_queries.py has the later
    families).  Each seed scales its scene by 2^k — 1, an all-subnormal band, a band where surface areas overflow, 2^-20 — and a tenth of
    its rays are caller-built (inv = ±0, subnormal, huge, or not 1/d).  dtype, kind and scale follow from seed % 8 (fuzz_scenes.historic):
    8 of the 32 combinations, however many seeds run; test_fuzz_all_queries_other_combos runs the same body on the others."""
    import fuzz_scenes as fs
    _fuzz_all_queries(eng, orc, seed, *fs.historic(seed))


@pytest.mark.parametrize("seed,dtype,kind,scale_index", _unreached_combos())
def test_fuzz_all_queries_other_combos(eng, orc, seed, dtype, kind, scale_index):
    """test_fuzz_all_queries' body on combinations its map never reaches: grid-aligned scenes (the only ones with exact distance ties) in
    f64 and at scale 1, duplicated shapes in f32, spread and clustered scenes in the subnormal band of the other dtype"""
    import fuzz_scenes as fs
    _fuzz_all_queries(eng, orc, seed, dtype, kind, fs.k_scales(dtype)[scale_index])


def _fuzz_all_queries(eng, orc, seed, dtype, kind, k_scale):
    """the scene of fuzz_scenes.draw(seed, dtype, kind, k_scale); the seed also rotates the tuning knobs"""
    import fuzz_scenes as fs
    import query_ref as qr
    from test_gpu_any_hit import first_match
    scene = fs.draw(seed, dtype, kind, k_scale)
    sc, tri, aabbs, rays = (scene[name] for name in ("sc", "tri", "aabbs", "rays"))
    bvh = eng.Bvh.from_aabbs(aabbs)
    ot = orc.build(aabbs)
    assert bvh.nodes.tobytes() == ot.nodes.tobytes() and np.array_equal(bvh.shape_nodes, ot.shape_node)
    flat = bvh.flatten()
    oflat = orc.flatten(ot.nodes)
    assert flat.nodes.tobytes() == oflat.tobytes()
    flat.set_triangles(tri)
    rb = _rb(eng, rays)
    ooff, oidx, ots, ost = orc.traverse_flat(oflat, aabbs, rays, want_t=True)
    off, idx, ts, st = flat.traverse_batch(rb, want_t=True, stats=True)
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    if len(idx):
        assert same_bytes(ts, ots)
    # a split without SAH winner (the band where surface areas overflow) leaves empty child boxes, which every ray enters:
    # Bvh::traverse then reports the shapes below them unfiltered while FlatBvh::traverse tests each shape's own AABB, and
    # the visit counters stop being comparable (see _variant_suite's overflow scene)
    if not np.any((oflat["entry"] != 0xFFFFFFFF) & (oflat["min"][:, 0] > oflat["max"][:, 0])):
        assert st["visited"] == ost["visited"]
        toff, tidx = orc.traverse_tree(ot.nodes, aabbs, rays)           # Bvh::traverse == FlatBvh::traverse
        assert np.array_equal(toff, ooff) and np.array_equal(tidx, oidx)
    # the large-batch walk (four grandchildren per step, rays cut into items) on the same small batch, and the two level-tier
    # schedules of the builder alternating with the seed
    from bvh_amd import Context
    from bvh_amd._lib import TUNE_BUILD_LEVEL_LAUNCHES, TUNE_BUILD_LEVEL_TILE, TUNE_FLATTEN_INLINE, TUNE_TRAVERSE_LDS_MIN_RAYS, TUNE_WIDE_ITEMS_LOG4
    wctx = Context(0)
    wctx.set_tuning(TUNE_FLATTEN_INLINE, seed % 2)   # the wave tier flattens its own subtrees / the flatten kernel writes everything
    wctx.set_tuning(TUNE_BUILD_LEVEL_TILE, (0, 1024, 2048)[seed % 3])
    wctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    wctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, (seed // 2) % 3)
    wctx.set_tuning(TUNE_BUILD_LEVEL_LAUNCHES, 1 + seed % 2)
    wb = eng.Bvh.from_aabbs(aabbs, wctx)
    assert wb.nodes.tobytes() == ot.nodes.tobytes()
    wflat = wb.flatten()
    woff, widx, _, _ = wflat.traverse_batch(eng.RayBatch(len(rays), dtype, host=np.ascontiguousarray(rays)))
    assert np.array_equal(woff, ooff) and np.array_equal(widx, oidx)
    if (seed // 2) % 3 == 0:   # whole rays: also the staged hand-over of COHERENT batches (per-ray slots, the slot copy through LDS, pair records)
        woff, widx, _, _ = wflat.traverse_batch(eng.RayBatch(len(rays), dtype, host=np.ascontiguousarray(rays)), coherent=True)
        assert np.array_equal(woff, ooff) and np.array_equal(widx, oidx)
    oisect, oclosest, oprim = orc.triangle_stage(tri, rays, ooff, oidx)
    _, _, isect, _ = flat.intersect_triangles(rb)
    cl, prim, _ = flat.closest_hits(rb)
    assert same_bytes(isect, oisect) and same_bytes(cl, oclosest) and np.array_equal(prim, oprim)
    if orc.tree_stats(ot.nodes, aabbs)["max_depth"] < 31:
        for order, asc in (("nearest", True), ("farthest", False)):
            noff, nidx, _, _ = flat.traverse_batch(rb, order=order)
            qoff, qidx = orc.traverse_child_ordered(ot.nodes, aabbs, rays, asc)
            assert np.array_equal(noff, qoff) and np.array_equal(nidx, qidx)
    for order, asc in (("nearest_heap", True), ("farthest_heap", False)):
        noff, nidx, _, _ = flat.traverse_batch(rb, order=order)
        qoff, qidx = orc.traverse_distance(ot.nodes, aabbs, rays, asc)
        assert np.array_equal(noff, qoff) and np.array_equal(nidx, qidx)
    pts = scene["pts"]
    for use_tris in (False, True):
        s_, d_ = flat.nearest_batch(pts, triangles=use_tris)
        os_, od_ = orc.nearest(oflat, aabbs, pts, tri if use_tris else None)
        assert np.array_equal(s_, os_) and same_bytes(d_, od_)
    # any hit with segment ends drawn around the nearest hit
    c = oclosest[:, 0].astype(np.float64)
    tmax = (np.where(np.isfinite(c), c, 200.0 * sc) * scene["tmax_u"]).astype(dtype)
    want = first_match(ooff, oidx, oisect, tmax)
    isect_a, shape_a = flat.any_hits(rb, tmax)
    assert same_bytes(isect_a, want[0]) and np.array_equal(shape_a, want[1])
    # AABB / point / ball queries around random shapes, the walks of knob 22 alternating with the seed
    cq, e = scene["cq"], scene["e"]
    for qkind, q64 in ((qr.AABB, np.concatenate([cq - e, cq + e], axis=1)), (qr.POINT, cq), (qr.BALL, np.concatenate([cq, e[:, :1]], axis=1))):
        q = (q64 * sc).astype(dtype)
        qoff, qidx = qr.walk(oflat, aabbs, qkind, q)
        wctx.set_tuning(22, (seed // 8) % 2)
        goff, gidx = wflat.query_batch(qkind, q)
        assert goff.tobytes() == qoff.tobytes() and gidx.tobytes() == qidx.tobytes(), qkind


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coherent", [False, True])
def test_pair_records_every_hit_count(eng, orc, dtype, coherent):
    """Whole-ray index batches hand their hits over as PAIR records (walk.hpp report_pair: two consecutive hits of a ray per 16-byte
    record, the last one alone when the count is odd; behind the first 8 per-ray slot entries when the batch is COHERENT).  Rays with
    exactly 0, 1, 2, ... 90 hits, interleaved so that one wave holds odd and even counts, retiring rays and fresh ones at once; a small
    batch first, so that the large one finds the pool too small (grow + replay), then the large one again on the grown pool."""
    from bvh_amd import Context
    from bvh_amd._lib import TUNE_TRAVERSE_LDS_MIN_RAYS, TUNE_WIDE_ITEMS_LOG4, WALK_REC8, WALK_WIDE
    ctx = Context(0)
    ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    ctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, 0)
    m = 90
    x = np.arange(m, dtype=dtype) * dtype(2.0)
    lo = np.stack([x, np.zeros(m, dtype), np.zeros(m, dtype)], axis=1)
    aabbs = np.concatenate([lo, lo + dtype(1.0)], axis=1)               # unit boxes at x = 0, 2, 4, ...: a +x ray from the gap before box j hits m - j of them
    rng = np.random.default_rng(5)
    starts = rng.integers(0, m + 1, size=20_000)                         # (m: behind the last box — no hit)
    starts[:m + 1] = np.arange(m + 1)
    o = np.stack([2.0 * starts - 0.5, np.full(len(starts), 0.5), np.full(len(starts), 0.5)], axis=1).astype(dtype)
    d = np.tile(np.array([1, 0, 0], dtype), (len(starts), 1))
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    ooff, oidx, _, _ = orc.traverse_flat(oflat, aabbs, rays)
    assert np.array_equal(np.diff(ooff.astype(np.int64)), m - starts)
    tree = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    few = eng.RayBatch(m + 1, dtype, host=np.ascontiguousarray(rays[:m + 1]))   # 91 rays first: the pool is sized for them ...
    off, idx, _, _ = tree.traverse_batch(few, coherent=coherent)
    assert np.array_equal(off, ooff[:m + 2]) and np.array_equal(idx, oidx[:ooff[m + 1]])
    rb = eng.RayBatch(len(rays), dtype, host=np.ascontiguousarray(rays))
    for _ in range(2):                                                           # ... and must grow for 20 000 (replay), then is reused
        off, idx, _, st = tree.traverse_batch(rb, coherent=coherent)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        assert st["walk"] & WALK_WIDE and st["walk"] & WALK_REC8
