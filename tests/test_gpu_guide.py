"""f64 index batches walked over the tree's f32 guide boxes (walk_wide.hip "guide walk", BVHGPU_TUNE_WIDE_F64_GUIDE): the lists are the
oracle's — on random rays, on rays that graze faces / edges / corners of the shapes' boxes (where a conservative inner test and the
f64 leaf test must agree exactly), with whole rays and with rays cut into items, after a refit, on an imported scene — and a batch with
a ray outside the guide walk's range is replayed with the f64 walk without the caller noticing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _csr(eng, flat, rays, **kw):
    off, idx, _, st = flat.traverse_batch(eng.RayBatch(len(rays), np.float64, host=np.ascontiguousarray(rays)), **kw)
    return off, idx, st


def _oracle(orc, aabbs, rays):
    oflat = orc.flatten(orc.build(aabbs).nodes)
    ooff, oidx, _, _ = orc.traverse_flat(oflat, aabbs, rays, threads=orc.max_threads())
    return ooff, oidx


def _cubes64(n):
    from bvh_amd import testbase as tb
    _, aabbs = tb.create_n_cubes(n)
    return aabbs.astype(np.float64)


def _grazing_rays(orc, aabbs, n, seed):
    """rays from inside the scene's bounds aimed at points ON the surface of random shapes' boxes (corners, edges, faces)"""
    rng = np.random.default_rng(seed)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    b = aabbs[rng.integers(0, len(aabbs), n)]
    pick = rng.integers(0, 3, (n, 3))                                   # per axis: min plane, max plane, somewhere between
    u = rng.uniform(0, 1, (n, 3))
    tgt = np.where(pick == 0, b[:, :3], np.where(pick == 1, b[:, 3:], b[:, :3] + u * (b[:, 3:] - b[:, :3])))
    o = rng.uniform(lo, hi, (n, 3))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return orc.make_rays(o, d, np.float64)


@pytest.mark.parametrize("items", [-1, 0, 2])
def test_guide_walk_lists_are_the_oracles(eng, orc, items):
    from bvh_amd._lib import TUNE_WIDE_F64_GUIDE, TUNE_WIDE_ITEMS_LOG4, WALK_F64_GUIDE, WALK_WIDE
    aabbs = _cubes64(3000)
    ctx = eng.Context(0)
    ctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, items)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    rays = np.concatenate([orc.create_rays(0, 60_000, dtype=np.float64), _grazing_rays(orc, aabbs, 60_000, 3)])
    ooff, oidx = _oracle(orc, aabbs, rays)
    off, idx, st = _csr(eng, flat, rays)
    assert st["walk"] & WALK_WIDE and st["walk"] & WALK_F64_GUIDE          # the guide walk ran (no ray was out of range)
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    ctx.set_tuning(TUNE_WIDE_F64_GUIDE, 0)
    off2, idx2, st2 = _csr(eng, flat, rays)
    assert st2["walk"] & WALK_WIDE and not st2["walk"] & WALK_F64_GUIDE    # the f64 walk
    assert np.array_equal(off2, ooff) and np.array_equal(idx2, oidx)


def test_guide_walk_hit_heavy_scene_whole_rays_and_staged(eng, orc):
    from bvh_amd import scene
    from bvh_amd._lib import WALK_F64_GUIDE
    _, a32, bounds = scene.parse_obj(scene.make_atrium_obj(4))
    aabbs = a32.astype(np.float64)
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    r32 = orc.create_rays(5_000_000, 120_000, bounds=bounds)
    rays = np.concatenate([orc.make_rays(r32["o"].astype(np.float64), r32["d"].astype(np.float64), np.float64), _grazing_rays(orc, aabbs, 40_000, 9)])
    ooff, oidx = _oracle(orc, aabbs, rays)
    assert len(oidx) > 4 * len(rays)                                        # hit-heavy: most steps report a leaf candidate
    for coherent in (False, True):
        off, idx, st = _csr(eng, flat, rays, coherent=coherent)
        assert st["walk"] & WALK_F64_GUIDE
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)


def test_ray_outside_the_guide_range_replays_in_f64(eng, orc):
    from bvh_amd._lib import WALK_F64_GUIDE, WALK_WIDE
    aabbs = _cubes64(2000)
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    good = orc.create_rays(77, 40_000, dtype=np.float64)
    S = np.abs(aabbs).max()
    far = orc.make_rays(np.array([[20 * S, 0.3, 0.1]]), np.array([[-1.0, 0.001, 0.002]]), np.float64)        # origin beyond 3 x the scene
    axis = orc.make_rays(np.array([[-S, 1.0, 2.0]]), np.array([[1.0, 0.0, 0.0]]), np.float64)               # 1/d = inf on two axes
    for odd in (far, axis):
        rays = np.concatenate([good[:20_000], odd, good[20_000:]])
        ooff, oidx = _oracle(orc, aabbs, rays)
        off, idx, st = _csr(eng, flat, rays)
        assert st["walk"] & WALK_WIDE and not st["walk"] & WALK_F64_GUIDE   # replayed with the f64 walk
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    # the result object backs off — 1, 2, 4 … batches in f64 after consecutive out-of-range batches — and then tries its guide again
    # (round 4: the fall-back used to be for ever)
    ooff, oidx = _oracle(orc, aabbs, good)

    def guided(r):
        off, idx, st = _csr(eng, flat, r)
        if r is good:
            assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
        return bool(st["walk"] & WALK_F64_GUIDE)
    # (above: `far` failed → one batch of back-off, which the `axis` batch used up in f64) → the guide is back
    assert guided(good) and guided(good)
    bad = np.concatenate([good[:100], axis, good[100:]])
    assert not guided(bad)                                 # out of range: replayed in f64, back-off one batch
    assert [guided(good), guided(good)] == [False, True]
    assert not guided(bad) and not guided(good)            # fails (1 batch of back-off, used up by the good batch) …
    assert not guided(bad)                                 # … the guide is tried, fails again: second failure in a row → two batches
    assert [guided(good), guided(good), guided(good)] == [False, False, True]
    flat2 = eng.Bvh.from_aabbs(aabbs).flatten()
    ooff, oidx = _oracle(orc, aabbs, good)
    off, idx, st = _csr(eng, flat2, good)
    assert st["walk"] & WALK_F64_GUIDE and np.array_equal(off, ooff) and np.array_equal(idx, oidx)


def test_guide_boxes_follow_refit_and_scene_import(eng, orc):
    from bvh_amd import FlatBvh
    from bvh_amd._lib import WALK_F64_GUIDE
    aabbs = _cubes64(1500)
    bvh = eng.Bvh.from_aabbs(aabbs)
    flat = bvh.flatten()
    rays = np.concatenate([orc.create_rays(5, 30_000, dtype=np.float64), _grazing_rays(orc, aabbs, 30_000, 21)])
    ooff, oidx = _oracle(orc, aabbs, rays)
    off, idx, st = _csr(eng, flat, rays)
    assert st["walk"] & WALK_F64_GUIDE and np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    # an imported scene makes its wide nodes (and with them the guide boxes) from the traversal array alone (flatten.hip k_wide)
    blob = np.zeros(flat.scene_nbytes(), np.uint8)
    flat.scene_export(blob)
    imp = FlatBvh.scene_import(blob, len(blob))
    off, idx, st = _csr(eng, imp, rays)
    assert st["walk"] & WALK_F64_GUIDE and np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    # the shapes move (same topology): the refit re-flattens, the guide boxes follow; the oracle refits the same tree
    rng = np.random.default_rng(2)
    moved = aabbs + np.tile(rng.uniform(-0.4, 0.4, (len(aabbs), 3)), 2)
    bvh.refit(moved)                                                          # (flat is the same tree: it is re-flattened)
    rays2 = np.concatenate([rays[:30_000], _grazing_rays(orc, moved, 30_000, 22)])
    ot = orc.build(aabbs)
    oflat = orc.flatten(orc.refit(ot.nodes, moved))
    off, idx, st = _csr(eng, flat, rays2)
    assert st["walk"] & WALK_F64_GUIDE
    from bvh_amd._lib import TUNE_WIDE_F64_GUIDE
    flat.ctx.set_tuning(TUNE_WIDE_F64_GUIDE, 0)                              # the f64 walk over the same refitted tree is the reference here
    off2, idx2, st2 = _csr(eng, flat, rays2)
    flat.ctx.set_tuning(TUNE_WIDE_F64_GUIDE, 1)
    assert not st2["walk"] & WALK_F64_GUIDE and np.array_equal(off, off2) and np.array_equal(idx, idx2)
    ooff2, oidx2, _, _ = orc.traverse_flat(oflat, moved, rays2, threads=orc.max_threads())
    assert np.array_equal(off, ooff2) and np.array_equal(idx, oidx2)


@pytest.mark.parametrize("log2_s,log2_inv,guide", [(-124, 30, True), (-101, 0, True), (0, 0, True), (90, -40, True), (124, -90, True),
                                                   (-130, 40, False), (126, -90, False), (-60, 130, False), (100, -140, False)])
def test_guide_walk_at_the_edges_of_its_range(eng, orc, log2_s, log2_inv, guide):
    """VERDICT r3 #6 / ADVICE r3: scenes scaled to the smallest and largest S the containment argument covers (2^-125 .. 2^125, f32 denormal
    coordinates below that), raw rays whose 1/d is scaled so that 4 S |1/d| sits inside 2^+-100 — the guide walk runs and its lists are
    the f64 oracle's; one step outside (S too small / too large, (float)(1/d) = inf or denormal) and the batch is replayed in f64."""
    from bvh_amd._lib import RAY_F64, WALK_F64_GUIDE, WALK_WIDE
    unit = _cubes64(800)
    unit = unit / np.abs(unit).max()                                         # largest |coordinate| = 1
    S = 2.0 ** log2_s
    aabbs = unit * S
    assert np.all(np.isfinite(aabbs)) and np.abs(aabbs).max() == S
    g = _grazing_rays(orc, unit, 30_000, 500 + log2_s)
    rays = np.zeros(len(g), RAY_F64)
    rays["o"] = g["o"] * S                                                   # (exact: a power of two)
    rays["d"] = g["d"]
    rays["inv"] = g["inv"] * 2.0 ** log2_inv                                 # an unnormalised direction: every t scales alike, the hit set is the same
    flat = eng.Bvh.from_aabbs(aabbs).flatten()
    ooff, oidx = _oracle(orc, aabbs, rays)
    assert len(oidx) > len(rays) // 2                                        # grazing rays: the corner cases are hits
    off, idx, st = _csr(eng, flat, rays)
    assert st["walk"] & WALK_WIDE and bool(st["walk"] & WALK_F64_GUIDE) == guide
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)


@pytest.mark.parametrize("items", [-1, 0])
def test_guide_walk_closest_hit_is_the_oracles(eng, orc, items):
    """round 6: closest-hit batches of an f64 tree through the guide walk — inner tests in f32 on the grown boxes, every leaf candidate's box AND
    triangle (Ray::intersects_triangle, ray_impl.rs:154-213) decided in f64, the nearest one kept with the reference's strict < (testbase.rs:831-833):
    (distance, u, v, shape) of every ray byte-equal to the oracle's loop, rays cut into items and whole, and a batch with a ray outside the
    guide's range replayed in f64 without the caller noticing."""
    from bvh_amd import testbase as tb
    from bvh_amd._lib import TUNE_WIDE_ITEMS_LOG4
    tris32, a32 = tb.create_n_cubes(2500)
    tris, aabbs = tris32.astype(np.float64), a32.astype(np.float64)
    ctx = eng.Context(0)
    ctx.set_tuning(TUNE_WIDE_ITEMS_LOG4, items)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    rng = np.random.default_rng(11)
    n = 50_000
    centres = tris.reshape(2500, 36, 3).mean(axis=1)
    target = centres[rng.integers(0, 2500, size=n)] + rng.uniform(-0.6, 0.6, size=(n, 3))
    o = rng.uniform(-1e5, 1e5, size=(n, 3))
    rays = np.concatenate([orc.make_rays(o, target - o, np.float64), _grazing_rays(orc, aabbs, 30_000, 5), orc.create_rays(0, 20_000, dtype=np.float64)])
    oflat = orc.flatten(orc.build(aabbs).nodes)

    def check(r):
        ooff, oidx, _, _ = orc.traverse_flat(oflat, aabbs, r, threads=orc.max_threads())
        _, oclosest, oprim = orc.triangle_stage(tris, r, ooff, oidx)
        cl, prim, _ = flat.closest_hits(eng.RayBatch(len(r), np.float64, host=np.ascontiguousarray(r)))
        assert cl.tobytes() == oclosest.tobytes() and np.array_equal(prim, oprim)
        return np.isfinite(oclosest[:, 0]).sum()
    assert check(rays) > n // 2
    assert flat._hits.walk_kernel() == "bvhgpu::k_traverse_wide<float, 3, %d, 1024, 8, 1>" % (2 if items < 0 else 0)
    S = np.abs(aabbs).max()
    axis = orc.make_rays(np.array([[-S, 1.0, 2.0]]), np.array([[1.0, 0.0, 0.0]]), np.float64)               # 1/d = inf on two axes: outside the guide's range
    check(np.concatenate([rays[:30_000], axis, rays[30_000:60_000]]))
    assert flat._hits.walk_kernel().startswith("bvhgpu::k_traverse_wide<double, 3, ")                       # replayed with the f64 walk
