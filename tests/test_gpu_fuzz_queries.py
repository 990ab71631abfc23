"""Fuzz over the query families added after tests/test_gpu_parity.py::test_fuzz_all_queries: knearest_batch, knearest_tree_batch (with
max_dist), the box-hit and sphere-hit queries, khits_batch and allhits_batch, on the random scenes of tests/fuzz_scenes.py — every shape
count from 1 to 60 000, four scene characters, four scale bands, caller-built rays, both dtypes; fuzz_scenes.combo reaches all 32
(dtype, kind, scale) combinations, 16 of them by default.  One build per seed; every leg against its reference byte for byte (two NaNs
count as equal).  tests/test_fuzz_queries_cpu.py shows on the references alone what the default seeds contain: ties, rows beyond every tier
of allhits.hip, rows that k cuts, segment ends and limits pinned on a candidate's own distance, odd spheres, padding rows.

The Python references set the sizes.  The k-nearest references compute every shape's distance per point, so fuzz_scenes.extras draws
fewer points the more shapes a scene has; the ray references sort the scene's whole CSR per call, so on a scene whose CSR holds more than
BIG_CSR members the (k, tmax) crossing of khits_batch and the (order, tmax) crossing of allhits_batch are thinned — every k, every order
and both limits still run, in pairings that rotate with the seed — and no family is dropped."""
import os
import time

import numpy as np
import pytest

import allhits_ref as ar
import fuzz_scenes as fs
import khits_ref as khr
from sphere_ref import sphere_match
from test_box_hit_cpu import box_match
from test_fp_extremes_cpu import same as same_bytes  # byte equality, two NaNs equal
from test_gpu_allhits import _dev_rays, _to_host
from test_gpu_any_hit import _rb
from test_gpu_box_hit import WALKS

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FORCED_WALKS = WALKS[:4]     # binary, LDS, wide over whole rays, wide over items: forced by tuning (the fifth entry, the default tuning, is the
                             # binary walk again at these batch sizes)
BINARY_WALKS = [w for w in FORCED_WALKS if "wide" not in w[1]]
BIG_CSR = 200_000            # members


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


def _walk_for(seed, shift, wide_eligible):
    """(tuning, kernel-name prefix) of the seed's walk: FORCED_WALKS in rotation; on a tree with empty child bounds, which the wide walk
    does not take, the binary ones in rotation"""
    walks = FORCED_WALKS if wide_eligible else BINARY_WALKS
    return walks[(seed + shift) % len(walks)]


def _repetitions(seed, ks, big):
    """(khits: [(k, limit name)], allhits: [(sort, limit name)]) per leaf: the full crossings, or on a big CSR every k without tmax and one
    k with it, the sorted rows without tmax (the long ones), list order with it, and one more pairing — k and pairing rotate with the seed"""
    if not big:
        return [(k, lim) for k in ks for lim in ("none", "tmax")], [(sort, lim) for lim in ("none", "tmax") for sort in (True, False)]
    return [(k, "none") for k in ks] + [(ks[seed % 3], "tmax")], [(True, "none"), (False, "tmax"), ((True, "tmax"), (False, "none"))[seed % 2]]


class _tuned:
    """the context's tuning set for one leg, and put back"""

    def __init__(self, ctx, tune):
        self.ctx, self.tune = ctx, tune

    def __enter__(self):
        self.saved = {k: self.ctx.get_tuning(k) for k in self.tune}
        for k, v in self.tune.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_tuning(k, v)


def _same_rows(got, want, label):
    """(shape[n, k], dist[n, k]) of the k-nearest families"""
    assert np.array_equal(got[0], want[0]), (label, "shapes, first rows", np.nonzero((got[0] != want[0]).any(axis=1))[0][:5])
    assert same_bytes(got[1], want[1]), (label, "distances")


def _same_hit(got, want, label):
    """(record[n, 2], shape[n]) of the box and sphere queries"""
    assert np.array_equal(got[1], want[1]), (label, "shapes, first rays", np.nonzero(got[1] != want[1])[0][:5])
    assert same_bytes(got[0], want[0]), (label, "records")


def _same_khits(got, want, label):
    """(vals[n, k, W], shape[n, k])"""
    assert np.array_equal(got[1], want[1]), (label, "shapes, first rays", np.nonzero((got[1] != want[1]).any(axis=1))[0][:5])
    assert same_bytes(got[0], want[0]), (label, "records")


def _same_csr(got, want, label):
    """(offsets[n + 1], shape[total], vals[total, W])"""
    assert np.array_equal(got[0], want[0]), (label, "offsets, first rays", np.nonzero(got[0] != want[0])[0][:5])
    bad = np.nonzero(got[1] != want[1])[0][:5]
    assert len(bad) == 0, (label, "shapes differ at", bad, "rays", np.searchsorted(want[0], bad, side="right") - 1)
    assert same_bytes(got[2], want[2]), (label, "records")


@pytest.mark.parametrize("seed", range(int(os.environ.get("BVH_FUZZ_SEEDS", fs.DEFAULT_SEEDS))))   # BVH_FUZZ_SEEDS=64 for a soak over every combination twice
def test_fuzz_later_query_families(eng, seed):
    import torch
    t0 = time.perf_counter()
    c = fs.case(seed)
    knn = fs.knn_rows(seed)
    t1 = time.perf_counter()
    scene, ex = c["scene"], c["extras"]
    dtype, tri, aabbs, rays = scene["dtype"], scene["tri"], scene["aabbs"], scene["rays"]
    off, idx, records, ks, kpts = c["off"], c["idx"], c["records"], ex["ks"], ex["kpts"]
    name = fs.label(seed)

    # one build, one flatten — and first of all the tree itself: a wrong tree must not show up as six query failures
    ctx = eng.Context(0)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    assert bvh.nodes.tobytes() == c["nodes"].tobytes() and np.array_equal(bvh.shape_nodes, c["shape_node"]), name
    flat = bvh.flatten()
    assert flat.nodes.tobytes() == c["oflat"].tobytes(), name
    flat.set_triangles(tri)
    flat.set_spheres(ex["spheres"])
    rb = _rb(eng, rays)

    # k nearest, flat walk and tree descent: shape distance = the box / the triangle; the descent without and with the drawn limits
    for kind in (0, 1):
        for k in ks:
            _same_rows(flat.knearest_batch(kpts, k, triangles=bool(kind)), knn["flat"][kind][k], (name, "knearest", kind, k))
            for lim, max_dist in (("none", None), ("limit", ex["max_dist"][kind])):
                got = flat.knearest_tree_batch(kpts, k, triangles=bool(kind), max_dist=max_dist)
                _same_rows(got, knn["tree"][kind][lim][k], (name, "knearest_tree", kind, k, lim))

    # box hits and sphere hits, each under one walk of the rotation — and under that walk's kernel, not another one
    limited = {leaf: dict(none=None, tmax=ex["tmax"][leaf]) for leaf in fs.LEAVES}
    tname = "float" if dtype == np.float32 else "double"

    def took(kernel, mode, what):
        if scene["n"] >= 2:   # (a tree of one shape has no walk to choose)
            assert flat.query_kernel().startswith(kernel.format(t=tname, m=mode)), (name, what, flat.query_kernel())

    tune, box_kernel = _walk_for(seed, 0, c["wide_eligible"])
    with _tuned(ctx, tune):
        for lim, tmax in limited["box"].items():
            want = {first: box_match(off, idx, records["box"], tmax, first) for first in (False, True)}
            _same_hit(flat.closest_box_hits(rb, tmax), want[False], (name, "closest_box_hits", lim))
            took(box_kernel, 5, "closest_box_hits")
            _same_hit(flat.first_box_hits(rb, tmax), want[True], (name, "first_box_hits", lim))
            took(box_kernel, 6, "first_box_hits")
            assert np.array_equal(flat.box_occluded(rb, tmax), want[True][1] != NONE), (name, "box_occluded", lim)
    tune, sphere_kernel = _walk_for(seed, 1, c["wide_eligible"])
    with _tuned(ctx, tune):
        for lim, tmax in limited["sphere"].items():
            want = {first: sphere_match(off, idx, rays, ex["spheres"], tmax, first, hits=records["sphere"]) for first in (False, True)}
            _same_hit(flat.closest_sphere_hits(rb, tmax), want[False], (name, "closest_sphere_hits", lim))
            took(sphere_kernel, 7, "closest_sphere_hits")
            _same_hit(flat.first_sphere_hits(rb, tmax), want[True], (name, "first_sphere_hits", lim))
            took(sphere_kernel, 8, "first_sphere_hits")
            assert np.array_equal(flat.sphere_occluded(rb, tmax), want[True][1] != NONE), (name, "sphere_occluded", lim)

    # k hits: three leaves x three k x (no segment end, the drawn ones), thinned on a big CSR
    khits_reps, allhits_reps = _repetitions(seed, ks, len(idx) > BIG_CSR)
    khits = {}
    for leaf in fs.LEAVES:
        for k, lim in khits_reps:
            tmax = limited[leaf][lim]
            khits[leaf, k, lim] = flat.khits_batch(rb, k, leaf, tmax)
            _same_khits(khits[leaf, k, lim], khr.khits_match(off, idx, records[leaf], tmax, k), (name, "khits", leaf, k, lim))

    # all hits: sorted and in list order; one leaf per seed with rays and segment ends resident on the device; the head of every sorted
    # row against khits_batch's row, GPU against GPU
    on_device = fs.LEAVES[seed % 3]
    rb_dev = _dev_rays(eng, rays)
    for leaf in fs.LEAVES:
        for sort, lim in allhits_reps:
            tmax = limited[leaf][lim]
            if leaf == on_device:
                got = flat.allhits_batch(rb_dev, leaf, None if tmax is None else torch.from_numpy(tmax.copy()).cuda(), sort)
            else:
                got = flat.allhits_batch(rb, leaf, tmax, sort)
            got = _to_host(*got)
            _same_csr(got, ar.allhits_match(off, idx, records[leaf], tmax, sort), (name, "allhits", leaf, lim, sort))
            if sort:
                for k in ks:
                    if (leaf, k, lim) in khits:
                        _same_khits(ar.head_rows(*got, k), khits[leaf, k, lim], (name, "allhits head", leaf, k, lim))
    print(f"{name}: n = {scene['n']}, {len(rays)} rays, {len(kpts)} points, k = {ks}; references {t1 - t0:.2f} s, GPU side "
          f"{time.perf_counter() - t1:.2f} s, CSR of {len(idx)} members")
