"""Fuzz over every query family of instanced scenes — closest_hits / any_hits / occluded, allhits_batch, khits_batch, within_batch,
knearest_batch / nearest_batch and region_batch, and update() followed by one leg of each — on the random scenes of
tests/fuzz_instances.py: 1 to 1 000 instances (one, two and three workgroups of k_instances_prep<T, 1>; top levels of the builder's wave,
workgroup and level tiers), members of 1 to 1 100 shapes (up to five passes of prep phase 0's stride loop), four scene characters
(well-conditioned poses, an exact lattice with whole duplicates, members stored at 2^+-e, singular / overflowing / underflowing
transforms), both dtypes.  One set per seed; every leg against its reference byte for byte (two NaNs count as equal).
tests/test_fuzz_instances_cpu.py shows on the references alone what the default seeds contain — and the one thing they cannot: a 2^70
world box overflows the surface areas of the top level's SAH, so the region rows of the degenerate seeds are empty by definition.

The input memory space is a function of the seed: even seeds pass host arrays, odd seeds device tensors (rays, tmax, points, limits,
planes); every fourth seed passes the transforms and tree_of as device tensors as well."""
import os
import time

import numpy as np
import pytest

import fuzz_instances as fi
import instances_allhits_ref as iar
import instances_khits_ref as ikh
import instances_knn_ref as iknn
import instances_within_ref as iwr
from test_fp_extremes_cpu import same as same_bytes  # byte equality, two NaNs equal
from test_gpu_any_hit import _rb

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


def _np(a):
    """an engine output as numpy: indices as uint32 (a device tensor holds them as int32, offsets as int64)"""
    if a is None or isinstance(a, np.ndarray):
        return a
    a = a.cpu().numpy()
    if a.dtype == np.int32:
        return a.view(np.uint32)
    if a.dtype == np.int64:
        assert a.min(initial=0) >= 0 and a.max(initial=0) <= NONE
        return a.astype(np.uint32)
    return a


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _dev_rays(eng, rays):
    import torch
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    return eng.RayBatch.from_device(torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda(), len(rays), dt)


def _same(got, want, names, label, offsets=None):
    """arrays in order, byte for byte (two NaNs equal); a difference names the first differing rows — of the CSR `offsets` if given"""
    for name, g, w in zip(names, got, want):
        g, w = _np(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.kind == "f":
            if same_bytes(g, w):
                continue
            with np.errstate(invalid="ignore"):
                differ = ~((g == w) & (np.signbit(g) == np.signbit(w)) | (np.isnan(g) & np.isnan(w)))
        else:
            differ = g != w
        bad = np.unique(np.nonzero(differ)[0])[:5]
        if len(bad):
            rows = bad if offsets is None or name == "offsets" else np.searchsorted(np.asarray(offsets), bad, side="right") - 1
            raise AssertionError((label, name, "first differing rows", rows.tolist(), "got", g[bad].tolist(), "want", w[bad].tolist()))


def _region_want(ref, combo):
    off, inst, shape, ins = ref["full"]
    toff, tidx, _ = ref["top"]
    return dict(plain=(("offsets", "instance", "shape"), (off, inst, shape)),
                classify=(("offsets", "instance", "shape", "inside"), (off, inst, shape, ins)),
                count_only=(("offsets",), (off,)),
                instances_only=(("offsets", "instance"), (toff, tidx)))[combo]


def _region_leg(inst, planes, ref, combo, label):
    kw = dict(classify=combo == "classify", count_only=combo == "count_only", instances_only=combo == "instances_only")
    got = inst.region_batch(planes, **kw)
    names, want = _region_want(ref, combo)
    if combo == "count_only":
        assert _np(got["instance"]).size == 0, label
    else:
        assert set(got) == set(names), (label, sorted(got))
    _same([got[n] for n in names], want, names, label, offsets=want[0])


@pytest.mark.parametrize("seed", range(int(os.environ.get("BVH_FUZZ_SEEDS", fi.DEFAULT_SEEDS))))   # BVH_FUZZ_SEEDS=32: every combination with the other dtype too
def test_fuzz_instanced_queries(eng, seed):
    c = fi.case(seed)
    t0 = time.perf_counter() - c["seconds"]        # (the case is computed once per process: its own time is what counts)
    dtype, sc, sc2, ks, n = c["dtype"], c["scene"], c["scene2"], c["ks"], c["n"]
    name = fi.label(seed)
    nr, npts = len(c["rays"]), len(c["points"])
    free, cut, cut2 = c["free"], c["cut"], c["cut2"]
    tab, tab2 = free["table"], cut2["table"]
    want_rows = {(sort, lim): iar.rows(tab, nr, tm, dtype, sort) for sort in (True, False) for lim, tm in (("none", None), ("tmax", c["tmax"]))}
    want_khits = {(k, lim): ikh.definition(tab, nr, tm, k, dtype) for k in ks for lim, tm in (("none", None), ("tmax", c["tmax"]))}
    want_within = {sort: iwr.csr(c["within"], dtype, sort) for sort in (True, False)}
    want_scalar = {sort: iwr.csr(c["within_scalar"], dtype, sort) for sort in (True, False)}
    want_knn = {k: iknn.padded(c["knn"][k], k, dtype) for k in ks}
    want_rows2 = iar.rows(tab2, nr, c["tmax"], dtype, True)
    want_within2 = iwr.csr(c["within2"], dtype, True)
    want_knn2 = iknn.padded(c["knn2"], ks[1], dtype)
    t1 = time.perf_counter()

    # the seed decides where the inputs live
    device = seed % 2 == 1
    put = _dev if device else (lambda a: a)
    rb = _dev_rays(eng, c["rays"]) if device else _rb(eng, c["rays"])
    tmax, pts, limits, planes = put(c["tmax"]), put(c["points"]), put(c["limits"]), put(c["planes"])
    scalar_pts = put(c["scalar_points"])
    set_on_device = seed % 4 == 3
    tree_of = _dev(c["tree_of"].astype(np.int32)) if set_on_device else c["tree_of"]
    x = _dev(c["x"].reshape(n, 12)) if set_on_device else c["x"]
    x2 = _dev(c["x2"].reshape(n, 12)) if set_on_device else c["x2"]

    ctx = eng.Context(0)
    trees = []
    for t, (aabbs, tris) in enumerate(c["trees"]):
        flat = eng.FlatBvh.from_flat_nodes(sc.flats[t], aabbs, ctx) if t == c["uploaded"] else eng.Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris)
        trees.append(flat)
    with eng.Instances(trees, tree_of, x, ctx) as inst:
        # 1, 2: the commit first — a wrong inverse or world box must not show up as seven query failures
        assert inst.info() == (len(trees), n), name
        _same([inst.world_boxes], [sc.w], ["world_boxes"], (name, "world_boxes"))

        # 3: closest, first, occluded
        hit = ("vals", "instance", "shape")
        for lim, tm, want in (("none", None, free), ("tmax", tmax, cut)):
            _same(_order(inst.closest_hits(rb, tm)), _order(want["closest"]), hit, (name, "closest_hits", lim))
            _same(_order(inst.any_hits(rb, tm)), _order(want["first"]), hit, (name, "any_hits", lim))
            _same([inst.occluded(rb, tm)], [want["first"][1] != NONE], ["occluded"], (name, "occluded", lim))

        # 4: all hits, sorted and in list order; count_only; the heads are the closest and the first hit
        csr = ("offsets", "instance", "shape", "vals")
        for (sort, lim), want in want_rows.items():
            tm = None if lim == "none" else tmax
            got = inst.allhits_batch(rb, tm, sort=sort)
            _same([got[k] for k in csr], want, csr, (name, "allhits_batch", "sorted" if sort else "list order", lim), offsets=want[0])
            counts = inst.allhits_batch(rb, tm, sort=sort, count_only=True)
            assert set(counts) == {"offsets"}, name
            _same([counts["offsets"]], want[:1], csr[:1], (name, "allhits_batch count_only", sort, lim))
            off = _np(got["offsets"]).astype(np.int64)
            rows = np.nonzero(np.diff(off))[0]
            head = (free if lim == "none" else cut)["closest" if sort else "first"]
            assert np.array_equal(rows, np.nonzero(head[1] != NONE)[0]), (name, "allhits rows and hits", sort, lim)
            _same([_np(got["vals"])[off[rows]], _np(got["instance"])[off[rows]], _np(got["shape"])[off[rows]]],
                  [head[0][rows], head[1][rows], head[2][rows]], hit, (name, "allhits head", sort, lim))

        # 5: k hits
        padded = ("instance", "shape", "vals")
        for (k, lim), want in want_khits.items():
            _same(inst.khits_batch(rb, k, None if lim == "none" else tmax), want, padded, (name, "khits_batch", k, lim))

        # 6: radius search: sorted, list order, count_only; per-point limits and one scalar limit
        wcsr = ("offsets", "instance", "shape", "dist")
        for what, p, m, wants in (("limits", pts, limits, want_within), ("scalar", scalar_pts, c["scalar_limit"], want_scalar)):
            for sort, want in wants.items():
                got = inst.within_batch(p, m, sort=sort)
                _same([got[k] for k in wcsr], want, wcsr, (name, "within_batch", what, "sorted" if sort else "list order"), offsets=want[0])
            counts = inst.within_batch(p, m, count_only=True)
            assert set(counts) == {"offsets"}, name
            _same([counts["offsets"]], wants[True][:1], wcsr[:1], (name, "within_batch count_only", what))

        # 7: k nearest, and nearest
        kn = ("instance", "shape", "dist")
        for k, want in want_knn.items():
            _same(inst.knearest_batch(pts, k), want, kn, (name, "knearest_batch", k))
        _same(inst.nearest_batch(pts), [a[:, 0] for a in want_knn[1]], kn, (name, "nearest_batch"))

        # 8: regions
        for combo in ("plain", "classify", "count_only", "instances_only"):
            _region_leg(inst, planes, c["region"], combo, (name, "region_batch", combo))

        # 9: the second pose, and one leg of every family on it
        assert inst.update(x2) is inst
        _same([inst.world_boxes], [sc2.w], ["world_boxes"], (name, "update: world_boxes"))
        _same(_order(inst.closest_hits(rb, tmax)), _order(cut2["closest"]), hit, (name, "update: closest_hits"))
        got = inst.allhits_batch(rb, tmax)
        _same([got[k] for k in csr], want_rows2, csr, (name, "update: allhits_batch"), offsets=want_rows2[0])
        got = inst.within_batch(pts, limits)
        _same([got[k] for k in wcsr], want_within2, wcsr, (name, "update: within_batch"), offsets=want_within2[0])
        _same(inst.knearest_batch(pts, ks[1]), want_knn2, kn, (name, "update: knearest_batch", ks[1]))
        _region_leg(inst, planes, c["region2"], "plain", (name, "update: region_batch"))
    t2 = time.perf_counter()
    print(f"{name}: n = {n}, members {c['counts']}{' (one uploaded)' if c['uploaded'] is not None else ''}, {nr} rays, {npts} points, "
          f"k = {ks}, {c['planes'].shape[1]} planes, inputs {'in HBM' if device else 'on the host'}; references {t1 - t0:.2f} s "
          f"(the case {c['seconds']:.2f} s), engine {t2 - t1:.2f} s; candidate table {len(tab['ray'])}, within {len(want_within[True][1])}, "
          f"region {c['region']['full'][0][-1]} pairs")


def _order(r):
    """(vals, instance, shape) as the engine and Scene.trace both give them"""
    return [r[0], r[1], r[2]]
