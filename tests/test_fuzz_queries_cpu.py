"""What the default seeds of tests/test_gpu_fuzz_queries.py contain, shown on the oracle and the references alone: a fuzz that never reaches
a regime must not look green.  Every assertion is on fuzz_scenes.case(seed) / fuzz_scenes.knn_rows(seed) — the scenes, records and rows
the GPU file compares — over the seeds it runs by default.  A regime that the draw cannot reach is asserted absent by name, so that a
later change to the draw flips an assertion here and does not pass unnoticed."""
import os

import numpy as np
import pytest

import allhits_ref as ar
import fuzz_scenes as fs
import khits_ref as khr
import knn_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SEEDS = range(fs.DEFAULT_SEEDS)        # what tests/test_gpu_fuzz_queries.py runs unless BVH_FUZZ_SEEDS says otherwise
LANE_ROW_MAX = ar.engine_thresholds(ROOT)[0]


def test_maps_cover_what_they_claim():
    name = {np.float32: "f32", np.float64: "f64"}
    triple = lambda t: (name[t[0]], t[1], fs.k_scales(t[0]).index(t[2]))
    assert len({triple(fs.historic(s)) for s in range(400)}) == 8                      # the old map, however many seeds
    for first in (0, 16, 37):
        sixteen = [triple(fs.combo(s)) for s in range(first, first + 16)]
        assert len({(k, sc) for _, k, sc in sixteen}) == 16
        assert len({(d, k) for d, k, _ in sixteen}) == 8 and len({(d, sc) for d, _, sc in sixteen}) == 8
        assert len({triple(fs.combo(s)) for s in range(first, first + 32)}) == 32
    # the eight combinations test_fuzz_all_queries_other_combos adds to the historic eight: every pair of axes is then covered
    both = {triple(fs.historic(s)) for s in range(8)} | {triple((d, k, fs.k_scales(d)[si])) for d, k, si in fs.OTHER_COMBOS}
    assert len(both) == 16 and len({(k, sc) for _, k, sc in both}) == 16
    assert len({(d, k) for d, k, _ in both}) == 8 and len({(d, sc) for d, _, sc in both}) == 8


def _candidates(c, leaf, tmax=None):
    return khr.candidate_counts(c["off"], c["records"][leaf], tmax)


def _rows_with_ties(c, leaf):
    """per ray: does its sorted row hold two candidates of equal distance"""
    off, shape, vals = ar.allhits_match(c["off"], c["idx"], c["records"][leaf], None, True)
    o = off.astype(np.int64)
    same = np.zeros(len(vals), dtype=bool)
    same[1:] = vals[1:, 0] == vals[:-1, 0]
    same[o[:-1][o[:-1] < len(vals)]] = False                                          # (a row's first entry has no neighbour in its row)
    out = np.zeros(len(o) - 1, dtype=bool)
    out[np.repeat(np.arange(len(o) - 1), np.diff(o))[same]] = True
    return out


@pytest.mark.parametrize("leaf", fs.LEAVES)
def test_rows_tie_and_cross_the_tiers(leaf):
    """ties (the stable insertion of khits.hip / allhits.hip's lane tier, the (distance, position) key of the sort tiers), rows beyond the
    lane tier, rows that k = 64 cuts — and ties inside rows of the sort tiers"""
    ties, long_rows, cut_rows, ties_in_long = {}, {}, {}, {}
    for seed in SEEDS:
        c = fs.case(seed)
        n = _candidates(c, leaf)
        t = _rows_with_ties(c, leaf)
        ties[seed], long_rows[seed], cut_rows[seed] = int(t.sum()), int((n > LANE_ROW_MAX).sum()), int((n > 64).sum())
        ties_in_long[seed] = int((t & (n > LANE_ROW_MAX)).sum())
    print(f"{leaf}: rays with a tie {ties}\n  rows > {LANE_ROW_MAX}: {long_rows}\n  rows > 64: {cut_rows}\n  ties in rows > {LANE_ROW_MAX}: {ties_in_long}")
    # in one scene at least, and there on ten rays at least: no regime hangs on a single ray
    assert min(max(ties.values()), max(long_rows.values()), max(cut_rows.values()), max(ties_in_long.values())) >= 10
    # two scenes at least tie, in both dtypes
    assert {fs.combo(s)[0] for s in SEEDS if ties[s] >= 20} == {np.float32, np.float64}


def test_absent_by_construction():
    """the triangle and the sphere stage yield no candidate in the all-subnormal and the overflow band (the absolute epsilon and r * r /
    dot(l, l) decide there), and without whole duplicates no triangle or sphere record of a ray equals another"""
    for seed in SEEDS:
        c = fs.case(seed)
        dtype, kind, k_scale = fs.combo(seed)
        band = fs.k_scales(dtype).index(k_scale)
        for leaf in ("triangle", "sphere"):
            if band in (1, 2):
                assert _candidates(c, leaf).sum() == 0, (fs.label(seed), leaf)
            elif kind in (0, 1):
                assert _rows_with_ties(c, leaf).sum() == 0, (fs.label(seed), leaf)
        if band in (1, 2):
            assert _candidates(c, "box").sum() > 0, fs.label(seed)                    # the box stage works there
    for seed in (2, 3):                                                               # ... and the draw alone: none on the tie-rich kinds either
        scene = fs.draw(seed, *fs.combo(seed))
        assert len(np.unique(scene["tri"].reshape(len(scene["tri"]), 9), axis=0)) == scene["n"], seed
        dup = fs.with_whole_duplicates(scene, seed)
        assert len(np.unique(dup["tri"].reshape(len(dup["tri"]), 9), axis=0)) <= scene["n"] - scene["n"] // 4, seed


def test_segment_ends_cut_rows_and_every_pin_occurs():
    for leaf in fs.LEAVES:
        partial, later_keeps, pinned = 0, 0, {name: 0 for name in fs.TMAX_PINS}
        for seed in SEEDS:
            c = fs.case(seed)
            ex = c["extras"]
            tmax, pins = ex["tmax"][leaf], ex["tmax_pins"][leaf]
            free, cut = _candidates(c, leaf), _candidates(c, leaf, tmax)
            partial += int(((cut > 0) & (cut < free)).sum())
            for name in fs.TMAX_PINS:
                pinned[name] += len(pins[name])
            assert np.isnan(tmax[pins["nan"]]).all() and np.isposinf(tmax[pins["inf"]]).all()
            assert (cut[np.concatenate([pins["nan"], pins["zero"], pins["minus_one"]])] == 0).all(), (fs.label(seed), leaf)
            assert np.array_equal(cut[pins["inf"]], free[pins["inf"]])
            # the exact pins: a candidate sits AT the segment end and is not admitted (strict <), one fewer at least than <= would admit
            o = c["off"].astype(np.int64)
            for r in np.concatenate([pins["first"], pins["later"]]):
                d = c["records"][leaf][o[r]:o[r + 1], 0]
                assert (d == tmax[r]).sum() >= 1 and cut[r] == (d < tmax[r]).sum() < (d <= tmax[r]).sum(), (fs.label(seed), leaf, r)
            later_keeps += int((cut[pins["later"]] >= 1).sum())                       # (later in the list: not always farther)
        print(f"{leaf}: rays that keep some candidates and lose others {partial}; pinned rays {pinned}, {later_keeps} of the later pins keep a candidate")
        assert partial >= 100 and min(pinned.values()) >= 20 and later_keeps >= 10, (leaf, partial, pinned, later_keeps)


def test_odd_spheres_reach_the_lists():
    met = {name: 0 for name in fs.SPHERE_ODDITIES}
    hits = {name: 0 for name in fs.SPHERE_ODDITIES}
    for seed in SEEDS:
        c = fs.case(seed)
        ex = c["extras"]
        odd = ex["oddity"][c["idx"].astype(np.int64)]
        r = ex["spheres"][:, 3]
        for j, name in enumerate(fs.SPHERE_ODDITIES):
            met[name] += int((odd == j).sum())
            hits[name] += int(np.isfinite(ex["sphere"][odd == j, 0]).sum())
        with np.errstate(invalid="ignore"):
            assert (r[ex["oddity"] == 0] == 0).all() and (r[ex["oddity"] == 1] <= 0).all() and np.isnan(r[ex["oddity"] == 2]).all()
        assert np.isposinf(r[ex["oddity"] == 3]).all()
        assert 0.01 <= (ex["oddity"] >= 0).mean() <= 0.06 or c["scene"]["n"] < 1000, fs.label(seed)
    print(f"list members with an odd sphere {met}, of which hit {hits}")
    assert min(met.values()) >= 100, met
    assert hits["r_negative"] >= 10 and hits["r_tenfold"] >= 10 and hits["r_nan"] == 0 and hits["r_inf"] == 0, hits


def test_k_nearest_rows_tie_pad_and_meet_their_limits():
    ties = {0: 0, 1: 0}          # rows with equal neighbouring distances, per shape distance
    at_the_cut = {0: 0, 1: 0}    # (point, k) whose k-th and (k+1)-th nearest distances are equal: a full list meets its own bound again
    padded = partial = unlimited = 0
    pinned = {name: 0 for name in fs.LIMIT_PINS}
    differ = 0
    for seed in SEEDS:
        c = fs.case(seed)
        ex, rows = c["extras"], fs.knn_rows(seed)
        n = c["scene"]["n"]
        assert ex["ks"][0] == 1 and 2 <= ex["ks"][1] <= 63 and ex["ks"][2] == 64
        for kind in (0, 1):
            shape, dist = rows["flat"][kind][64]
            real = shape != NONE
            ties[kind] += int(((dist[:, 1:] == dist[:, :-1]) & real[:, 1:] & (shape[:, 1:] != shape[:, :-1])).any(axis=1).sum())
            for p in ex["kpts"]:
                d2 = np.sort(kr.dists_vector(c["oflat"], c["scene"]["aabbs"], p, dist.dtype.type, c["scene"]["tri"] if kind else None)[1])
                at_the_cut[kind] += sum(int(d2[k - 1] == d2[k]) for k in ex["ks"] if n > k)
            if n < 64:
                assert (real.sum(axis=1) == n).all() and np.isposinf(dist[~real]).all()
                padded += 1
            free, lim = rows["tree"][kind]["none"][64][0], rows["tree"][kind]["limit"][64][0]
            kept, of = (lim != NONE).sum(axis=1), (free != NONE).sum(axis=1)
            partial += int(((kept > 0) & (kept < of)).sum())
            m, pins = ex["max_dist"][kind], ex["limit_pins"][kind]
            for name in fs.LIMIT_PINS:
                pinned[name] += len(pins[name])
            # (+inf is no limit for numbers, but x <= inf * inf turns a NaN distance away where no limit lets it in: <=, not ==)
            assert (kept[np.concatenate([pins["minus_one"], pins["nan"]])] == 0).all() and (kept[pins["inf"]] <= of[pins["inf"]]).all()
            unlimited += int((kept[pins["inf"]] == of[pins["inf"]]).sum())
            assert (m[pins["zero"]] == 0).all() and np.isnan(m[pins["nan"]]).all() and np.isposinf(m[pins["inf"]]).all()
            differ += int((rows["flat"][kind][64][0] != free).any(axis=1).sum())
    print(f"rows with ties {ties}, ties across the cut at k {at_the_cut}, scenes x distances with padding {padded}, "
          f"points whose limit keeps some and loses others {partial}, pinned {pinned}, k = 64 rows the two forms order differently {differ}")
    assert min(ties.values()) >= 50 and min(at_the_cut.values()) >= 20, (ties, at_the_cut)
    assert padded >= 2 and partial >= 100 and min(pinned.values()) >= 20 and unlimited >= 20 and differ >= 10
