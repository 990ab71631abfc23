"""What the default seeds of tests/test_gpu_fuzz_instances.py contain, shown on the oracle and the references alone: a fuzz that never reaches
a regime must not look green.  Every assertion is on fuzz_instances.case(seed) — the scenes and answers the GPU file compares — over the
seeds it runs by default.  The thresholds are conditions on the draw: a draw that misses one is changed or pinned (fuzz_instances.N_PINS,
SMALL_SETS), the condition stays.

Then two things about the references themselves.  The prune of the point families is honest: what the two-level walks of
instances_within_ref.rows / instances_knn_ref.rows return is what a brute force over all (instance, shape) pairs returns, except in
instances whose inverse is not finite (the definition's NaN r2o passes no box test) and for at most 1 pair in 1 000 where a box test and
the triangle distance round apart.  And the scenes are sensitive: ten subtle mutations of the definition, each applied to
a copy of the reference, change an answer on a default seed — a kernel wrong in that way would be seen.

Measured on the 16 default seeds: 4 059 rays whose closest hit is not their first; 1 505 lattice rays with tied candidates in different
instances; 248 hit rows longer than 32 and 47 longer than 64; 7 to 22 rays per segment-end pin and seed; 7 to 11 mixed 64-ray groups in
every lattice and degenerate seed, and no failing object ray in any posed seed; 6 to 46 non-finite inverses per degenerate seed, entered
by 124 to 306 rays; radius-search rows longer than 32 in 15 seeds, 83 empty ones; 60 k = 64 rows padded (seed 1) and 421 cut; 128 points
at distance 0; 136 lattice points with a tie at a k-th distance.  The largest share of pairs a brute force has and the walks lack outside
non-finite inverses is 9.0e-05 for the radius search (seed 0; 1.3e-05 in seed 15, 0 elsewhere) and 0 for the k nearest.  Every mutation
is seen, by seed 0, 1, 2 or 5.  The references of one seed take 0.1 to 7 s on a desktop CPU."""
import os

import numpy as np

import fuzz_instances as fi
import fuzz_scenes as fs
import instances_allhits_ref as iar
import instances_knn_ref as iknn
import instances_ref as ir
import instances_within_ref as iwr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SEEDS = range(fi.DEFAULT_SEEDS)        # what tests/test_gpu_fuzz_instances.py runs unless BVH_FUZZ_SEEDS says otherwise
LANE_ROW_MAX = iar.engine_thresholds(ROOT)[0]
PRUNE_CAP = 1e-3


def _kind(seed):
    return fi.KINDS[fi.combo(seed)[1]]


def _of_kind(*names):
    return [s for s in SEEDS if _kind(s) in names]


def ray_is_finite(rays):
    """common.hpp ray_is_finite: o finite, inv finite and nonzero (false for inf, for NaN and for +-0 in inv)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(rays["o"]) < np.inf).all(axis=1) & (np.abs(rays["inv"]) < np.inf).all(axis=1) & (rays["inv"] != 0).all(axis=1)


def object_frames(c):
    """per ray: does it enter an instance at all, and does it enter one in whose frame it fails ray_is_finite (by the top-level list)"""
    sc, rays = c["scene"], c["rays"]
    toff, tidx = c["free"]["top"]
    n = len(rays)
    ray_of = np.repeat(np.arange(n), np.diff(toff.astype(np.int64)))
    fails = np.zeros(n, dtype=bool)
    for i in np.unique(tidx):
        rid = ray_of[tidx == i]
        fails[rid[~ray_is_finite(sc.object_rays(rays[rid], int(i)))]] = True
    return np.diff(toff.astype(np.int64)) > 0, fails


def hit_rows(c, tmax=None, sort=True):
    return iar.rows(c["free"]["table"], len(c["rays"]), tmax, c["dtype"], sort)


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------
def test_combo_reaches_every_character_in_both_dtypes():
    for first in (0, 16, 32):
        sixteen = [fi.combo(s) for s in range(first, first + 16)]
        assert len(set(sixteen)) == 8 and all(sixteen.count(p) == 2 for p in set(sixteen))
        for s in range(first, first + 16):                                               # the other dtype 16 seeds later
            assert fi.combo(s + 16)[1] == fi.combo(s)[1] and fi.combo(s + 16)[0] != fi.combo(s)[0]
    assert fi.DEFAULT_SEEDS == 16


def test_a_case_is_a_pure_function_of_its_seed():
    a = fi.case(2)
    b = fi.case.__wrapped__(2)
    for key in ("x", "x2", "tree_of", "rays", "tmax", "points", "limits", "planes"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["ks"] == b["ks"] and a["counts"] == b["counts"]
    assert a["free"]["closest"][0].tobytes() == b["free"]["closest"][0].tobytes()


def test_sizes():
    ns = {s: fi.case(s)["n"] for s in SEEDS}
    assert {1, 2, 64, 65, 256, 257, 513} <= set(ns.values()), ns
    assert sum(800 <= n <= 1000 for n in ns.values()) >= 1 and all(1 <= n <= 1000 for n in ns.values())
    used = set()
    for s in SEEDS:
        c = fi.case(s)
        assert 2 <= len(c["counts"]) <= 5 and all(1 <= k <= 1100 for k in c["counts"])
        members = np.unique(c["tree_of"])
        assert len(members) == (1 if s in fi.SMALL_SETS else min(c["n"], len(c["counts"]))), fi.label(s)   # every member is used when n allows
        used |= {c["counts"][int(t)] for t in members}
        for (aabbs, tris), k in zip(c["trees"], c["counts"]):
            assert len(aabbs) == len(tris) == k and aabbs.dtype == tris.dtype == c["dtype"]
        assert 450 <= len(c["rays"]) <= 701 and len(c["rays"]) % 64 != 0
        assert fi.MIN_POINTS <= len(c["points"]) <= fi.MAX_POINTS and c["planes"].shape[0] == fi.N_REGIONS
        assert c["ks"][0] == 1 and 2 <= c["ks"][1] <= 63 and c["ks"][2] == 64
    assert set(fi.MEMBER_COUNTS) <= used, used
    by_kind = {}
    for s in SEEDS:
        by_kind.setdefault(_kind(s), []).append(ns[s])
    for kind, sizes in by_kind.items():                                                # every character at small and at large instance counts
        assert min(sizes) <= 128 and max(sizes) >= 256, (kind, sizes)
    assert sum(fi.case(s)["uploaded"] is not None for s in SEEDS) == len([s for s in SEEDS if s % 3 == 1]) >= 5
    assert {fi.case(s)["planes"].shape[1] for s in SEEDS} == set(fi.PLANE_COUNTS)


def test_scene_characters_are_what_they_are_named_for():
    for s in _of_kind("lattice"):
        c = fi.case(s)
        for x in (c["x"], c["x2"]):
            m = x[:, :, :3]
            assert ((m != 0).sum(axis=2) == 1).all() and ((m != 0).sum(axis=1) == 1).all() and np.isin(np.abs(m[m != 0]), [0.5, 1, 2]).all()
            assert (x[:, :, 3] % 4 == 0).all()
            keyed = np.concatenate([x.reshape(len(x), 12), c["tree_of"][:, None].astype(x.dtype)], axis=1)
            assert len(np.unique(keyed, axis=0)) <= len(x) - len(x) // 3, fi.label(s)   # whole duplicates: same member, same transform
        assert np.signbit(c["x"][:, :, 3][c["x"][:, :, 3] == 0]).any() or c["n"] < 8       # (-0 translations are there)
        for _, tris in c["trees"]:
            assert (tris * 2 == np.round(tris * 2)).all()
    for s in _of_kind("scaled"):
        c = fi.case(s)
        e = fi.scale_exponent(c["dtype"])
        with np.errstate(all="ignore"):
            y = np.abs(c["scene"].y[:, :, :3].astype(np.float64))
        assert np.isfinite(c["scene"].y).all() and y.max() >= 2.0 ** (e - 2) and y[y > 0].min() <= 2.0 ** (2 - e), fi.label(s)
        sizes = sorted(float(np.abs(t[1]).max()) for t in c["trees"])
        assert sizes[0] <= 2.0 ** (3 - e) and sizes[-1] >= 2.0 ** (e - 1)
        assert np.abs(c["scene"].w).max() < 1e3                                          # ... and every copy has world size ~ 1


# ---- ray families -----------------------------------------------------------------------------------------------------------------------
def test_ray_families_reach_their_regimes():
    later = ties = long_rows = cut = pad = 0
    pins_min = {}
    for s in SEEDS:
        c = fi.case(s)
        free = c["free"]
        later += int(((free["closest"][1] != free["first"][1]) | (free["closest"][2] != free["first"][2])).sum())
        off, inst, shape, vals = hit_rows(c)
        o = off.astype(np.int64)
        counts = np.diff(o)
        same = np.zeros(len(vals), dtype=bool)
        same[1:] = (vals[1:, 0] == vals[:-1, 0]) & (inst[1:] != inst[:-1])
        same[o[:-1][o[:-1] < len(vals)]] = False                                         # (a row's first entry has no neighbour in its row)
        tied = np.zeros(len(counts), dtype=bool)
        tied[np.repeat(np.arange(len(counts)), counts)[same]] = True
        if _kind(s) == "lattice":
            ties += int(tied.sum())
        long_rows += int((counts > LANE_ROW_MAX).sum())
        cut += int((counts > 64).sum())
        pad += int(((counts > 0) & (counts < 64)).sum())
        assert (counts > 0).sum() >= 120, fi.label(s)                                    # every default seed has hits, and enough for its pins
        tmax, pins = c["tmax"], c["tmax_pins"]
        pins_min[s] = min(len(pins[name]) for name in fs.TMAX_PINS)
        assert pins_min[s] >= 5, (fi.label(s), {k: len(v) for k, v in pins.items()})
        assert np.isnan(tmax[pins["nan"]]).all() and (tmax[pins["zero"]] == 0).all() and (tmax[pins["minus_one"]] == -1).all()
        assert np.isposinf(tmax[pins["inf"]]).all()
        kept = np.diff(hit_rows(c, tmax)[0].astype(np.int64))
        assert (kept[np.concatenate([pins["nan"], pins["zero"], pins["minus_one"]])] == 0).all() and np.array_equal(kept[pins["inf"]], counts[pins["inf"]])
        tab = free["table"]
        for r in np.concatenate([pins["first"], pins["later"]]):                         # a candidate sits AT the segment end: strict < leaves it out
            d = tab["vals"][tab["cand_off"][r]:tab["cand_off"][r + 1], 0]
            assert (d == tmax[r]).sum() >= 1 and kept[r] == (d < tmax[r]).sum() < (d <= tmax[r]).sum(), (fi.label(s), r)
    print(f"closest != first on {later} rays; lattice rays with tied candidates in different instances {ties}; hit rows > {LANE_ROW_MAX}: "
          f"{long_rows}, > 64: {cut}, of 1 .. 63: {pad}; fewest rays of a tmax pin per seed {pins_min}")
    assert later >= 200 and ties >= 100 and long_rows >= 50 and cut >= 1 and pad >= 1


def test_waves_mix_finite_and_non_finite_object_rays():
    mixed, clean_posed = {}, []
    for s in SEEDS:
        c = fi.case(s)
        enters, fails = object_frames(c)
        group = np.arange(len(enters)) // 64
        both = [g for g in np.unique(group) if (fails & (group == g)).any() and (enters & ~fails & (group == g)).any()]
        mixed[s] = len(both)
        if _kind(s) in ("lattice", "degenerate"):
            assert len(both) >= 4, (fi.label(s), len(both))
        if _kind(s) == "posed" and not fails.any():
            clean_posed.append(s)
        if _kind(s) == "lattice":                                                        # d'[k] == +-0, and world rays that are not finite themselves
            assert (~ray_is_finite(c["rays"])).sum() >= 20 and fails.sum() >= 50, fi.label(s)
    print(f"64-ray groups with both kinds of ray, per seed: {mixed}; posed seeds without a failing ray: {clean_posed}")
    assert clean_posed


def test_degenerate_transforms_commit_and_are_entered():
    for s in _of_kind("degenerate"):
        c = fi.case(s)
        for sc, klass in ((c["scene"], c["klass"]), (c["scene2"], c["klass2"])):
            assert np.isfinite(sc.w).all(), fi.label(s)                                  # the commit succeeds
            assert np.isfinite(sc.x).all()                                               # nothing non-finite goes INTO a transform
            bad = ~np.isfinite(sc.y).all(axis=(1, 2))
            assert bad.sum() >= 3 and not bad[klass < 0].any(), (fi.label(s), int(bad.sum()))
            assert {int(k) for k in klass[klass >= 0]} >= {0, 1, 2, 3}, fi.label(s)
        assert not np.array_equal(c["klass"] >= 0, c["klass2"] >= 0)                     # update() moves which instances are degenerate
        sc = c["scene"]
        bad = ~np.isfinite(sc.y).all(axis=(1, 2))
        toff, tidx = c["free"]["top"]
        ray_of = np.repeat(np.arange(len(c["rays"])), np.diff(toff.astype(np.int64)))
        into_bad = np.zeros(len(c["rays"]), dtype=bool)
        into_bad[ray_of[bad[tidx.astype(np.int64)]]] = True
        hit = c["free"]["closest"][1] != NONE
        print(f"{fi.label(s)}: {int(bad.sum())} of {c['n']} inverses are not finite, {int(into_bad.sum())} rays enter one, "
              f"{int((hit & ~into_bad).sum())} of the {int((~into_bad).sum())} others have a hit")
        assert into_bad.sum() >= 20 and (hit & ~into_bad).sum() >= 20, fi.label(s)


def test_regions_report_pairs_except_over_an_overflowing_top_level():
    """a 2^70 world box overflows the surface areas of the top level's SAH: its root split has no winner and leaves empty child bounds, and by
    the definition no region with a plane reaches an instance through them — every degenerate seed's rows are empty, in both poses"""
    partly = wholly = 0
    for s in SEEDS:
        c = fi.case(s)
        for sc, ref in ((c["scene"], c["region"]), (c["scene2"], c["region2"])):
            total = int(ref["full"][0][-1])
            if _kind(s) == "degenerate":
                assert fs.has_empty_child_bounds(sc.top) and total == 0 and len(ref["top"][1]) == 0, fi.label(s)
            else:
                assert not fs.has_empty_child_bounds(sc.top) and total >= 100 and (np.diff(ref["full"][0].astype(np.int64)) > 0).sum() >= 8, (fi.label(s), total)
        inside = c["region"]["full"][3]
        partly, wholly = partly + int((inside == 0).sum()), wholly + int((inside == 1).sum())
    print(f"region pairs partly inside {partly}, wholly inside {wholly}")
    assert partly >= 1000 and wholly >= 1000


# ---- point families ---------------------------------------------------------------------------------------------------------------------
def _pair_distances(c):
    """per point the squared distances to every (instance, shape) pair, ascending"""
    sc, pts = c["scene"], c["points"]
    g = iknn._Dists(sc, iknn._points(sc, pts), {})
    with np.errstate(all="ignore"):
        return [np.sort(np.concatenate([np.asarray(d, dtype=np.float64) for d in g.d(j)])) for j in range(len(pts))]


def test_point_families_reach_their_regimes():
    long_seeds, empty, zero, padded, cut, kth_ties = [], 0, 0, 0, 0, 0
    pinned = {name: 0 for name in fs.LIMIT_PINS}
    for s in SEEDS:
        c = fi.case(s)
        lens = np.array([len(r) for r in c["within"]])
        if (lens > 32).any():
            long_seeds.append(s)
        empty += int((lens == 0).sum())
        m = c["limits"]
        for name in fs.LIMIT_PINS:
            pinned[name] += len(c["limit_pins"][name])
        p = c["limit_pins"]
        assert (m[p["zero"]] == 0).all() and (m[p["minus_one"]] == -1).all() and np.isnan(m[p["nan"]]).all() and np.isposinf(m[p["inf"]]).all()
        assert (lens[np.concatenate([p["minus_one"], p["nan"]])] == 0).all()
        rows64 = c["knn"][64]
        padded += sum(len(r) < 64 for r in rows64)
        cut += sum(len(r) == 64 for r in rows64) if c["n_pairs"] > 64 else 0
        zero += sum(1 for r in c["knn"][1] if len(r) and r[0][0] == 0)
        if _kind(s) == "lattice":
            for d2 in _pair_distances(c):
                kth_ties += int(any(k < len(d2) and d2[k - 1] == d2[k] for k in c["ks"]))
    print(f"seeds with within rows > 32: {long_seeds}; empty within rows {empty}; limit pins {pinned}; k = 64 rows padded {padded}, cut {cut}; "
          f"points at distance 0 {zero}; lattice points with a tie at a k-th distance {kth_ties}")
    assert len(long_seeds) >= 3 and empty >= 1 and min(pinned.values()) >= 1 and padded >= 1 and cut >= 1 and zero >= 1 and kth_ties >= 20


def _excused(sc):
    """instances whose inverse is not finite: the definition's NaN r2o / q passes no box test there"""
    return ~np.isfinite(sc.y).all(axis=(1, 2))


def test_the_prune_is_honest():
    worst = {"within": 0.0, "knearest": 0.0}
    for s in SEEDS:
        c = fi.case(s)
        sc, pts = c["scene"], c["points"]
        nofin = _excused(sc)
        # radius search: rows is a subset of brute
        brute = iwr.brute(sc, pts, c["limits"])
        total = missing = 0
        for row, want in zip(c["within"], brute):
            got = {(i, k) for _, i, k in row}
            assert len(got) == len(row) and got <= want, fi.label(s)
            total += len(want)
            missing += sum(1 for i, _ in want - got if not nofin[i])
        share_w = missing / max(total, 1)
        # k nearest: the same pairs (and so the same distance multiset); a pair that only a non-finite inverse hides is made up for by another
        cache = {}
        total = missing = 0
        for k in c["ks"]:
            for row, want in zip(c["knn"][k], iknn.brute(sc, pts, k, cache=cache)):
                got, ref = {(i, j) for _, i, j in row}, {(i, j) for _, i, j in want}
                lost = ref - got
                assert len(got - ref) <= len(lost), fi.label(s)
                if not lost:
                    assert sorted(d for d, _, _ in row) == sorted(d for d, _, _ in want) or any(d != d for d, _, _ in want), fi.label(s)
                total += len(ref)
                missing += sum(1 for i, _ in lost if not nofin[i])
        share_k = missing / max(total, 1)
        print(f"{fi.label(s)}: pairs a brute force has and the walk lacks outside non-finite inverses: within {share_w:.2e}, k nearest {share_k:.2e}")
        assert share_w <= PRUNE_CAP and share_k <= PRUNE_CAP, (fi.label(s), share_w, share_k)
        worst["within"], worst["knearest"] = max(worst["within"], share_w), max(worst["knearest"], share_k)
    print(f"largest shares: {worst}")


# ---- sensitivity: a subtly wrong kernel would be seen ------------------------------------------------------------------------------------
def select(table, n, tmax, dtype, first=False, closest_le=False, tmax_le=False):
    """a copy of Scene.trace's closest / first rule over a candidate table, with its two comparisons open to mutation"""
    ft = np.dtype(dtype).type
    tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
    vals = np.zeros((n, 3), dtype=ft); vals[:, 0] = np.inf
    inst = np.full(n, NONE, dtype=np.uint32); shape = np.full(n, NONE, dtype=np.uint32)
    off = table["cand_off"]
    for j in range(n):
        for c in range(off[j], off[j + 1]):
            d = table["vals"][c, 0]
            inside = d <= tm[j] if tmax_le else d < tm[j]
            nearer = first or (d <= vals[j, 0] if closest_le else d < vals[j, 0])
            if inside and nearer:
                vals[j] = table["vals"][c]; inst[j] = table["instance"][c]; shape[j] = table["shape"][c]
                if first:
                    break
    return vals, inst, shape


def _same_hits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def rows_reversing_ties(table, n, dtype):
    """instances_allhits_ref.rows with a sort that reverses equal keys"""
    off = table["cand_off"]
    sel = []
    for j in range(n):
        lo, hi = int(off[j]), int(off[j + 1])
        d = table["vals"][lo:hi, 0]
        keep = np.nonzero(d < np.inf)[0]
        sel.append(lo + keep[np.lexsort((-keep, d[keep]))])
    sel = np.concatenate(sel).astype(np.int64)
    return table["instance"][sel], table["shape"][sel]


def inverse_other_association(x):
    """instances_ref.inverse with y[k][3] summed as a + (b + c)"""
    y = _true["inverse"](x)
    with np.errstate(all="ignore"):
        for k in range(3):
            y[:, k, 3] = -((y[:, k, 0] * x[:, 0, 3]) + ((y[:, k, 1] * x[:, 1, 3]) + y[:, k, 2] * x[:, 2, 3]))
    return y


def world_boxes_two_corners(bounds, tree_of, x):
    """instances_ref.world_boxes from the corners 0 and 7 alone"""
    with np.errstate(all="ignore"):
        lo, hi = ir.forward(x, bounds[tree_of, :3]), ir.forward(x, bounds[tree_of, 3:])
    return np.concatenate([np.minimum(lo, hi), np.maximum(lo, hi)], axis=1).astype(x.dtype)


def stretch_two_rows(y):
    return (y[0, 0] * y[0, 0] + y[0, 1] * y[0, 1]) + y[0, 2] * y[0, 2] + ((y[1, 0] * y[1, 0] + y[1, 1] * y[1, 1]) + y[1, 2] * y[1, 2])


def offer_later_wins(ld, li, ls, k, d, i, s):
    """instances_knn_ref._offer with ties resolved by the later candidate: it goes in front of its equals, and displaces an equal bound"""
    full = len(ld) == k
    if full and not d <= ld[-1]:
        return False
    if full:
        ld.pop(); li.pop(); ls.pop()
    pos = len(ld)
    for j, e in enumerate(ld):
        if d <= e:
            pos = j
            break
    ld.insert(pos, d); li.insert(pos, i); ls.insert(pos, s)
    return True


class SceneRenormalised(ir.Scene):
    def object_rays(self, rays, i):
        out = super().object_rays(rays, i)
        with np.errstate(all="ignore"):
            out["d"] = (out["d"] / np.sqrt((out["d"].astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(self.ft)
            out["inv"] = self.ft(1) / out["d"]
        return out


class SceneWorldInverse(ir.Scene):
    def object_rays(self, rays, i):
        out = super().object_rays(rays, i)
        out["inv"] = rays["inv"]
        return out


_true = dict(inverse=ir.inverse, world_boxes=ir.world_boxes, join_min=ir._join_min, join_max=ir._join_max, stretch=iwr.stretch,
             offer=iknn._offer)


def _rebuilt(c, cls=ir.Scene):
    return cls(c["trees"], c["tree_of"], c["x"], c["dtype"])


def _first_seed(seeds, differs):
    for s in seeds:
        if differs(fi.case(s)):
            return s
    return None


def test_mutations_of_the_definition_are_seen(monkeypatch):
    seen = {}
    nr = lambda c: len(c["rays"])     # noqa: E731
    # the copy is the reference: unmutated it gives the reference's answers
    c = fi.case(1)
    assert _same_hits(select(c["free"]["table"], nr(c), c["tmax"], c["dtype"]), c["cut"]["closest"])
    assert _same_hits(select(c["free"]["table"], nr(c), c["tmax"], c["dtype"], first=True), c["cut"]["first"])
    assert _same_hits(_rebuilt(c).trace(c["rays"])["closest"], c["free"]["closest"])

    lattice_first = _of_kind("lattice") + [s for s in SEEDS if _kind(s) != "lattice"]
    seen["<= in the closest rule"] = _first_seed(lattice_first, lambda c: not _same_hits(
        select(c["free"]["table"], nr(c), None, c["dtype"], closest_le=True), c["free"]["closest"]))
    seen["<= against tmax"] = _first_seed(SEEDS, lambda c: not _same_hits(
        select(c["free"]["table"], nr(c), c["tmax"], c["dtype"], tmax_le=True), c["cut"]["closest"]))

    def sorted_rows_differ(c):
        _, inst, shape, _ = hit_rows(c)
        minst, mshape = rows_reversing_ties(c["free"]["table"], nr(c), c["dtype"])
        return inst.tobytes() != minst.tobytes() or shape.tobytes() != mshape.tobytes()
    seen["all-hits sort reverses equal keys"] = _first_seed(lattice_first, sorted_rows_differ)

    def within_sort_differs(c):
        rows = c["within"]
        rev = [[e for _, e in sorted(enumerate(r), key=lambda t: (t[1][0], -t[0]))] for r in rows]
        return [sorted(r, key=lambda e: e[0]) for r in rows] != rev
    seen["within sort reverses equal keys"] = _first_seed(lattice_first, within_sort_differs)

    def with_patch(module, name, value, differs, seeds):
        monkeypatch.setattr(module, name, value)
        try:
            return _first_seed(seeds, differs)
        finally:
            monkeypatch.setattr(module, name, _true[{"_offer": "offer", "_join_min": "join_min", "_join_max": "join_max"}.get(name, name)])

    def knn_differs(c):
        return not iknn.same_rows(iknn.rows(c["scene"], c["points"], c["ks"][1]), c["knn"][c["ks"][1]])
    seen["ties resolved by the later candidate"] = with_patch(iknn, "_offer", offer_later_wins, knn_differs, lattice_first)

    def closest_differs(cls=ir.Scene):
        return lambda c: not _same_hits(_rebuilt(c, cls).trace(c["rays"])["closest"], c["free"]["closest"])
    ordinary = _of_kind("posed", "scaled") + _of_kind("degenerate", "lattice")
    seen["y[k][3] summed as a + (b + c)"] = with_patch(ir, "inverse", inverse_other_association, closest_differs(), ordinary)
    seen["world box from 2 corners"] = with_patch(ir, "world_boxes", world_boxes_two_corners,
                                                  lambda c: _rebuilt(c).w.tobytes() != c["scene"].w.tobytes(), ordinary)

    def zeros_differ(c):
        monkeypatch.setattr(ir, "_join_max", lambda a, axis=0: a.max(axis=axis))
        try:
            return _rebuilt(c).w.tobytes() != c["scene"].w.tobytes()
        finally:
            monkeypatch.setattr(ir, "_join_max", _true["join_max"])
    seen["-0 / +0 order dropped from the joins"] = with_patch(ir, "_join_min", lambda a, axis=0: a.min(axis=axis), zeros_differ, lattice_first)

    def within_differs(c):
        return iwr.rows(c["scene"], c["points"], c["limits"]) != c["within"]
    seen["F without its third row"] = with_patch(iwr, "stretch", stretch_two_rows, within_differs, ordinary)
    seen["d' renormalised"] = _first_seed(ordinary, closest_differs(SceneRenormalised))
    seen["inv' taken from the world ray"] = _first_seed(ordinary, closest_differs(SceneWorldInverse))

    print("mutation → the first default seed that sees it:", {k: (None if v is None else fi.label(v)) for k, v in seen.items()})
    for name, s in seen.items():
        assert s is not None, f"no default seed sees the mutation: {name} (the others, by first seed: {seen})"
    # and the references are whole again
    assert ir.inverse is _true["inverse"] and ir.world_boxes is _true["world_boxes"] and iwr.stretch is _true["stretch"]
    assert iknn._offer is _true["offer"] and ir._join_min is _true["join_min"] and ir._join_max is _true["join_max"]
