"""Visibility masks for the point and region queries over instanced scenes, CPU side: the masks and scenes
tests/test_gpu_instances_point_masks.py runs, shown on the references alone (tests/instances_point_masks_ref.py) to exercise what a mask
can change in each family — so that a mask pattern that exercises nothing cannot pass silently; each reference against a brute force that
builds no tree, row for row with order; the all-ones identity; and the wiring of the new entries.
The instance masks are tests/test_instances_masks_cpu.py's (M[i] = 1 << (i % 4), the high bit where i % 9 == 0, M[5] = 0, M[7] = all ones);
row masks are drawn from its palette."""
import os

import numpy as np
import pytest

import instances_knn_ref as ikr
import instances_knn_tree_ref as iktr
import instances_point_masks_ref as ipm
import instances_ref as ir
import instances_region_ref as irr
import instances_within_ref as iwr
from test_instances_cpu import SIZES
from test_instances_knn_cpu import cluster
from test_instances_masks_cpu import ALL, HIGH, PAL, inst_masks
from test_instances_within_cpu import cluster_rows as within_cluster_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF
N_POINTS = 600          # what the GPU test runs
N_CPU = 200             # what the brute forces are run on
KS = (1, 3, 9, 17, 64)  # every block size of the list kernels
K_FIG = 3               # the k the figures are read at
FLOOR = 20


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


def point_masks(n_instances, count=N_POINTS):
    """the row masks of the cluster scene of n_instances instances: the palette, drawn with seed 700 + n_instances"""
    return PAL[np.random.default_rng(700 + n_instances).integers(0, 10, N_POINTS)][:count]


def region_masks(n_regions):
    """the row masks of instances_region_ref.main_scene's regions: the palette drawn with seed 752, then every second of the first 44
    regions 0 — the draw alone empties about 5 of the 52 regions, the floor asks for 20"""
    p = PAL[np.random.default_rng(752).integers(0, 10, n_regions)].copy()
    p[0:44:2] = 0
    return p


# ---- the line of instances: ties at the cut ------------------------------------------------------------------------------------------------
LINE_N = 60
LINE_TIES = {1: 31, 3: 31}   # rows of the line scene with a visible / hidden tie at the cut, per k (read off the reference)


def line_points(dtype):
    """60 points ON the triangles at x = 3 .. 62 of instances_within_ref.line_instances: instance 0 and its coincident copy 64 both hold
    each of them, so every distance appears twice there.  M[0] = 1 | HIGH and M[64] = 1: the row mask HIGH — every second row; the others
    drawn — sees instance 0 and not its copy, and a cut at an odd k runs through such a twin"""
    pts = np.zeros((LINE_N, 3), dtype=dtype)
    pts[:, 0] = np.arange(3, 3 + LINE_N)
    p = PAL[np.random.default_rng(764).integers(0, 10, LINE_N)].copy()
    p[::2] = HIGH
    return pts, p


_LINE = {}


def line_case(dtype):
    key = np.dtype(dtype).name
    if key not in _LINE:
        trees, tree_of, x = iwr.line_instances(dtype)
        sc = ir.Scene(trees, tree_of, x, dtype)
        pts, P = line_points(dtype)
        _LINE[key] = dict(trees=trees, tree_of=tree_of, x=x, scene=sc, points=pts, P=P, M=inst_masks(len(x)), cache={})
    return _LINE[key]


def _tie_at_cut(full_sorted, vis_row, k):
    """the stable ascending list of ALL pairs has equal distances at positions k - 1 and k, and the pairs at that distance include a
    visible and a hidden one"""
    if len(full_sorted) <= k or full_sorted[k - 1][0] != full_sorted[k][0]:
        return False
    d = full_sorted[k][0]
    v = [bool(vis_row[e[1]]) for e in full_sorted if e[0] == d]
    return any(v) and not all(v)


# ---- within --------------------------------------------------------------------------------------------------------------------------------
_WITHIN = {}


def within_want(orc, dtype, n):
    """(scene case, points, limits, unmasked rows, masked rows, M, P) — computed once, never modified"""
    key = (np.dtype(dtype).name, n)
    if key not in _WITHIN:
        c, pts, m, rows, _ = within_cluster_rows(orc, dtype, n)
        M, P = inst_masks(n), point_masks(n)
        _WITHIN[key] = (c, pts, m, rows, ipm.within_filter(rows, M, P), M, P)
    return _WITHIN[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_within_rows_equal_brute_force(orc, dtype, n):
    c, pts, m, rows, masked, M, P = within_want(orc, dtype, n)
    want = ipm.within_brute(c["scene"], pts, m, M, P)
    for j in range(N_POINTS):
        assert set((i, s) for _, i, s in masked[j]) == want[j], j
        # the order and the distances are the unmasked row's: a subsequence of it
        it = iter(rows[j])
        assert all(any(e == f for f in it) for e in masked[j]), j
    ones = ipm.within_filter(rows, np.full(n, ALL, np.uint32), None)
    assert ones == rows
    assert all(r == [] for r in ipm.within_filter(rows, np.zeros(n, np.uint32), None)) and all(r == [] for r in ipm.within_filter(rows, M, 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_masks_are_worth_running(orc, dtype):
    """the 37-instance scene, both dtypes alike: of the 267 rows that are not empty unmasked, 105 are shortened but not emptied, 87 are
    emptied and 75 keep every pair"""
    _, _, _, rows, masked, _, _ = within_want(orc, dtype, 37)
    lf, lm = np.array([len(r) for r in rows]), np.array([len(r) for r in masked])
    shortened, emptied, unchanged = int(((lm < lf) & (lm > 0)).sum()), int(((lf > 0) & (lm == 0)).sum()), int(((lf > 0) & (lm == lf)).sum())
    print(shortened, emptied, unchanged, int(lm.max()), int(lm.sum()))
    assert min(shortened, emptied, unchanged) >= FLOOR
    assert (shortened, emptied, unchanged) == (105, 87, 75)


# ---- knearest ------------------------------------------------------------------------------------------------------------------------------
_KNN = {}


def knn_want(orc, dtype, n, k, count=N_POINTS):
    """the masked reference rows of the flat form for the first `count` cluster points (computed once, never modified)"""
    key = (np.dtype(dtype).name, n, k, count)
    if key not in _KNN:
        c, pts, cache = cluster(orc, dtype, n)
        _KNN[key] = ipm.knn_rows(c["scene"], pts[:count], k, inst_masks(n), point_masks(n, count), cache)
    return _KNN[key]


def _replaced(free, masked, vis):
    """rows where a hidden pair was among the unmasked nearest k and a visible pair that the unmasked row does not hold takes a slot"""
    out = 0
    for j, (rf, rm) in enumerate(zip(free, masked)):
        hidden = any(not vis[j, i] for _, i, _ in rf)
        have = set((i, s) for _, i, s in rf)
        out += hidden and any((i, s) not in have for _, i, s in rm)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", (1, K_FIG, 64))
def test_knearest_rows_equal_brute_force(orc, dtype, n, k):
    c, pts, cache = cluster(orc, dtype, n)
    M, P = inst_masks(n), point_masks(n, N_CPU)
    rows = knn_want(orc, dtype, n, k, N_CPU)
    want = ipm.knn_brute(c["scene"], pts[:N_CPU], k, M, P, cache)
    bad = [j for j in range(N_CPU) if rows[j] != want[j]]
    assert not bad, (bad[:5], rows[bad[0]][:3], want[bad[0]][:3])
    ones = ipm.knn_rows(c["scene"], pts[:N_CPU], k, np.full(n, ALL, np.uint32), None, cache)
    assert ones == ikr.rows(c["scene"], pts[:N_CPU], k, None, cache)
    assert all(r == [] for r in ipm.knn_rows(c["scene"], pts[:20], k, M, 0, cache))


@pytest.mark.parametrize("dtype", DTYPES)
def test_knearest_masks_are_worth_running(orc, dtype):
    """37 instances, k = 3, the first 200 points: in 105 rows a hidden pair was among the unmasked nearest 3 and a farther visible pair takes
    its place — what a filter after the fact gets wrong.  The line of instances: 31 rows with a tie at the cut (k = 1 and k = 3 alike) between a
    visible and a hidden pair"""
    c, pts, cache = cluster(orc, dtype, 37)
    M, P = inst_masks(37), point_masks(37, N_CPU)
    vis = ipm._vis(M, P, N_CPU)
    free = ikr.rows(c["scene"], pts[:N_CPU], K_FIG, None, cache)
    replaced = _replaced(free, knn_want(orc, dtype, 37, K_FIG, N_CPU), vis)
    print("replaced", replaced)
    assert replaced >= FLOOR and replaced == 105
    L = line_case(dtype)
    sc, lp = L["scene"], L["points"]
    vis = ipm._vis(L["M"], L["P"], LINE_N)
    full = ikr.brute(sc, lp, 66 * 64, L["cache"])             # every pair, stable ascending
    for k in (1, 3):
        ties = sum(_tie_at_cut(full[j], vis[j], k) for j in range(LINE_N))
        print("ties", k, ties)
        assert ties >= FLOOR and ties == LINE_TIES[k], (k, ties)
        rows = ipm.knn_rows(sc, lp, k, L["M"], L["P"], L["cache"])
        assert rows == ipm.knn_brute(sc, lp, k, L["M"], L["P"], L["cache"])
        for j in range(0, LINE_N, 2):                         # the row mask HIGH: instance 0's twin, never its hidden copy's
            assert rows[j][0][0] == 0.0 and all(i != 64 for _, i, _ in rows[j]) and rows[j][0][1] == 0


# ---- knearest_tree -------------------------------------------------------------------------------------------------------------------------
LIMITS = ("none", "scalar", "drawn", "special")
_KNT = {}


def limits_of(kind, dtype, n_instances, count=N_POINTS):
    """none: no limit; scalar: 2.5 for every point; drawn: instances_within_ref.cluster_points' own limits; special: 0, negative, NaN, +inf
    and 2.5 in turn"""
    if kind == "none":
        return None
    if kind == "scalar":
        return 2.5
    if kind == "drawn":
        return np.ascontiguousarray(iwr.cluster_points(n_instances, dtype, N_POINTS)[1][:count])
    return iktr.special_limits(count, dtype)


def knt_want(orc, dtype, n, k, kind, count=N_POINTS):
    """the masked reference rows of the tree form (computed once, never modified)"""
    key = (np.dtype(dtype).name, n, k, kind, count)
    if key not in _KNT:
        c, pts, cache = cluster(orc, dtype, n)
        _KNT[key] = ipm.knn_tree_rows(c["scene"], pts[:count], k, inst_masks(n), point_masks(n, count), limits_of(kind, dtype, n, count), cache)
    return _KNT[key]


@pytest.mark.parametrize("kind", LIMITS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", (1, K_FIG, 64))
def test_knearest_tree_rows_equal_ordered_brute(orc, dtype, n, k, kind):
    c, pts, cache = cluster(orc, dtype, n)
    M, P = inst_masks(n), point_masks(n, N_CPU)
    lim = limits_of(kind, dtype, n, N_CPU)
    rows = knt_want(orc, dtype, n, k, kind, N_CPU)
    want = ipm.knn_tree_brute(c["scene"], pts[:N_CPU], k, M, P, lim, cache)
    bad = [j for j in range(N_CPU) if rows[j] != want[j]]
    assert not bad, (bad[:5], rows[bad[0]][:3], want[bad[0]][:3])
    if kind == "none":                                        # the distances are the flat form's (the pairs may differ at ties)
        flat = knn_want(orc, dtype, n, k, N_CPU)
        assert [[e[0] for e in r] for r in rows] == [[e[0] for e in r] for r in flat]
    ones = ipm.knn_tree_rows(c["scene"], pts[:N_CPU], k, np.full(n, ALL, np.uint32), None, lim, cache)
    assert ones == iktr.rows(c["scene"], pts[:N_CPU], k, lim, None, cache)


@pytest.mark.parametrize("dtype", DTYPES)
def test_knearest_tree_masks_are_worth_running(orc, dtype):
    """37 instances, k = 3, 200 points: 105 rows where a farther visible pair replaces a hidden one; with the drawn limits 27 rows whose limit
    admits hidden pairs only, so the row is all padding; the line of instances: 31 rows with a visible / hidden tie at the cut"""
    c, pts, cache = cluster(orc, dtype, 37)
    M, P = inst_masks(37), point_masks(37, N_CPU)
    vis = ipm._vis(M, P, N_CPU)
    free = iktr.rows(c["scene"], pts[:N_CPU], K_FIG, None, None, cache)
    replaced = _replaced(free, knt_want(orc, dtype, 37, K_FIG, "none", N_CPU), vis)
    lim = limits_of("drawn", dtype, 37, N_CPU)
    free_l = iktr.rows(c["scene"], pts[:N_CPU], 64, lim, None, cache)
    masked_l = knt_want(orc, dtype, 37, K_FIG, "drawn", N_CPU)
    hidden_only = sum(1 for j in range(N_CPU) if free_l[j] and not masked_l[j])
    assert all(not vis[j, i] for j in range(N_CPU) if free_l[j] and not masked_l[j] for _, i, _ in free_l[j])
    print("replaced", replaced, "hidden only", hidden_only)
    assert replaced >= FLOOR and hidden_only >= FLOOR
    assert (replaced, hidden_only) == (105, 27)
    L = line_case(dtype)
    sc, lp = L["scene"], L["points"]
    vis = ipm._vis(L["M"], L["P"], LINE_N)
    full = ikr.brute(sc, lp, 66 * 64, L["cache"])
    for k in (1, 3):
        ties = sum(_tie_at_cut(full[j], vis[j], k) for j in range(LINE_N))
        assert ties >= FLOOR and ties == LINE_TIES[k], (k, ties)
        rows = ipm.knn_tree_rows(sc, lp, k, L["M"], L["P"], None, L["cache"])
        assert rows == ipm.knn_tree_brute(sc, lp, k, L["M"], L["P"], None, L["cache"])
        assert [[e[0] for e in r] for r in rows] == [[e[0] for e in r] for r in ipm.knn_rows(sc, lp, k, L["M"], L["P"], L["cache"])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("member", "top"))
def test_split_without_sah_winner(orc, dtype, which):
    """far_member_scene / coincident_scene: empty child boxes on either level; the masked descent is the ordered brute force there too"""
    sc, _, x, pts = iktr.far_member_scene(dtype) if which == "member" else iktr.coincident_scene(dtype)
    M = inst_masks(len(x))
    P = PAL[np.random.default_rng(770).integers(0, 10, len(pts))]
    cache = {}
    some = 0
    for k in (1, 7):
        rows = ipm.knn_tree_rows(sc, pts, k, M, P, None, cache)
        assert rows == ipm.knn_tree_brute(sc, pts, k, M, P, None, cache)
        some += sum(1 for r in rows if r)
    assert some >= FLOOR


# ---- region --------------------------------------------------------------------------------------------------------------------------------
_REGION = {}


def region_want(dtype):
    """(main scene, M, P, the filtered reference) — computed once, never modified"""
    key = np.dtype(dtype).name
    if key not in _REGION:
        m = irr.main_scene(dtype)
        M, P = inst_masks(len(m["x"])), region_masks(len(m["planes"]))
        _REGION[key] = (m, M, P, ipm.region_filter(m["ref"], M, P))
    return _REGION[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_rows_equal_brute_force(dtype):
    m, M, P, w = region_want(dtype)
    bf = ipm.region_brute(m["scene"], m["planes"], M, P)
    toff, tinst, tins = w["top"]
    foff, finst, fshape, fins = w["full"]
    for q, row in enumerate(bf):
        lo, hi = int(toff[q]), int(toff[q + 1])
        assert [r[0] for r in row] == tinst[lo:hi].tolist() and [r[1] for r in row] == tins[lo:hi].tolist(), q
        lo, hi = int(foff[q]), int(foff[q + 1])
        assert [r[0] for r in row for _ in r[2]] == finst[lo:hi].tolist(), q
        assert [s for r in row for s, _ in r[2]] == fshape[lo:hi].tolist() and [b for r in row for _, b in r[2]] == fins[lo:hi].tolist(), q
    ones = ipm.region_filter(m["ref"], np.full(len(M), ALL, np.uint32), None)
    for name in ("top", "full"):
        assert all(a.tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(ones[name], m["ref"][name])), name
    assert ipm.region_filter(m["ref"], M, 0)["full"][0][-1] == 0 and ipm.region_filter(m["ref"], np.zeros(len(M), np.uint32), None)["top"][0][-1] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_masks_are_worth_running(dtype):
    """the main scene's 52 regions, both dtypes alike: I_q loses some but not all of its instances in 25 regions and is emptied in 25 (all
    52 are non-empty unmasked) — these are the INSTANCES_ONLY rows; 46 of the 133 pairs of I_q with inside = 1 survive, and 150 587 of the
    495 903 (instance, shape) pairs with inside = 1.  Of the 39 (instance, shape) rows that hold pairs unmasked, 18 lose some but not all
    and 19 are emptied (read off and asserted, no floor: 39 rows cannot give 20 of each)"""
    m, M, P, w = region_want(dtype)
    f = {}
    for name in ("top", "full"):
        lf = np.diff(m["ref"][name][0].astype(np.int64))
        lm = np.diff(w[name][0].astype(np.int64))
        f[name] = (int(((lm < lf) & (lm > 0)).sum()), int(((lf > 0) & (lm == 0)).sum()), int(w[name][-1].sum()))
    print(f)
    assert min(f["top"]) >= FLOOR and f["full"][2] >= FLOOR, f
    assert f == {"top": (25, 25, 46), "full": (18, 19, 150587)}


# ---- wiring ---------------------------------------------------------------------------------------------------------------------------------
NEW = (("within_masked", 8), ("knearest_masked", 9), ("knearest_tree_masked", 10), ("region_masked", 8))


def test_the_new_entries_are_built_and_bound():
    from bvh_amd import _lib, build_ext
    from bvh_amd.instances import Instances, InstancesMaskedQueries
    for src in ("instances_within.hip", "instances_knn.hip", "instances_knn_tree.hip", "region.hip"):
        assert src in build_ext.SOURCES
        text = open(os.path.join(ROOT, "bvh_amd", "csrc", src)).read()
        assert "bool MASKED = false" in text and "if constexpr (MASKED)" in text, src
    assert "struct InstMasks" in open(os.path.join(ROOT, "bvh_amd", "csrc", "instances.hpp")).read()
    sig = {s[0]: s for s in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    for name, n_args in NEW:
        for sfx in ("f32", "f64"):
            full = f"bvhgpu_instances_{name}_{sfx}"
            assert len(sig[full][2]) == n_args and sig[full][1] is not None, full
            assert len(sig[full][2]) == len(sig[full.replace("_masked", "")][2]) + 1
            assert f"int {full}(" in header and f"pub fn {full}(" in ffi, full
    assert _lib.ABI_VERSION == 7 and "#define BVHGPU_ABI_VERSION 7" in header
    assert issubclass(Instances, InstancesMaskedQueries)
    assert {k for k in vars(InstancesMaskedQueries) if not k.startswith("_")} == {
        "within_masked_batch", "knearest_masked_batch", "nearest_masked_batch", "knearest_tree_masked_batch", "nearest_tree_masked_batch",
        "region_masked_batch"}


def test_the_library_holds_the_masked_kernels():
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    # (Itanium mangling: ...Lb<masked>E — the masked instantiations are there beside the unmasked ones)
    for kern in (b"k_instances_within_countIfLb1E", b"k_instances_within_countIdLb0E", b"k_instances_within_fillIfLb1ELb1E",
                 b"k_instances_within_fillIdLb0ELb1E", b"k_instances_within_fillIfLb1ELb0E", b"k_instances_knearestIfLb1E",
                 b"k_instances_knearestIdLb1E", b"k_instances_knearestIfLb0E", b"k_instances_knearest_treeIfLb1E",
                 b"k_instances_knearest_treeIdLb1E", b"k_instances_knearest_treeIdLb0E", b"k_instances_region_walkIfLb0ELb0ELb1E",
                 b"k_instances_region_walkIdLb0ELb0ELb1E", b"k_instances_region_walkIfLb1ELb0ELb0E", b"k_instances_region_walkIfLb1ELb1ELb0E",
                 b"k_instances_region_visible", b"k_instances_region_keep"):
        assert kern in blob, kern
