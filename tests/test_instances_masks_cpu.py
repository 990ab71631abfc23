"""Per-instance visibility masks, CPU side: the masks and scenes tests/test_gpu_instances_masks.py runs, shown on the reference alone
(tests/instances_masks_ref.py over tests/instances_ref.py's candidate table) to exercise what a mask can change — closest hits that move to
another pair, rays that become misses, rays that keep their pair, first hits that move, rows that shrink around k — so that a mask pattern
that exercises nothing cannot pass silently; the filtered definition against a brute force that never builds a table; the all-ones
identity; and the wiring of the new entries."""
import os

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_khits_ref as ikh
import instances_masks_ref as imr
from test_instances_cpu import N_RAYS, SIZES, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF
ALL = 0xFFFFFFFF
HIGH = 0x80000000
PAL = np.array([1, 2, 4, 8, 3, 0xC, HIGH, ALL, 0, 5], dtype=np.uint32)
KS = (1, 3, 9, 17, 64)


def inst_masks(n):
    """M[i] = 1 << (i % 4), the high bit too where i % 9 == 0; instance 5 hidden from every ray, instance 7 visible to every non-zero ray"""
    m = (np.uint32(1) << (np.arange(n, dtype=np.uint32) % 4)).astype(np.uint32)
    m[np.arange(n) % 9 == 0] |= np.uint32(HIGH)
    if n > 5:
        m[5] = 0
    if n > 7:
        m[7] = ALL
    return m


def ray_masks(n):
    return PAL[np.random.default_rng(500 + n).integers(0, 10, N_RAYS)]


_WANT = {}


def masked_want(orc, dtype, n, cut):
    """the masked reference answers of scene n (computed once, never modified): closest, first, all-hits sorted / list order, k-hits at KS"""
    key = (np.dtype(dtype).name, n, bool(cut))
    if key not in _WANT:
        c = case(orc, dtype, n)
        tm = c["tmax"] if cut else None
        t = imr.filter_table(c["free"]["table"], inst_masks(n), ray_masks(n))
        w = dict(table=t, closest=imr.select(t, N_RAYS, tm, dtype, False), first=imr.select(t, N_RAYS, tm, dtype, True),
                 sorted=iar.rows(t, N_RAYS, tm, dtype, True), listed=iar.rows(t, N_RAYS, tm, dtype, False))
        w["khits"] = {k: ikh.cut_rows(w["sorted"], N_RAYS, k, dtype) for k in KS}
        _WANT[key] = w
    return _WANT[key]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


def _pairs(sel):
    return sel[1].astype(np.int64) * (1 << 32) + sel[2]


def _figures(orc, dtype, n):
    c = case(orc, dtype, n)
    M, R = inst_masks(n), ray_masks(n)
    w = masked_want(orc, dtype, n, False)
    free = c["free"]
    hit = free["closest"][1] != NONE
    mhit = w["closest"][1] != NONE
    moved = hit & mhit & (_pairs(w["closest"]) != _pairs(free["closest"]))
    misses = hit & ~mhit
    kept = hit & mhit & (_pairs(w["closest"]) == _pairs(free["closest"]))
    first_vs_closest = mhit & (_pairs(w["first"]) != _pairs(w["closest"]))
    first_vs_first = mhit & (_pairs(w["first"]) != _pairs(free["first"]))    # (a first hit that moved, not one that went away)
    full = iar.rows(free["table"], N_RAYS, None, dtype, True)
    lf, lm = np.diff(full[0].astype(np.int64)), np.diff(w["sorted"][0].astype(np.int64))
    toff, tidx = free["top"]
    ray_of = np.repeat(np.arange(N_RAYS), np.diff(toff.astype(np.int64)))
    vis = (M[tidx.astype(np.int64)] & R[ray_of]) != 0
    visits, seen = np.bincount(ray_of, minlength=N_RAYS), np.bincount(ray_of[vis], minlength=N_RAYS)
    groups = sum(len(np.unique(R[g:g + 64])) > 1 for g in range(0, N_RAYS, 64))
    return dict(hit=int(hit.sum()), moved=int(moved.sum()), misses=int(misses.sum()), kept=int(kept.sum()),
                first_vs_closest=int(first_vs_closest.sum()), first_vs_first=int(first_vs_first.sum()),
                zero=int((hit & (R == 0)).sum()), high=int((mhit & (R == HIGH)).sum()),
                shortened=int(((lm < lf) & (lm > 0)).sum()), three=int((lm >= 3).sum()), longest=int(lm.max()), longest_free=int(lf.max()),
                partly=int(((seen > 0) & (seen < visits)).sum()), groups=groups, n_groups=(N_RAYS + 63) // 64,
                hits_kept=int(lm.sum()), hits=int(lf.sum()), lm=lm)


# ---- the masks exercise every way a mask can change an answer ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_are_worth_running(orc, dtype):
    """the 37-instance scene.  Figures of the reference, both dtypes alike: 1 086 rays hit unmasked; the masked closest hit is another pair
    for 235, 388 become misses, 463 keep their pair; masked first differs from masked closest for 259 and from unmasked first for 257; 106
    hitting rays carry mask 0; 62 rays with the high bit alone still hit; 460 rows shortened but not emptied, 222 with at least 3 hits left,
    the longest 9 (14 unmasked); 1 165 rays skip some but not all of their top-level visits; all 24 groups of 64 rays hold different
    masks; 1 585 of 4 104 hits kept."""
    f = _figures(orc, dtype, 37)
    print({k: v for k, v in f.items() if k != "lm"})
    for key in ("hit", "moved", "misses", "kept", "first_vs_closest", "first_vs_first", "zero"):
        assert f[key] >= 100, (key, f[key])
    assert f["zero"] >= 50 and f["high"] >= 30
    assert f["shortened"] >= 100 and f["three"] >= 100 and f["partly"] >= 100
    assert f["longest"] < f["longest_free"] and f["groups"] == f["n_groups"] == 24
    assert 0 < f["hits_kept"] < f["hits"]
    assert (f["hit"], f["moved"], f["misses"], f["kept"], f["first_vs_closest"], f["first_vs_first"], f["zero"], f["high"]) == \
        (1086, 235, 388, 463, 259, 257, 106, 62)
    assert (f["shortened"], f["three"], f["longest"], f["longest_free"], f["partly"], f["hits_kept"], f["hits"]) == (460, 222, 9, 14, 1165, 1585, 4104)
    lm = f["lm"]                                            # k = 3: rows shorter than, equal to and longer than k
    assert ((lm > 0) & (lm < 3)).sum() >= 10 and (lm == 3).sum() >= 10 and (lm > 3).sum() >= 10


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,misses,kept", [(2, 111, 39), (1, 70, 62)])
def test_small_scenes_are_worth_running(orc, dtype, n, misses, kept):
    f = _figures(orc, dtype, n)
    print({k: v for k, v in f.items() if k != "lm"})
    assert f["misses"] >= 30 and f["kept"] >= 30
    assert (f["misses"], f["kept"]) == (misses, kept)


def test_mask_layout():
    m = inst_masks(37)
    assert m.dtype == np.uint32 and m[5] == 0 and m[7] == ALL and m[0] == (1 | HIGH) and m[9] == (2 | HIGH) and m[6] == 4 and m[36] == (1 | HIGH)
    assert inst_masks(1).tolist() == [1 | HIGH] and inst_masks(2).tolist() == [1 | HIGH, 2]
    r = ray_masks(37)
    assert r.dtype == np.uint32 and len(r) == N_RAYS and set(np.unique(r).tolist()) == set(PAL.tolist())


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_filtered_table_is_the_brute_force(orc, dtype, n):
    """per ray, the visible instances of its top-level list in order, each walked alone: the rows, their order and their bits are the
    filtered table's; closest, first, the sorted rows and the k-hits rows follow from them by hand"""
    c = case(orc, dtype, n)
    M, R = inst_masks(n), ray_masks(n)
    for cut in (False, True):
        tmax = c["tmax"] if cut else None
        w = masked_want(orc, dtype, n, cut)
        bf = imr.brute_force(c["scene"], c["rays"], M, R, tmax, dtype)
        off, li, ls, lv = w["listed"]
        so, si, ss, sv = w["sorted"]
        some = 0
        for j in range(N_RAYS):
            row = bf[j]
            lo, hi = int(off[j]), int(off[j + 1])
            assert hi - lo == len(row), j
            assert [r[0] for r in row] == li[lo:hi].tolist() and [r[1] for r in row] == ls[lo:hi].tolist()
            assert b"".join(r[2].tobytes() for r in row) == lv[lo:hi].tobytes()
            some += bool(row)
            # closest: strict <, the earlier keeps a tie; first: the first of the row
            best = None
            for r in row:
                if best is None or r[2][0] < best[2][0]:
                    best = r
            cv, ci, cs = (x[j] for x in w["closest"])
            fv, fi, fs = (x[j] for x in w["first"])
            if best is None:
                assert ci == NONE and cs == NONE and np.isinf(cv[0]) and fi == NONE
            else:
                assert (ci, cs) == best[:2] and cv.tobytes() == best[2].tobytes()
                assert (fi, fs) == row[0][:2] and fv.tobytes() == row[0][2].tobytes()
            order = sorted(range(len(row)), key=lambda e: (row[e][2][0], e))
            assert [row[e][0] for e in order] == si[int(so[j]):int(so[j + 1])].tolist()
            assert [row[e][1] for e in order] == ss[int(so[j]):int(so[j + 1])].tolist()
            assert b"".join(row[e][2].tobytes() for e in order) == sv[int(so[j]):int(so[j + 1])].tobytes()
            ki, ks, kv = (x[j] for x in w["khits"][3])
            head = order[:3]
            assert ki[:len(head)].tolist() == [row[e][0] for e in head] and (ki[len(head):] == NONE).all() and (ks[len(head):] == NONE).all()
            assert kv[:len(head)].tobytes() == b"".join(row[e][2].tobytes() for e in head)
        assert cut or some >= 30                              # (uncut: the rays that keep their pair, at least)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_all_ones_is_the_unmasked_reference(orc, dtype, n):
    c = case(orc, dtype, n)
    ones = np.full(n, ALL, dtype=np.uint32)
    for tm, ref in ((None, c["free"]), (c["tmax"], c["cut"])):
        for rm in (None, ALL, np.full(N_RAYS, 1, dtype=np.uint32)):
            t = imr.filter_table(c["free"]["table"], ones, rm)
            assert all(t[k].tobytes() == np.ascontiguousarray(c["free"]["table"][k]).tobytes() for k in ("instance", "shape", "vals"))
            assert (t["cand_off"] == c["free"]["table"]["cand_off"]).all()
            for name, fn in (("closest", imr.closest), ("first", imr.first)):
                got = fn(c["free"]["table"], ones, rm, N_RAYS, tm, dtype)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref[name])), name
        for so in (True, False):
            got, want = imr.allhits(c["free"]["table"], ones, None, N_RAYS, tm, dtype, so), iar.rows(c["free"]["table"], N_RAYS, tm, dtype, so)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert ikh.same(imr.khits(c["free"]["table"], ones, None, N_RAYS, tm, 3, dtype), ikh.definition(c["free"]["table"], N_RAYS, tm, 3, dtype))
    # ... and a zero on either side hides everything
    for M, R in ((np.zeros(n, np.uint32), None), (ones, 0)):
        assert imr.filter_table(c["free"]["table"], M, R)["cand_off"][-1] == 0


# ---- wiring ---------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_built_and_bound():
    from bvh_amd import _lib, build_ext
    from bvh_amd.instances import Instances, InstancesMasks
    for src in ("instances.hip", "instances_allhits.hip", "instances_khits.hip"):
        assert src in build_ext.SOURCES
        text = open(os.path.join(ROOT, "bvh_amd", "csrc", src)).read()
        assert "bool MASKED" in text and "if constexpr (MASKED)" in text, src
    sig = {s[0]: s for s in _lib.SYMBOLS}
    for name, n_args in (("set_masks", 4), ("masks", 3), ("trace_masked_f32", 10), ("trace_masked_f64", 10), ("khits_masked_f32", 10),
                         ("khits_masked_f64", 10), ("allhits_masked_f32", 8), ("allhits_masked_f64", 8)):
        assert len(sig["bvhgpu_instances_" + name][2]) == n_args and sig["bvhgpu_instances_" + name][1] is not None, name
    assert _lib.ABI_VERSION == 7
    assert issubclass(Instances, InstancesMasks)
    assert {k for k in vars(InstancesMasks) if not k.startswith("_")} == {
        "set_masks", "masks", "closest_hits_masked", "any_hits_masked", "occluded_masked", "khits_masked_batch", "allhits_masked_batch"}
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    for name in ("set_masks", "masks", "trace_masked_f32", "khits_masked_f64", "allhits_masked_f32"):
        assert f"int bvhgpu_instances_{name}(" in header, name
    assert "#define BVHGPU_ABI_VERSION 7" in header


def test_the_library_holds_the_masked_kernels():
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    # (Itanium mangling: ...ILb<first>ELb<masked>E... — the masked instantiations are there beside the unmasked ones)
    for kern in (b"k_instances_traceIfLb0ELb1E", b"k_instances_traceIdLb1ELb1E", b"k_instances_traceIfLb0ELb0E", b"k_instances_khitsIfLb1E",
                 b"k_instances_khitsIdLb0E", b"k_instances_allhits_countIfLb1E", b"k_instances_allhits_fillIdLb1ELb1E",
                 b"k_instances_allhits_fillIfLb0ELb1E"):
        assert kern in blob, kern
