"""k-hits over instanced scenes, CPU side: the inputs tests/test_gpu_instances_khits.py runs, shown on the reference alone
(tests/instances_khits_ref.py) to be worth running — the definition (the sorted all-hits rows cut to k) and the incremental list the
kernel runs agree byte for byte; k = 1 is `closest`; rows shorter than, equal to and longer than k occur for every k; ties straddle the
cut at every odd k and lie inside the row at every even k — and the wiring of the new HIP file into the build."""
import os

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_khits_ref as ikh
from test_instances_allhits_cpu import N_STACK_RAYS, cluster_rows, reachable, stack_case
from test_instances_cpu import N_RAYS, SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF
# both sides of every block-size boundary (f32: 10 | 11 and 21 | 22; f64: 8 | 9 and 16 | 17), and the ends
K = (1, 2, 3, 8, 9, 10, 11, 16, 17, 21, 22, 63, 64)
N_TIE_RAYS = 16


def block_lds(k, dtype):
    """the block rule of bvh_amd/csrc/instances_khits.hip → (lanes, bytes of LDS)"""
    per_lane = k * (np.dtype(dtype).itemsize + 8)
    lanes = 256 if 256 * per_lane <= 32 * 1024 else 128 if 128 * per_lane <= 32 * 1024 else 64
    return lanes, lanes * per_lane


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the cluster scene ---------------------------------------------------------------------------------------------------------------------
def cluster_want(orc, dtype, n, cut, k):
    """the definition's rows of case(orc, dtype, n), free or cut, from the all-hits rows that test file keeps"""
    return ikh.cut_rows(cluster_rows(orc, dtype, n)[1][(cut, True)], N_RAYS, k, dtype)


# ---- the stack scene with 16 more rays in front of coincident copies -------------------------------------------------------------------------
_TIES = {}


def tie_case(orc, dtype):
    """16 rays along +z with x, y in U(-0.3, 0.3): eight from z = 299, in front of the coincident copies 30 / 31, eight from z = 209, in front
    of 21 / 22.  Every distance is exact and appears twice, once per copy.  → dict(rays, table, uncut, uncut_list) (computed once)"""
    key = np.dtype(dtype).name
    if key not in _TIES:
        s = stack_case(orc, dtype)
        xy = np.random.default_rng(11).uniform(-0.3, 0.3, size=(N_TIE_RAYS, 2))
        o = np.zeros((N_TIE_RAYS, 3)); d = np.zeros((N_TIE_RAYS, 3))
        o[:, :2] = xy
        o[:8, 2], o[8:, 2], d[:, 2] = 299.0, 209.0, 1.0
        rays = orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)
        table = s["scene"].trace(rays)["table"]
        _TIES[key] = dict(rays=rays, table=table, uncut=iar.rows(table, N_TIE_RAYS, None, dtype, True),
                          uncut_list=iar.rows(table, N_TIE_RAYS, None, dtype, False))
    return _TIES[key]


_PLANS = {}


def stack_plan(orc, dtype, k):
    """the stack scene's own 72 rays with tmax[j] = the L-th smallest distance of ray j's uncut row, L cycling through 0, 1, k - 1, k, k + 1
    and uncut (an L at which a tie pair straddles the cut is skipped), then the 16 tie rays uncut.
    → dict(rays[88], tmax[88], plan[72], lens[88] = the candidates per ray, want = the definition's rows) (computed once, never modified)"""
    key = (np.dtype(dtype).name, k)
    if key not in _PLANS:
        s, t = stack_case(orc, dtype), tie_case(orc, dtype)
        n = len(s["rays"])
        targets = [0, 1, k - 1, k, k + 1, None]
        off, _, _, vals = s["uncut"]
        tmax = np.full(n, np.inf, dtype=dtype)
        plan = [None] * n
        for j in range(n):
            for step in range(len(targets)):
                L = targets[(j + step) % len(targets)]
                if L is None:
                    break
                if reachable(s, j, L):
                    tmax[j], plan[j] = vals[off[j] + L, 0], L
                    break
        cut = iar.rows(s["table"], n, tmax, dtype, True)
        main, ties = ikh.cut_rows(cut, n, k, dtype), ikh.cut_rows(t["uncut"], N_TIE_RAYS, k, dtype)
        _PLANS[key] = dict(rays=np.concatenate([s["rays"], t["rays"]]), tmax=np.concatenate([tmax, np.full(N_TIE_RAYS, np.inf, dtype=dtype)]),
                           plan=plan, lens=np.concatenate([np.diff(cut[0].astype(np.int64)), np.diff(t["uncut"][0].astype(np.int64))]),
                           want=tuple(np.concatenate([a, b]) for a, b in zip(main, ties)))
    return _PLANS[key]


# ---- 1. the two forms agree ------------------------------------------------------------------------------------------------------------------
def test_the_k_values_sit_on_both_sides_of_every_block_size():
    for dtype, edges in ((np.float32, (10, 21)), (np.float64, (8, 16))):
        assert [block_lds(k, dtype)[0] for k in (edges[0], edges[0] + 1, edges[1], edges[1] + 1)] == [256, 128, 128, 64]
        assert all(e in K and e + 1 in K for e in edges)
    assert block_lds(64, np.float64) == (64, 65536) and block_lds(64, np.float32) == (64, 49152) and K[0] == 1 and K[-1] == 64


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_agree_on_the_cluster_scene(orc, dtype, n):
    c, _ = cluster_rows(orc, dtype, n)
    table = c["free"]["table"]
    for cut in (False, True):
        for k in K:
            assert ikh.same(ikh.incremental(table, N_RAYS, c["tmax"] if cut else None, k, dtype), cluster_want(orc, dtype, n, cut, k)), (cut, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_agree_on_the_stack_scene(orc, dtype):
    s, t = stack_case(orc, dtype), tie_case(orc, dtype)
    n = len(s["rays"])
    for k in K:
        p = stack_plan(orc, dtype, k)
        main = ikh.incremental(s["table"], n, p["tmax"][:n], k, dtype)
        ties = ikh.incremental(t["table"], N_TIE_RAYS, None, k, dtype)
        assert ikh.same(tuple(np.concatenate([a, b]) for a, b in zip(main, ties)), p["want"]), k
        assert ikh.same(ikh.definition(t["table"], N_TIE_RAYS, None, k, dtype), tuple(w[n:] for w in p["want"])), k


# ---- 2. consequences -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_consequences_hold_on_the_reference(orc, dtype, n):
    """k = 1 is `closest` on every ray, free and cut; the row in front of its padding is the head of the sorted all-hits row"""
    c, rows_ = cluster_rows(orc, dtype, n)
    table = c["free"]["table"]
    for cut in (False, True):
        tm = c["tmax"] if cut else None
        want = (c["cut"] if cut else c["free"])["closest"]
        oi, os_, ov = ikh.incremental(table, N_RAYS, tm, 1, dtype)
        assert ov[:, 0].tobytes() == want[0].tobytes() and oi[:, 0].tobytes() == want[1].tobytes() and os_[:, 0].tobytes() == want[2].tobytes(), cut
        off, inst, shape, vals = rows_[(cut, True)]
        for k in (3, 8):
            oi, os_, ov = ikh.incremental(table, N_RAYS, tm, k, dtype)
            filled = os_ != NONE
            for j in range(N_RAYS):
                lo = int(off[j])
                m = min(k, int(off[j + 1]) - lo)
                assert filled[j].sum() == m and filled[j, :m].all()
                assert oi[j, :m].tobytes() == inst[lo:lo + m].tobytes() and os_[j, :m].tobytes() == shape[lo:lo + m].tobytes()
                assert ov[j, :m].tobytes() == vals[lo:lo + m].tobytes()
    lens = np.diff(rows_[(False, True)][0].astype(np.int64))
    assert n < 37 or ((lens >= 2).sum() >= 20 and (lens == 0).sum() >= 20)        # rows with and without padding at small k


# ---- 3. row lengths around k -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lengths_around_every_k(orc, dtype):
    s = stack_case(orc, dtype)
    uncut = np.diff(s["uncut"][0].astype(np.int64))
    lo = s["uncut_list"]
    # the list-order row of every main ray is not ascending: the insertion has to move elements
    assert all((np.diff(lo[3][lo[0][j]:lo[0][j + 1], 0]) < 0).any() for j in range(N_STACK_RAYS))
    for k in K:
        p = stack_plan(orc, dtype, k)
        n = len(s["rays"])
        lens = p["lens"][:n]
        for j, L in enumerate(p["plan"]):
            assert lens[j] == (uncut[j] if L is None else L), (k, j, L)
        have = set(lens.tolist())
        for L in {0, 1, k - 1, k, k + 1}:
            assert L in have, (k, L)
        assert any(L is None for L in p["plan"]) and lens.max() > 64
        filled = (p["want"][1] != NONE).sum(axis=1)
        assert np.array_equal(filled, np.minimum(p["lens"], k)), k
        pad = filled < k
        assert pad.any() and (filled == k).any()


# ---- 4. ties at the cut, at every block size -------------------------------------------------------------------------------------------------
def _list_position(t, j):
    """(instance, shape) → position in ray j's list-order row"""
    off, inst, shape, _ = t["uncut_list"]
    return {(int(i), int(sh)): p for p, (i, sh) in enumerate(zip(inst[off[j]:off[j + 1]], shape[off[j]:off[j + 1]]))}


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_at_the_cut(orc, dtype):
    t = tie_case(orc, dtype)
    off, inst, shape, vals = t["uncut"]
    lens = np.diff(off.astype(np.int64))
    assert lens[:8].tolist() == [512] * 8 and lens[8:].tolist() == [1088] * 8
    lo = t["uncut_list"]
    rows = {k: ikh.incremental(t["table"], N_TIE_RAYS, None, k, dtype) for k in K}
    for j in range(N_TIE_RAYS):
        d = vals[off[j]:off[j + 1], 0]
        first = 30 if j < 8 else 21
        assert d[:4].tolist() == [1.0625, 1.0625, 1.1875, 1.1875]
        head = d[:128]                                                                     # the coincident pair: 64 hits each
        assert (head[0::2] == head[1::2]).all() and (np.diff(head[0::2]) > 0).all()        # every distance there appears exactly twice
        assert inst[off[j]:off[j] + 64].tolist() == [first, first + 1] * 32                # the pair met first comes first
        ld = lo[3][lo[0][j]:lo[0][j + 1], 0]
        assert (lo[1][lo[0][j]:lo[0][j] + 64] == first).all() and (np.diff(ld) < 0).any()  # the list starts with one copy alone: not ascending
        pos = _list_position(t, j)
        for k in K:
            oi, os_, ov = (w[j] for w in rows[k])
            assert ov[:, 0].tobytes() == d[:k].tobytes()
            if k % 2:       # the cut splits a tie pair: the kept slot holds the pair met first
                assert d[k - 1] == d[k]
                kept, dropped = (int(oi[k - 1]), int(os_[k - 1])), (int(inst[off[j] + k]), int(shape[off[j] + k]))
                assert kept == (int(inst[off[j] + k - 1]), int(shape[off[j] + k - 1])) and pos[kept] < pos[dropped], (j, k)
            else:           # ties inside the row
                assert (np.diff(ov[:, 0]) == 0).sum() == k // 2, (j, k)


def test_the_reference_stands_alone():
    src = open(os.path.join(ROOT, "tests", "instances_khits_ref.py")).read()
    assert "import bvh_amd" not in src and "from bvh_amd" not in src


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_is_built_and_bound():
    import re
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances_khits.hip" in build_ext.SOURCES
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert re.search(r"#define BVHGPU_INSTANCES_KHITS_MAX_K 64u", header)
    for sfx in ("f32", "f64"):
        assert re.search(r"\nint bvhgpu_instances_khits_%s\(bvhgpu_instances \*s, const bvhgpu_ray_%s \*rays," % (sfx, sfx), header), sfx
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_instances_khits", b"k_instances_khits_fill"):
        assert kern in blob, kern
    symbols = {s[0]: s for s in _lib.SYMBOLS}
    for sym in ("bvhgpu_instances_khits_f32", "bvhgpu_instances_khits_f64"):
        assert sym in symbols and len(symbols[sym][2]) == 9, sym
    assert _lib.INSTANCES_KHITS_MAX_K == 64
    import bvh_amd
    assert hasattr(bvh_amd.Instances, "khits_batch")
