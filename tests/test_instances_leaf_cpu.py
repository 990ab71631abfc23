"""Instance sets of BOX and SPHERE leaves, CPU side: hand anchors with exact answers in f32 and f64; the scenes
tests/test_gpu_instances_leaf.py runs, shown on the reference alone (tests/instances_leaf_ref.py over the oracle) to be non-trivial; the
k-hits definition against the incremental list; and the wiring of the new entries."""
import os

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_khits_ref as ikr
import instances_leaf_ref as ilr
import instances_masks_ref as imr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF
AT_LEAST = 20


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- hand anchors ------------------------------------------------------------------------------------------------------------------------
UNIT = (np.array([[-1, -1, -1, 1, 1, 1.0]]), np.array([[0, 0, 0, 1.0]]))     # the unit sphere at the origin in its box [-1, 1]^3
POSE = np.array([[2, 0, 0, 8], [0, 1, 0, 0], [0, 0, 1, 0.0]])               # diag(2, 1, 1), then (8, 0, 0)


def _anchor(orc, dtype, leaf, n):
    sc = ilr.LeafScene([UNIT], [0] * n, np.stack([POSE] * n), dtype, leaf)
    rays = orc.make_rays(np.zeros((1, 3), dtype), np.array([[1, 0, 0]], dtype), dtype)
    return sc, rays


@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_stretched_unit_sphere(orc, dtype, leaf):
    """X = diag(2, 1, 1) + (8, 0, 0): the ellipsoid / the box spans x in [6, 10].  In the object frame o' = (-4, 0, 0), d' = (0.5, 0, 0):
    a = 0.25, tc = 8, h = 2 — every number a small dyadic rational, so {6, 10} is exact in both formats and for both kinds"""
    sc, rays = _anchor(orc, dtype, leaf, 1)
    o = sc.object_rays(rays, 0)
    assert o["o"].tolist() == [[-4, 0, 0]] and o["d"].tolist() == [[0.5, 0, 0]]
    res = sc.trace(rays)
    for name in ("closest", "first"):
        vals, inst, shape = res[name]
        assert vals.dtype == dtype and vals.tolist() == [[6, 10, 0]] and inst.tolist() == [0] and shape.tolist() == [0], (name, vals)
    for tmax, hit in ((6, False), (np.nextafter(dtype(6), dtype(7)), True)):     # tmax is strict, in T
        cut = sc.trace(rays, np.array([tmax], dtype))
        for name in ("closest", "first"):
            vals, inst, shape = cut[name]
            assert (inst.tolist(), shape.tolist()) == (([0], [0]) if hit else ([NONE], [NONE])), (name, tmax)
            assert vals.tolist() == ([[6, 10, 0]] if hit else [[np.inf, 0, 0]])


@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_tie_goes_to_the_earlier_instance_of_the_top_level(orc, dtype, leaf):
    sc, rays = _anchor(orc, dtype, leaf, 2)
    res = sc.trace(rays)
    order = res["top"][1].tolist()
    assert sorted(order) == [0, 1]
    assert res["table"]["vals"].tolist() == [[6, 10, 0], [6, 10, 0]] and res["table"]["instance"].tolist() == order
    assert res["closest"][1].tolist() == [order[0]] and res["first"][1].tolist() == [order[0]]
    oi, os_, ov = ikr.definition(res["table"], 1, None, 3, dtype)
    assert oi.tolist() == [order + [NONE]] and ov[0, :, 0].tolist() == [6, 6, np.inf]


# ---- what the GPU scenes contain -----------------------------------------------------------------------------------------------------------
def _per_ray(table, f):
    off = table["cand_off"]
    return np.array([f(table["vals"][off[j]:off[j + 1]]) for j in range(len(off) - 1)])


@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_scenes_are_not_trivial(orc, dtype, leaf):
    assert ilr.MEMBER_SHAPES == (1, 12, 240) and ilr.SIZES == (1, 2, 37) and ilr.N_RAYS == 1500
    assert [len(a) for a, _ in ilr.member_trees(dtype)] == [1, 12, 240]
    c = ilr.case(dtype, 37, leaf)
    free, cut = c["free"], c["cut"]
    assert (np.linalg.det(c["x"][:, :, :3].astype(np.float64)) < 0).sum() >= 5           # mirrored instances
    hit = free["closest"][1] != NONE
    seen = {
        "hit": hit.sum(),
        "miss": (~hit).sum(),
        "two or more world boxes": (np.diff(free["top"][0].astype(np.int64)) >= 2).sum(),
        "closest behind the first instance that yields a hit": (hit & (free["closest"][1] != free["first"][1])).sum(),
        "closest is not first": (hit & ((free["closest"][1] != free["first"][1]) | (free["closest"][2] != free["first"][2]))).sum(),
        "cut by tmax": (hit & (cut["closest"][1] == NONE)).sum(),
        "tmax moves the closest hit or leaves it": (cut["closest"][1] != NONE).sum(),
    }
    if leaf == "sphere":   # an origin inside an ellipsoid: t0 <= eps, the hit is at t1 = exit
        seen["origin inside an ellipsoid"] = _per_ray(free["table"], lambda v: bool((np.isfinite(v[:, 0]) & (v[:, 0] == v[:, 1])).any())).sum()
        assert not free["table"]["vals"][:, 2].any()
    M, R, table = c["inst_mask"], c["ray_mask"], free["table"]
    seen["a masked closest hit that is not the unmasked one"] = (imr.closest(table, M, R, ilr.N_RAYS, None, dtype)[1] != free["closest"][1]).sum()
    seen["all-hits rows beyond the tier a lane sorts itself"] = (
        np.diff(iar.rows(table, ilr.N_RAYS, None, dtype)[0].astype(np.int64)) > iar.engine_thresholds(ROOT)[0]).sum()
    for what, count in seen.items():
        assert count >= AT_LEAST, (what, count)
    # every set size has hits and misses, and the two smaller sets are where a ray meets one world box or none
    for n in (1, 2):
        small = ilr.case(dtype, n, leaf)["free"]
        assert (small["closest"][1] != NONE).sum() >= AT_LEAST and (small["closest"][1] == NONE).sum() >= AT_LEAST


@pytest.mark.parametrize("leaf", ilr.LEAVES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_khits_definition_is_the_incremental_list(orc, dtype, leaf):
    c = ilr.case(dtype, 37, leaf)
    table, n = c["free"]["table"], ilr.N_RAYS
    for tmax in (None, c["tmax"]):
        tm = np.full(n, np.inf, dtype) if tmax is None else tmax
        off = table["cand_off"]
        counts = np.array([(table["vals"][off[j]:off[j + 1], 0] < tm[j]).sum() for j in range(n)])
        for k in (1, 3, 64):
            a, b = ikr.definition(table, n, tmax, k, dtype), ikr.incremental(table, n, tmax, k, dtype)
            assert ikr.same(a, b), (k, tmax is None)
            assert (a[0][:, 0] != NONE).sum() == (counts > 0).sum()
            if tmax is None:
                assert (counts < k).any() and (counts == k).any() and (counts > k).any(), k
    k1 = ikr.definition(table, n, c["tmax"], 1, dtype)
    assert k1[2][:, 0].tobytes() == c["cut"]["closest"][0].tobytes() and k1[0][:, 0].tobytes() == c["cut"]["closest"][1].tobytes()


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_and_bound():
    from bvh_amd import _lib
    from bvh_amd.instances import Instances
    sig = {s[0]: s for s in _lib.SYMBOLS}
    assert len(sig["bvhgpu_instances_create_leaf_f32"][2]) == len(sig["bvhgpu_instances_create_f32"][2]) + 1 == 9
    assert len(sig["bvhgpu_instances_create_leaf_f64"][2]) == 9 and len(sig["bvhgpu_instances_leaf"][2]) == 2
    assert _lib.LEAF_KINDS == {"box": 0, "triangle": 1, "sphere": 2} and _lib.LEAF_WIDTH == {0: 2, 1: 3, 2: 2}
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    for name in ("create_leaf_f32", "create_leaf_f64", "leaf"):
        assert f"int bvhgpu_instances_{name}(" in header, name
    assert "#define BVHGPU_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    assert "leaf" not in vars(Instances)                     # a plain instance attribute
    for src in ("instances.hip", "instances_khits.hip", "instances_allhits.hip"):
        text = open(os.path.join(ROOT, "bvh_amd", "csrc", src)).read()
        assert "leaf_record<T, LEAF>" in text and "INST_LEAF_VALUE" in text, src


def test_the_library_holds_the_leaf_kernels():
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    # (Itanium mangling: the leaf kind is the last template argument, Li0E = BOX, Li2E = SPHERE; the triangle sets keep the kernels without it)
    for kern in (b"k_instances_trace_leafIfLb0ELb0ELi0E", b"k_instances_trace_leafIdLb1ELb1ELi2E", b"k_instances_khits_leafIfLb0ELi2E",
                 b"k_instances_khits_leafIdLb1ELi0E", b"k_instances_allhits_count_leafIfLb0ELi0E", b"k_instances_allhits_fill_leafIdLb1ELb1ELi2E",
                 b"k_instances_allhits_sort_row_leafIfLi0E", b"k_instances_traceIfLb0ELb0EEEv", b"k_instances_khitsIdLb1EEEv"):
        assert kern in blob, kern
    assert b"k_instances_trace_leafIfLb0ELb0ELi1E" not in blob   # no second triangle kernel
