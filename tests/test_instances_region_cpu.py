"""Convex regions over instanced scenes, CPU side: the plane transform by hand, two anchors that do not lean on the new reference's
stage 2, the kernel's (pair, chunk) schedule restated on the CPU against the definition, the scenes tests/test_gpu_instances_region.py
runs shown on the reference alone (tests/instances_region_ref.py) to be non-trivial, and the wiring of the new entry into every layer."""
import os
import re

import numpy as np
import pytest

import instances_ref as ir
import instances_region_ref as irr
import region_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


def _rows(off, *cols):
    return [tuple(c[off[q]:off[q + 1]].tolist() for c in cols) for q in range(len(off) - 1)]


# ---- 1. the plane transform, by hand -----------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["rotation", "scale", "mirror"])
def test_a_point_keeps_its_side_under_the_transformed_plane(dtype, kind):
    """n.(M p + t) + d = (M^T n).p + (n.t + d): the world plane's value at the image of p is the object plane's value at p"""
    M = {"rotation": _rot([1, 2, 3], 0.7), "scale": np.diag([0.5, 2.0, 1.25]), "mirror": _rot([0, 1, 1], 1.1) @ np.diag([1.0, -1.5, 0.75])}[kind]
    x = np.concatenate([M, [[3.0], [-2.0], [0.5]]], axis=1).astype(dtype)
    assert (np.linalg.det(M) < 0) == (kind == "mirror")
    rng = np.random.default_rng(3)
    planes = rng.normal(size=(50, 4)).astype(dtype)
    op = irr.object_planes(x, planes)
    assert op.dtype == dtype and op.shape == planes.shape
    p = rng.uniform(-4, 4, size=(50, 3))
    world = p @ x[:, :3].astype(np.float64).T + x[:, 3].astype(np.float64)
    vw = (planes[:, :3].astype(np.float64) * world).sum(axis=1) + planes[:, 3]
    vo = (op[:, :3].astype(np.float64) * p).sum(axis=1) + op[:, 3]
    tol = 64 * np.finfo(dtype).eps * 40
    assert np.abs(vw - vo).max() < tol
    clear = np.abs(vw) > tol
    assert clear.sum() >= 40 and ((vw[clear] >= 0) == (vo[clear] >= 0)).all()
    assert (vw[clear] >= 0).any() and (vw[clear] < 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_and_padding_planes(dtype):
    planes = np.random.default_rng(4).normal(size=(3, 5, 4)).astype(dtype)
    planes[1, 3:] = 0
    ident = np.eye(3, 4, dtype=dtype)
    assert irr.object_planes(ident, planes).tobytes() == (planes + dtype(0)).tobytes()   # (x + 0: the sums turn a -0 into +0, nothing else)
    x = np.concatenate([_rot([1, 1, 0], 2.0) @ np.diag([-1.0, 2.0, 0.5]), [[7.0], [8.0], [9.0]]], axis=1).astype(dtype)
    op = irr.object_planes(x, planes)
    assert (op[1, 3:] == 0).all() and (op[1, :3] != 0).any()
    # by hand, one plane: n' = M^T n, d' = n.t + d
    n, d = planes[0, 0, :3], planes[0, 0, 3]
    want = [(x[0, j] * n[0] + x[1, j] * n[1]) + x[2, j] * n[2] for j in range(3)] + [((n[0] * x[0, 3] + n[1] * x[1, 3]) + n[2] * x[2, 3]) + d]
    assert op[0, 0].tolist() == [float(v) for v in want]


# ---- 2. anchors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree(orc, dtype):
    """one instance, identity transform: the rows are region_ref.walk's over the member, instance 0 throughout"""
    aabbs, tris = irr.main_members(dtype)[2]
    sc = ir.Scene([(aabbs, tris)], [0], np.eye(3, 4, dtype=dtype)[None], dtype)
    planes = rr.random_regions(aabbs, 30, 17)
    off, idx, ins = rr.walk(sc.flats[0], aabbs, planes)
    # the top level is one leaf whose box is the member's bounds: a region that reports a shape passes it (exact joins, fact 1)
    ref = irr.reference(sc, planes)
    got = ref["full"]
    assert got[0].tobytes() == off.tobytes() and got[2].tobytes() == idx.tobytes() and got[3].tobytes() == ins.tobytes()
    assert (got[1] == 0).all() and len(idx) > 500 and (np.diff(off.astype(np.int64)) == 0).any()


def exact_scene(dtype, seed=23):
    """members whose box coordinates are multiples of 1/8 below 2^10 / 4, instances X = [I | t] with t a multiple of 1/8, planes with small
    integer normals and d a multiple of 1/8: every product and sum of both stages is exact in f32 → (trees, tree_of, x, planes)"""
    rng = np.random.default_rng(seed)
    trees = []
    for n in (40, 7):
        lo = rng.integers(-800, 800, size=(n, 3)) / 8.0
        hi = lo + rng.integers(1, 160, size=(n, 3)) / 8.0
        a = np.concatenate([lo, hi], axis=1).astype(dtype)
        tris = np.stack([a[:, :3], a[:, [3, 1, 5]], a[:, [0, 4, 5]]], axis=1)
        trees.append((np.ascontiguousarray(a), np.ascontiguousarray(tris)))
    k = 6
    x = np.zeros((k, 3, 4), dtype=dtype)
    x[:, :, :3] = np.eye(3)
    x[:, :, 3] = rng.integers(-1200, 1200, size=(k, 3)) / 8.0
    of = np.array([0, 1, 0, 1, 0, 0], dtype=np.uint32)
    planes = np.zeros((30, 4, 4), dtype=dtype)
    for q in range(30):
        for j in range(int(rng.integers(1, 5))):
            nrm = rng.integers(-3, 4, size=3)
            nrm[0] = nrm[0] or 1
            pt = rng.integers(-1600, 1600, size=3) / 8.0
            planes[q, j, :3] = nrm
            planes[q, j, 3] = -float(np.dot(nrm, pt))
    return trees, of, x, planes


@pytest.mark.parametrize("dtype", DTYPES)
def test_translated_instances_equal_the_flattened_scene(orc, dtype):
    """X = [I | t] in exact arithmetic: the world-space boxes a row reports are the brute-force set over the flattened scene"""
    import fuzz_scenes as fz
    trees, of, x, planes = exact_scene(dtype)
    sc = ir.Scene(trees, of, x, dtype)
    assert not any(fz.has_empty_child_bounds(f) for f in sc.flats) and not fz.has_empty_child_bounds(sc.top)
    base = np.concatenate([[0], np.cumsum([len(trees[t][0]) for t in of])])
    world = np.concatenate([trees[t][0] + np.tile(x[i, :, 3], 2) for i, t in enumerate(of)])
    assert world.dtype == dtype
    off, inst, shape, _ = irr.reference(sc, planes)["full"]
    nonempty = 0
    for q in range(len(planes)):
        got = sorted((base[inst[off[q]:off[q + 1]]] + shape[off[q]:off[q + 1]]).tolist())
        assert got == rr.brute(world, planes[q], dtype).tolist(), q
        nonempty += bool(got)
    assert nonempty >= 10 and off[-1] < len(planes) * len(world) // 2


# ---- 3. the schedule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_chunk_units_cover_every_row(orc, dtype):
    """every pair of the main scene by the kernel's schedule (region_ref.scan over the member's folded array with the object-space
    planes) at the chunk the rule gives the batch and at the smallest chunk: the definition's L'"""
    m = irr.main_scene(dtype)
    sc, ref = m["scene"], m["ref"]
    inst = ref["top"][1]
    P = len(inst)
    sched = irr.schedule(sc, P)
    ents = [irr.member_entries(sc, t) for t in range(len(sc.trees))]
    over_border = 0
    for p in range(P):
        t = int(sc.tree_of[inst[p]])
        want = ref["pair_rows"][p].tolist()
        for ce in {sched["members"][t][1], irr.CHUNK_MIN}:
            units = []
            assert rr.scan(ents[t], ref["pair_planes"][p], 64, ce, units=units) == want, (p, ce)
            assert len(units) == -(-len(ents[t]["exit"]) // ce)
            over_border += sum(u["count"] > 0 for u in units) >= 2
    assert over_border >= 3
    assert sched["members"][3][0] == 16798 and -(-16798 // 1024) == 17
    assert len({mb[2] for mb in sched["members"]}) >= 2       # members with different chunk counts share the launch


@pytest.mark.parametrize("dtype", DTYPES)
def test_units_stay_below_pairs_plus_8192(orc, dtype):
    cases = [irr.main_scene(dtype)] + [irr.case(dtype, name) for name in irr.CASES]
    seen = set()
    for c in cases:
        P = len(c["ref"]["top"][1])
        if P == 0:
            continue
        s = irr.schedule(c["scene"], P)
        assert s["units"] < P + irr.REGION_UNITS_TARGET, (P, s)
        assert all(nc <= -(-irr.REGION_UNITS_TARGET // P) for _, _, nc in s["members"])
        seen.add(s["nc_max"])
    assert {1, 2, 17} <= seen                                  # one chunk per pair, two (the 2 500-region batch), the smallest chunks
    for P in (1, 37, 8191, 8192, 10 ** 6, 2 ** 32 - 1):
        for e in (1, 1023, 1025, 16798, 2 ** 32 - 100):
            ce = irr.chunk_entries(P, e)
            assert P * (-(-e // ce)) < P + irr.REGION_UNITS_TARGET


# ---- 4. the scenes are not trivial --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_main_scene_is_not_trivial(orc, dtype):
    m = irr.main_scene(dtype)
    sc, ref, planes = m["scene"], m["ref"], m["planes"]
    n = len(planes)
    assert [len(a) for a, _ in m["trees"]] == [1, 12, 240, 8400] and len(sc.x) == 37 and n == 52
    toff, tidx, tins = ref["top"]
    off, inst, shape, ins = ref["full"]
    assert off[-1] == len(inst) == len(shape) == len(ins) and off[-1] > 10000
    rows = _rows(off, inst, shape, ins)
    assert sum(len(set(r[0])) >= 2 for r in rows) >= 10                         # rows that hold two or more instances
    assert sum(len(r) == 0 for r in ref["pair_rows"]) >= 10                     # pairs that pass the top level and report no shape
    culled = set()
    for q in range(n):
        here = set(tidx[toff[q]:toff[q + 1]].tolist())
        if rows[q][0]:
            culled |= set(range(37)) - here
    assert len(culled) >= 10                                                    # instances culled at the top by a region that reports others
    assert sum(0 in r[2] for r in rows) >= 10 and sum(1 in r[2] for r in rows) >= 10
    assert (tins == 0).any() and (tins == 1).any()
    mirrored = [i for i in range(37) if i % 5 == 4]
    assert np.linalg.det(sc.x[4, :, :3].astype(np.float64)) < 0 and np.isin(inst, mirrored).any()
    # a cutting region reports a shape of the large member it does not wholly contain
    cut = slice(irr.MAIN_REGIONS, n)
    assert sum(any(i == 0 and b == 0 for i, b in zip(r[0], r[2])) for r in rows[cut]) >= 6
    # each instance's order inside a row is the top level's, and an instance's shapes are contiguous
    for q in range(n):
        order = [i for k, i in enumerate(rows[q][0]) if k == 0 or rows[q][0][k - 1] != i]
        assert len(order) == len(set(order))
        it = iter(tidx[toff[q]:toff[q + 1]].tolist())
        assert all(i in it for i in order)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pose_and_transforms_matter(orc, dtype):
    m = irr.main_scene(dtype)
    first = m["ref"]["full"]
    second = irr.reference(ir.Scene(m["trees"], m["tree_of"], m["x2"], dtype), m["planes"])["full"]
    assert second[0].tobytes() != first[0].tobytes() and second[1].tobytes() != first[1].tobytes()
    ident = np.tile(np.eye(3, 4, dtype=dtype), (37, 1, 1))
    plain = irr.reference(ir.Scene(m["trees"], m["tree_of"], ident, dtype), m["planes"])["full"]
    assert plain[0].tobytes() != first[0].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_other_cases_are_what_they_claim(orc, dtype):
    c = {name: irr.case(dtype, name) for name in irr.CASES}
    P = {name: len(v["ref"]["top"][1]) for name, v in c.items()}
    tot = {name: int(v["ref"]["full"][0][-1]) for name, v in c.items()}
    assert len(c["one"]["scene"].x) == 1 and len(c["two"]["scene"].x) == 2 and tot["one"] > 100 and tot["two"] > 100
    assert [len(a) for a, _ in c["tri"]["trees"]] == [1] and 0 < tot["tri"] < P["tri"]
    assert len(c["many"]["planes"]) == 2500 and 4096 <= P["many"] < 8192 and irr.schedule(c["many"]["scene"], P["many"])["nc_max"] == 2
    assert c["m0"]["planes"].shape[1] == 0 and P["m0"] == 2 * 37 and tot["m0"] == 2 * sum(len(c["m0"]["trees"][t][0]) for t in c["m0"]["tree_of"])
    assert c["m1"]["planes"].shape[1] == 1 and tot["m1"] > 100
    assert c["m32"]["planes"].shape[1] == 32 and (c["m32"]["planes"][:, :, :3] != 0).any(axis=2).all() and tot["m32"] > 100
    assert len(c["n1"]["planes"]) == 1 and P["n1"] >= 20 and irr.schedule(c["n1"]["scene"], P["n1"])["nc_max"] == 17
    assert P["none"] == 0 and tot["none"] == 0 and len(c["none"]["planes"]) == 3


# ---- 5. wiring ----------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_is_in_every_layer():
    from bvh_amd import _lib, build_ext
    from bvh_amd.instances import Instances
    names = [s[0] for s in _lib.SYMBOLS]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    for sym in ("bvhgpu_instances_region_f32", "bvhgpu_instances_region_f64", "bvhgpu_hits_fetch_instances_region"):
        assert sym in names, sym
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
    assert re.search(r"#define BVHGPU_REGION_INSTANCES_ONLY 4u\b", header)
    assert re.search(r"pub const BVHGPU_REGION_INSTANCES_ONLY: c_uint = 4;", ffi)
    assert _lib.REGION_INSTANCES_ONLY == 4
    assert re.search(r"#define BVHGPU_ABI_VERSION 7\b", header)
    assert "region.hip" in build_ext.SOURCES and "instances.hip" in build_ext.SOURCES and "rows.hpp" in build_ext.HEADERS
    src = open(os.path.join(ROOT, "bvh_amd", "csrc", "region.hip")).read()
    assert "k_instances_region_walk" in src and "region_unit<T, true, FILL, CLASSIFY>" in src and "region_unit<T, false, FILL, CLASSIFY>" in src
    assert hasattr(Instances, "region_batch")
    assert "region_query" in open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read().split("impl<T: GpuScalar> GpuInstances<T>")[1]
    assert os.path.exists(os.path.join(ROOT, "tools", "instances_region_bench.py"))
