"""CPU checker for convex-region batches over instanced scenes (a helper module, not collected by pytest).

Restates the definition of bvhgpu_instances_region_* (include/bvh_mi355x.h) with numpy in the set's dtype T, one rounded operation per
step, over instances_ref.Scene (its x, w, top, flats) and region_ref.walk:
  stage 1   I_q = row q of region_ref.walk(scene.top, scene.w, planes): the instances whose world box passes the WORLD planes
  planes'   the planes of region q in instance i's object frame, from the FORWARD transform X_i = m[k][j], written out by hand:
                n'[j] = ((m[0][j]*n[0] + m[1][j]*n[1]) + m[2][j]*n[2])
                d'    = (((n[0]*m[0][3] + n[1]*m[1][3]) + n[2]*m[2][3]) + d)
  stage 2   L' = region_ref.walk(member's FlatNode array, member's shape AABBs, planes') per (region, instance) pair
  row q     the concatenation of (i, s) for i in I_q, s in L'
It reads no array the engine produced.  Also the scenes tests/test_instances_region_cpu.py qualifies and tests/test_gpu_instances_region.py
runs, computed once per dtype and never modified.
"""
from __future__ import annotations

import numpy as np

import instances_ref as ir
import region_ref as rr

REGION_UNITS_TARGET = 8192   # bvh_amd/csrc/region.hip: units a batch is cut into at least, while chunks stay above the minimum
CHUNK_MIN = 1024


def object_planes(x: np.ndarray, planes: np.ndarray) -> np.ndarray:
    """planes (..., 4) in world space → the same planes in the frame of the instance with the forward transform x (3, 4); everything in
    the planes' dtype, in the header's order"""
    x = np.asarray(x).reshape(3, 4)
    n0, n1, n2, d = planes[..., 0], planes[..., 1], planes[..., 2], planes[..., 3]
    out = np.empty_like(planes)
    with np.errstate(all="ignore"):
        for j in range(3):
            out[..., j] = (x[0, j] * n0 + x[1, j] * n1) + x[2, j] * n2
        out[..., 3] = ((n0 * x[0, 3] + n1 * x[1, 3]) + n2 * x[2, 3]) + d
    return out


def pair_planes(scene: ir.Scene, planes: np.ndarray, pair_region: np.ndarray, pair_inst: np.ndarray) -> np.ndarray:
    """(P, m, 4): the object-space planes of every (region, instance) pair"""
    out = np.empty((len(pair_region),) + planes.shape[1:], dtype=planes.dtype)
    for p, (q, i) in enumerate(zip(pair_region, pair_inst)):
        out[p] = object_planes(scene.x[int(i)], planes[int(q)])
    return out


def reference(scene: ir.Scene, planes) -> dict:
    """every answer of one batch: dict(
         top = (offsets, instance, inside)            BVHGPU_REGION_INSTANCES_ONLY [| CLASSIFY]: I_q as a CSR — also the pair table
         full = (offsets, instance, shape, inside)    flags 0 / CLASSIFY; COUNT_ONLY is its offsets
         pair_region, pair_planes, pair_rows          per pair: its region, its object-space planes, its L' as a list)"""
    ft = scene.ft
    pl = rr._planes_in(planes, ft)
    n = len(pl)
    toff, tidx, tins = rr.walk(scene.top, scene.w, pl)
    pair_region = np.repeat(np.arange(n), np.diff(toff.astype(np.int64)))
    P = len(tidx)
    opl = pair_planes(scene, pl, pair_region, tidx)
    rows, bytes_ = [None] * P, [None] * P
    member_of = scene.tree_of[tidx.astype(np.int64)] if P else np.zeros(0, dtype=np.int64)
    for t in np.unique(member_of):                       # one lockstep walk per member over all of its pairs
        sel = np.nonzero(member_of == t)[0]
        off, idx, ins = rr.walk(scene.flats[int(t)], scene.trees[int(t)][0], opl[sel])
        for k, p in enumerate(sel):
            rows[p] = idx[off[k]:off[k + 1]]
            bytes_[p] = ins[off[k]:off[k + 1]]
    cnt = np.zeros(n, dtype=np.uint64)
    for p in range(P):
        cnt[pair_region[p]] += len(rows[p])
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(cnt).astype(np.uint32)
    inst = np.concatenate([np.full(len(rows[p]), tidx[p], dtype=np.uint32) for p in range(P)]) if P else np.zeros(0, dtype=np.uint32)
    shape = np.concatenate(rows).astype(np.uint32) if P else np.zeros(0, dtype=np.uint32)
    inside = np.concatenate(bytes_).astype(np.uint8) if P else np.zeros(0, dtype=np.uint8)
    return dict(top=(toff, tidx, tins), full=(offsets, inst, shape, inside), pair_region=pair_region, pair_planes=opl, pair_rows=rows)


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------
def chunk_entries(n_pairs: int, n_trav: int) -> int:
    """region.hip region_chunk_entries: entries per chunk of a member of n_trav entries in a batch of n_pairs pairs"""
    per = (REGION_UNITS_TARGET + n_pairs - 1) // n_pairs
    ce = (n_trav + per - 1) // per
    ce = (ce + 63) // 64 * 64
    return max(ce, CHUNK_MIN)


def member_entries(scene: ir.Scene, t: int) -> dict:
    """the array the kernel walks for member t: folded for a built tree, the one entry of a single-shape tree"""
    return rr.entries(scene.flats[t], scene.trees[t][0], True)


def schedule(scene: ir.Scene, n_pairs: int) -> dict:
    """how a batch of n_pairs pairs cuts the members: per member (n_trav, ce_t, nc_t), the uniform stride nc_max and the units"""
    per = []
    for t in range(len(scene.trees)):
        e = len(member_entries(scene, t)["exit"])
        ce = chunk_entries(n_pairs, e)
        per.append((e, ce, (e + ce - 1) // ce))
    nc_max = max(p[2] for p in per)
    return dict(members=per, nc_max=nc_max, units=n_pairs * nc_max)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
MAIN_INSTANCES, MAIN_REGIONS, MAIN_CUT, MAIN_SEED = 37, 40, 12, 5
BIG_CUBES = 700
_main = {}


def _tris_aabbs(tris):
    t = tris.reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))


def main_members(dtype) -> list:
    """one triangle, 12 (a cube), 240 (20 cubes) — test_instances_cpu.member_trees — and 700 cubes (8 400 shapes, 16 798 folded entries)
    drawn inside [-3, 3]^3 like the others → [(aabbs, tris)] in dtype"""
    from oracle import orc
    from test_instances_cpu import member_trees
    a, b, c = member_trees(orc, dtype)
    small = np.array([-3.0] * 3 + [3.0] * 3, dtype=np.float32)
    tb, _ = orc.create_n_cubes(BIG_CUBES, small)
    tb = np.ascontiguousarray(tb.astype(dtype)).reshape(-1, 3, 3)
    return [c, a, b, (_tris_aabbs(tb), tb)]


def main_slots(n: int, seed: int) -> np.ndarray:
    """which member each instance copies: the first four are the four members, the rest at random"""
    rng = np.random.default_rng(seed)
    of = rng.integers(0, 4, size=n)
    of[:min(n, 4)] = [3, 0, 1, 2][:min(n, 4)]
    return of.astype(np.uint32)


def cutting_regions(scene: ir.Scene, n: int, seed: int, pad_to: int) -> np.ndarray:
    """n regions whose FIRST plane passes through the centre of a shape of the large member as instance 0 places it (the centre mapped by
    the forward transform in float64), the others turned to keep that centre inside: rows that report shapes they do not wholly contain"""
    rng = np.random.default_rng(seed)
    a = scene.trees[int(scene.tree_of[0])][0].astype(np.float64)
    x = scene.x[0].astype(np.float64)
    out = np.zeros((n, pad_to, 4))
    for q in range(n):
        b = a[int(rng.integers(0, len(a)))]
        centre = x[:, :3] @ ((b[:3] + b[3:]) / 2) + x[:, 3]
        for j in range(int(rng.integers(1, pad_to + 1))):
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            pt = centre if j == 0 else centre + rng.normal(size=3) * 2.0
            if np.dot(nrm, centre - pt) < 0:
                nrm = -nrm
            out[q, j, :3] = nrm
            out[q, j, 3] = -np.dot(nrm, pt)
    return out.astype(scene.ft)


def small_balls(boxes: np.ndarray, n: int, seed: int, planes: int = 8) -> np.ndarray:
    """region_ref.ball_regions with radii of 4 - 12 % of the half extent: n regions that touch most world boxes of a small set and report
    few shapes each, so that a batch of thousands keeps a small total"""
    rng = np.random.default_rng(seed)
    a = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    lo, hi = a[:, :3].min(axis=0), a[:, 3:].max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    out = np.zeros((n, planes, 4))
    for q in range(n):
        c = mid + half * 0.6 * rng.uniform(-1, 1, size=3)
        r = float(half.min()) * rng.uniform(0.04, 0.12)
        nrm = rng.normal(size=(planes, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        out[q, :, :3] = nrm
        out[q, :, 3] = r - nrm @ c
    return out.astype(np.asarray(boxes).dtype)


CASES = ("one","two", "tri", "many", "m0", "m1", "m32", "n1", "none")
MANY_REGIONS = 2500
_cases = {}


def case(dtype, name: str) -> dict:
    """the other batches the GPU test runs, each dict(trees, tree_of, x, scene, planes, ref), computed once per dtype:
      one / two   sets of 1 and 2 instances (the large member; the large member and the 20 cubes), 20 random regions
      tri         5 instances of a set whose only member is the one-triangle tree
      many        2 500 small ball regions of 8 planes over the set `two`: 4 096 <= P < 8 192, so the large member is cut into 2 chunks
      m0, m1, m32 the main set with plane-less regions, with one plane each, and with 32 real planes tangent to balls in one world box
      n1          ONE region over the main set: the chunk rule gives its smallest chunks, so the stride nc_max is at its largest
      none        regions far outside every world box: P == 0"""
    key = (np.dtype(dtype).name, name)
    if key in _cases:
        return _cases[key]
    from test_instances_cpu import transforms
    m = main_scene(dtype)
    trees, of, x, sc = m["trees"], m["tree_of"], m["x"], m["scene"]
    if name in ("one", "two", "many"):
        k = 1 if name == "one" else 2
        trees, of, x = [m["trees"][3], m["trees"][2]][:k], np.arange(k, dtype=np.uint32), transforms(k, dtype, 70 + k)
        sc = ir.Scene(trees, of, x, dtype)
        planes = rr.random_regions(sc.w, 20, 80 + k) if name != "many" else small_balls(sc.w, MANY_REGIONS, 83)
    elif name == "tri":
        trees, of, x = [m["trees"][0]], np.zeros(5, dtype=np.uint32), transforms(5, dtype, 75)
        sc = ir.Scene(trees, of, x, dtype)
        planes = rr.random_regions(sc.w, 20, 85, max_planes=2)
    elif name == "m0":
        planes = np.zeros((2, 0, 4), dtype=dtype)
    elif name == "m1":
        planes = rr.random_regions(sc.w, 8, 86, max_planes=1)
    elif name == "m32":
        planes = rr.ball_regions(sc.w[:1], 12, 87)
    elif name == "n1":
        counts = np.diff(m["ref"]["top"][0].astype(np.int64))
        planes = m["planes"][int(np.argmax(counts))][None]
    elif name == "none":
        far = np.array([[1e4, 1e4, 1e4, 1e4 + 1, 1e4 + 1, 1e4 + 1]])
        planes = np.stack([rr.random_regions(far, 1, 88 + q, max_planes=3, pad_to=6)[0] for q in range(3)]).astype(dtype)
        planes[:, 0] = np.array([1, 0, 0, -9e3], dtype=dtype)      # x >= 9 000: beyond every world box
    else:
        raise KeyError(name)
    planes = np.ascontiguousarray(planes, dtype=dtype)
    _cases[key] = dict(trees=trees, tree_of=of, x=x, scene=sc, planes=planes, ref=reference(sc, planes))
    return _cases[key]


def main_scene(dtype) -> dict:
    """the scene the GPU test runs and tests/test_instances_region_cpu.py qualifies: four members, 37 instances, 40 random regions over the
    world boxes and 12 cutting ones, a second pose, and the definition's rows for both — computed once per dtype and shared"""
    key = np.dtype(dtype).name
    if key not in _main:
        from test_instances_cpu import transforms
        trees = main_members(dtype)
        of = main_slots(MAIN_INSTANCES, MAIN_SEED)
        x = transforms(MAIN_INSTANCES, dtype, MAIN_SEED + 1)
        x2 = transforms(MAIN_INSTANCES, dtype, MAIN_SEED + 2)
        sc = ir.Scene(trees, of, x, dtype)
        planes = np.ascontiguousarray(np.concatenate([rr.random_regions(sc.w, MAIN_REGIONS, MAIN_SEED + 3),
                                                      cutting_regions(sc, MAIN_CUT, MAIN_SEED + 4, 6)]))
        _main[key] = dict(trees=trees, tree_of=of, x=x, x2=x2, scene=sc, planes=planes, ref=reference(sc, planes))
    return _main[key]
