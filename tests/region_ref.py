"""CPU checker for convex-region (plane-set) batches (a helper module, not collected by pytest).

Restates the definition of bvhgpu_region_* (include/bvh_mi355x.h) in numpy, in the tree's dtype: <FlatBvh as BoundingHierarchy>::traverse
(src/flat_bvh.rs:396-431) with the corner test in place of intersects_aabb.  Region q is m planes (nx, ny, nz, d); a box [lo, hi] passes
when for every plane
    p[k] = (n[k] >= 0) ? hi[k] : lo[k];   s = ((n0*p0 + n1*p1) + n2*p2) + d;   s >= 0
and lies wholly inside when the same sums with the opposite corner are all >= 0.
  walk      all regions in lockstep over the oracle's FlatNode array, one entry per iteration (query_ref.walk's shape)
  walk_one  the same loop for one region, entry by entry in plain Python
  brute     every shape whose own box passes, in shape order (equals the walk's row as a SET on trees without empty child bounds)
  scan      the kernel's schedule (bvh_amd/csrc/region.hip) on the CPU: the array cut into chunks, a window of entries per step, the
            exclusive prefix maximum of the failing inner entries' exits, the ancestor table at a chunk's start.  Window, chunk and table
            size are parameters, so a change to the schedule can be checked against `walk` without a GPU.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
MAX_PLANES = 32


def _sums(planes: np.ndarray, lo: np.ndarray, hi: np.ndarray, far: bool) -> np.ndarray:
    """planes (r, m, 4) against boxes [lo, hi] (r, 3) → the sums s (r, m), every operation in the planes' dtype"""
    nn, d = planes[:, :, :3], planes[:, :, 3]
    ge = nn >= 0                                               # -0 → True (hi), NaN → False (lo)
    a, b = (hi, lo) if far else (lo, hi)
    p = np.where(ge, a[:, None, :], b[:, None, :])
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = nn[:, :, 0] * p[:, :, 0], nn[:, :, 1] * p[:, :, 1], nn[:, :, 2] * p[:, :, 2]
        return ((x + y) + z) + d


def predicate(planes: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """does box r pass region r: bool (r,); m = 0 passes, a NaN sum is a miss"""
    with np.errstate(invalid="ignore"):
        return (_sums(planes, lo, hi, True) >= 0).all(axis=1)


def inside(planes: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """does box r lie wholly inside region r (the opposite corner passes every plane): bool (r,)"""
    with np.errstate(invalid="ignore"):
        return (_sums(planes, lo, hi, False) >= 0).all(axis=1)


def _planes_in(planes, ft) -> np.ndarray:
    p = np.ascontiguousarray(planes, dtype=ft)
    if p.ndim == 2:
        p = p[None]
    assert p.ndim == 3 and p.shape[2] == 4 and p.shape[1] <= MAX_PLANES, p.shape
    return p


def walk(flat: np.ndarray, shape_aabbs: np.ndarray, planes) -> tuple:
    """the lockstep walk → (offsets[n+1] u32, indices u32, inside u8), region q's shapes in the crate's order"""
    ft = flat["min"].dtype
    pl = _planes_in(planes, ft)
    n = len(pl)
    boxes = np.ascontiguousarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    mn, mx = flat["min"], flat["max"]
    entry, exit_, shape = flat["entry"].astype(np.int64), flat["exit"].astype(np.int64), flat["shape"].astype(np.int64)
    idx = np.zeros(n, dtype=np.int64)
    hits, ins = [[] for _ in range(n)], [[] for _ in range(n)]
    while len(flat):
        live = np.nonzero(idx < len(flat))[0]
        if len(live) == 0:
            break
        i = idx[live]
        leaf = entry[i] == NONE
        lo, hi = mn[i].copy(), mx[i].copy()
        if leaf.any():   # leaf entries test the shape's own AABB (flat_bvh.rs:411-418)
            sb = boxes[shape[i[leaf]]]
            lo[leaf], hi[leaf] = sb[:, :3], sb[:, 3:]
        ok = predicate(pl[live], lo, hi)
        rep = np.nonzero(leaf & ok)[0]
        if len(rep):
            wi = inside(pl[live[rep]], lo[rep], hi[rep])
            for j, w in zip(rep, wi):
                hits[live[j]].append(int(shape[i[j]]))
                ins[live[j]].append(int(w))
        idx[live] = np.where(leaf, exit_[i], np.where(ok, entry[i], exit_[i]))
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(h) for h in hits], dtype=np.uint64).astype(np.uint32)
    indices = np.array([s for h in hits for s in h], dtype=np.uint32)
    flags = np.array([s for h in ins for s in h], dtype=np.uint8)
    return offsets, indices, flags


def walk_one(flat: np.ndarray, shape_aabbs: np.ndarray, planes) -> list:
    """the same loop for ONE region, entry by entry in plain Python (flat_bvh.rs:404-430) — the cross-check of `walk`"""
    ft = flat["min"].dtype
    pl = _planes_in(planes, ft)[:1]
    boxes = np.asarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    out, i = [], 0
    while i < len(flat):
        node = flat[i]
        if int(node["entry"]) == NONE:
            b = boxes[int(node["shape"])]
            if predicate(pl, b[None, :3], b[None, 3:])[0]:
                out.append(int(node["shape"]))
            i = int(node["exit"])
        elif predicate(pl, node["min"][None, :], node["max"][None, :])[0]:
            i = int(node["entry"])
        else:
            i = int(node["exit"])
    return out


def brute(shape_aabbs: np.ndarray, planes, ft) -> np.ndarray:
    """the shapes whose own box passes ONE region, ascending shape index"""
    pl = _planes_in(planes, ft)[:1]
    boxes = np.ascontiguousarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    return np.nonzero(predicate(np.repeat(pl, len(boxes), axis=0), boxes[:, :3], boxes[:, 3:]))[0]


# ---- the kernel's schedule ------------------------------------------------------------------------------------------------------------
def entries(flat: np.ndarray, shape_aabbs: np.ndarray, folded: bool) -> dict:
    """the array the kernel walks, as columns: lo, hi (E, 3), exit (E), leaf (E), shape (E).  folded=False: the FlatNode array entry for
    entry, a leaf entry carrying the shape's own box (the UNFOLDED rule).  folded=True: the engine's `trav` array — a leaf's navigator
    entry and its leaf entry become ONE entry with the shape's box (a single-shape tree keeps its one entry)."""
    ft = flat["min"].dtype
    boxes = np.ascontiguousarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    leaf = flat["entry"] == NONE
    lo, hi = flat["min"].copy(), flat["max"].copy()
    sh = flat["shape"].astype(np.int64)
    lo[leaf], hi[leaf] = boxes[sh[leaf], :3], boxes[sh[leaf], 3:]
    ex = flat["exit"].astype(np.int64)
    if not folded or len(flat) <= 1:
        return dict(lo=lo, hi=hi, exit=ex, leaf=leaf, shape=sh)
    keep = np.ones(len(flat), dtype=bool)
    keep[np.nonzero(leaf)[0] - 1] = False                      # the navigator entry in front of every leaf entry goes
    new = np.concatenate([np.cumsum(keep) - 1, [keep.sum()]])  # old index → new index (of the entry itself, or of the next kept one)
    new[np.nonzero(~keep)[0]] = new[np.nonzero(~keep)[0] + 1]  # a dropped navigator is its leaf
    return dict(lo=lo[keep], hi=hi[keep], exit=new[ex[keep]], leaf=leaf[keep], shape=sh[keep])


def ancestors(ent: dict, s: int) -> list:
    """the inner entries a < s with exit_a > s, root first: the descent of k_region_ancestors (follows `exit` only)"""
    out, i = [], 0
    while i < s:
        ex = int(ent["exit"][i])
        if not ent["leaf"][i] and ex > s:
            out.append(i)
            i += 1
        else:
            i = max(ex, i + 1)
    return out


def scan(ent: dict, planes, window: int = 64, chunk: int = 1024, anc_max: int = 64, units: list = None) -> list:
    """ONE region by the kernel's schedule → its row.  units (optional list): gets one dict per chunk — count, killed (a failing
    ancestor's exit reached the chunk end), deep (the ancestor path was longer than the table)."""
    ft = ent["lo"].dtype
    pl = _planes_in(planes, ft)[:1]
    E = len(ent["exit"])
    row = []
    for s in range(0, E, chunk):
        e = min(s + chunk, E)
        anc = ancestors(ent, s)
        skip = s
        if len(anc) <= anc_max:      # one gather step: every ancestor tested, the failing ones' largest exit
            if anc:
                a = np.array(anc)
                ok = predicate(np.repeat(pl, len(a), axis=0), ent["lo"][a], ent["hi"][a])
                if (~ok).any():
                    skip = max(skip, int(ent["exit"][a[~ok]].max()))
        else:                        # the serial descent: the first failing ancestor has the largest exit
            for a in anc:
                if not predicate(pl, ent["lo"][a][None], ent["hi"][a][None])[0]:
                    skip = int(ent["exit"][a])
                    break
        killed = skip >= e
        count, i = 0, skip
        while i < e:
            idx = np.arange(i, min(i + window, e))
            ok = predicate(np.repeat(pl, len(idx), axis=0), ent["lo"][idx], ent["hi"][idx])
            leaf = ent["leaf"][idx]
            ex = np.where(~leaf & ~ok, ent["exit"][idx], 0)
            incl = np.maximum.accumulate(ex)
            excl = np.concatenate([[0], incl[:-1]])
            live = idx >= np.maximum(excl, skip)
            rep = idx[live & leaf & ok]
            row.extend(int(v) for v in ent["shape"][rep])
            count += len(rep)
            skip = max(skip, int(incl[-1]))
            i = max(i + window, skip)
        if units is not None:
            units.append(dict(count=count, killed=killed, deep=len(anc) > anc_max))
    return row


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def oracle_tree(shape_aabbs: np.ndarray):
    """build + flatten with the oracle: the FlatNode array"""
    from oracle import orc
    a = np.ascontiguousarray(shape_aabbs).reshape(-1, 6)
    return orc.flatten(orc.build(a).nodes)


def random_regions(aabbs: np.ndarray, n: int, seed: int, max_planes: int = 6, pad_to: int = None, cut: int = 0) -> np.ndarray:
    """n regions of 1 .. max_planes random planes through points in the middle 80 % of the scene's bounds, padded with (0, 0, 0, 0)
    planes to pad_to (default max_planes) planes each: (n + cut, pad_to, 4) in the boxes' dtype.
    cut: that many MORE regions behind them, drawn the same way except that plane 0 passes through the centre of a randomly chosen shape's
    box and the other planes are turned to keep that centre inside — so that the region reports shapes it does not wholly contain (in a
    scene of unit cubes in bounds of +-1e5 a random plane cuts a shape in about one region of a hundred)."""
    rng = np.random.default_rng(seed)
    a = np.asarray(aabbs, dtype=np.float64).reshape(-1, 6)
    lo, hi = a[:, :3].min(axis=0), a[:, 3:].max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    m = pad_to or max_planes
    out = np.zeros((n + cut, m, 4), dtype=np.float64)
    for q in range(n + cut):
        centre = None
        if q >= n:
            b = a[int(rng.integers(0, len(a)))]
            centre = (b[:3] + b[3:]) / 2
        for j in range(int(rng.integers(1, max_planes + 1))):
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            pt = mid + half * 0.8 * rng.uniform(-1, 1, size=3)
            if centre is not None:
                if j == 0:
                    pt = centre
                elif np.dot(nrm, centre - pt) < 0:
                    nrm = -nrm
            out[q, j, :3] = nrm
            out[q, j, 3] = -np.dot(nrm, pt)
    return out.astype(np.asarray(aabbs).dtype)


BALL_REGIONS, BALL_SEED = 300, 12


def ball_regions(aabbs: np.ndarray, n: int, seed: int, planes: int = MAX_PLANES) -> np.ndarray:
    """n regions of `planes` REAL planes each, tangent to a ball: centre in the middle 60 % of the scene's bounds, radius 20 - 60 % of the
    half extent, unit normals drawn at random and pointing at the centre.  Every region holds its centre, so the rows are not empty where
    shapes are, and each plane cuts off a cap of its own: (n, planes, 4) in the boxes' dtype."""
    rng = np.random.default_rng(seed)
    a = np.asarray(aabbs, dtype=np.float64).reshape(-1, 6)
    lo, hi = a[:, :3].min(axis=0), a[:, 3:].max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    out = np.zeros((n, planes, 4), dtype=np.float64)
    for q in range(n):
        c = mid + half * 0.6 * rng.uniform(-1, 1, size=3)
        r = float(half.min()) * rng.uniform(0.2, 0.6)
        nrm = rng.normal(size=(planes, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        out[q, :, :3] = nrm
        out[q, :, 3] = r - nrm @ c                       # n.(x - (c - r n)) >= 0
    return out.astype(np.asarray(aabbs).dtype)


MAIN_CUBES, MAIN_REGIONS, MAIN_CUT, MAIN_SEED = 900, 40, 24, 11
_main = {}


def main_scene(dtype) -> dict:
    """the scene the GPU test runs and tests/test_region_cpu.py qualifies: 900 cubes (10 800 shapes), MAIN_REGIONS random regions and
    MAIN_CUT cutting ones, and the definition's rows — computed once per dtype and shared: dict(aabbs, flat, planes, off, idx, ins)"""
    key = np.dtype(dtype).name
    if key not in _main:
        from oracle import orc
        _, a = orc.create_n_cubes(MAIN_CUBES)
        a = np.ascontiguousarray(a.astype(dtype))
        flat = oracle_tree(a)
        planes = random_regions(a, MAIN_REGIONS, MAIN_SEED, cut=MAIN_CUT)
        off, idx, ins = walk(flat, a, planes)
        _main[key] = dict(aabbs=a, flat=flat, planes=planes, off=off, idx=idx, ins=ins)
    return _main[key]


def chain_flat(shape_aabbs: np.ndarray) -> np.ndarray:
    """a FlatNode array (flat_bvh.rs:60-143) of a right-leaning chain over the shapes in index order: node k = (leaf k, the rest).  Its
    last leaf has n - 1 ancestors (the n - 2 inner navigators and its own) — a path longer than the kernel's ancestor table from 66
    shapes on, which no built tree of test size has."""
    from oracle import orc
    a = np.ascontiguousarray(shape_aabbs).reshape(-1, 6)
    ft = a.dtype
    n = len(a)
    dt = orc.FLAT_F32 if ft == np.float32 else orc.FLAT_F64
    suffix_lo = np.minimum.accumulate(a[::-1, :3], axis=0)[::-1]   # the join of shapes k ..
    suffix_hi = np.maximum.accumulate(a[::-1, 3:], axis=0)[::-1]
    out = []

    def leaf_pair(k, at):        # navigator + leaf entry of shape k
        out.append((a[k, :3], a[k, 3:], at + 1, at + 2, NONE))
        out.append((np.full(3, np.inf, ft), np.full(3, -np.inf, ft), NONE, at + 2, k))

    total = 3 * n - 2
    for k in range(n - 1):
        leaf_pair(k, len(out))
        if k < n - 2:            # the navigator of the inner node "shapes k + 1 .."
            out.append((suffix_lo[k + 1], suffix_hi[k + 1], len(out) + 1, total, NONE))
    if n == 1:
        out.append((np.full(3, np.inf, ft), np.full(3, -np.inf, ft), NONE, 1, 0))
    else:
        leaf_pair(n - 1, len(out))
    flat = np.zeros(len(out), dtype=dt)
    for i, (lo, hi, en, ex, sh) in enumerate(out):
        flat[i]["min"], flat[i]["max"], flat[i]["entry"], flat[i]["exit"], flat[i]["shape"] = lo, hi, en, ex, sh
    assert len(flat) == total
    return flat
