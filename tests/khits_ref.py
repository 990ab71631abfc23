"""The definition of the multi-hit ray query bvhgpu_traverse_khits_* (include/bvh_mi355x.h) applied to a CSR, and the
row scenes its tests share.  A member of ray i's list is a candidate iff its record's first scalar — the distance — is < tmax[i] (strict,
in T); row i is the candidates in a stable ascending sort by distance, cut to the first k; the other slots hold NONE and {+inf, 0[, 0]}.
tests/test_khits_cpu.py pins khits_match on hand-made rows and the scenes on the oracle; tests/test_gpu_khits.py compares the GPU against
it byte for byte; tools/khits_bench.py times it as the host reduction a caller runs today."""
import numpy as np

NONE = 0xFFFFFFFF


def khits_match(off, idx, records, tmax, k):
    """the definition on a CSR (offsets, indices of FlatBvh::traverse's lists) and the per-member records[total, W] (distance first) →
    (vals[n, k, W], shape[n, k])"""
    n = len(off) - 1
    records = np.asarray(records)
    T, W = records.dtype, records.shape[1]
    counts = np.diff(off.astype(np.int64))
    row = np.repeat(np.arange(n), counts)
    t = np.full(n, np.inf, dtype=T) if tmax is None else np.asarray(tmax, dtype=T)
    dist = records[:, 0]
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(dist < t[row])[0]                               # strict, in T: a miss (+inf) and a NaN tmax admit nothing
    order = cand[np.lexsort((dist[cand], row[cand]))]                     # by row, then distance; stable: equal distances keep list order
    r = row[order]
    first = np.searchsorted(r, r, side="left")                            # where the row's candidates start in `order`
    rank = np.arange(len(order)) - first
    keep = rank < k
    vals = np.zeros((n, k, W), dtype=T)
    vals[:, :, 0] = np.inf
    shape = np.full((n, k), NONE, dtype=np.uint32)
    vals[r[keep], rank[keep]] = records[order[keep]]
    shape[r[keep], rank[keep]] = idx[order[keep]]
    return vals, shape


def candidate_counts(off, records, tmax=None):
    """candidates per ray"""
    n = len(off) - 1
    counts = np.diff(off.astype(np.int64))
    t = np.full(n, np.inf, dtype=records.dtype) if tmax is None else np.asarray(tmax, dtype=records.dtype)
    with np.errstate(invalid="ignore"):
        ok = records[:, 0] < np.repeat(t, counts)
    return np.bincount(np.repeat(np.arange(n), counts)[ok], minlength=n)


# ---- row scenes: 100 positions p = 8 j along x, two shapes each, rays along the row from both ends ---------------------------------------
ROW_POSITIONS = 100


def row_rays(orc, dtype, z=0.0):
    """32 rays from x = -10 - i along +x, then 32 from x = 900 + i along -x, y = 0"""
    i = np.arange(32, dtype=np.float64)
    o = np.zeros((64, 3))
    o[:32, 0] = -10 - i
    o[32:, 0] = 900 + i
    o[:, 2] = z
    d = np.zeros((64, 3))
    d[:32, 0] = 1
    d[32:, 0] = -1
    return orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)


def nested_pair_row(dtype):
    """spheres[200, 4] and their boxes c -/+ r: index 2j is {c = (p+3, 0, 0), r = 3}, index 2j+1 {c = (p+1, 0, 0), r = 1} — both start at
    x = p, so a ray along +x meets the pair at one distance, for the box and for the sphere stage"""
    p = 8.0 * np.arange(ROW_POSITIONS)
    s = np.zeros((2 * ROW_POSITIONS, 4))
    s[0::2, 0], s[0::2, 3] = p + 3, 3
    s[1::2, 0], s[1::2, 3] = p + 1, 1
    s = s.astype(dtype)
    aabbs = np.concatenate([s[:, :3] - s[:, 3:], s[:, :3] + s[:, 3:]], axis=1).astype(dtype)
    return s, aabbs


def triangle_row(dtype, alternate=False):
    """tris[200, 3, 3] and their boxes: per position two coplanar triangles in the plane x = p, index 2j (p,1,5), (p,5,-3), (p,-3,-3) and
    index 2j+1 (p,0,1), (p,1,-1), (p,-1,-1), front face toward -x.  alternate: the winding of every odd position is reversed (b and c
    swapped), so those face +x"""
    p = 8.0 * np.arange(ROW_POSITIONS)
    big = np.array([[0, 1, 5], [0, 5, -3], [0, -3, -3]], dtype=np.float64)
    small = np.array([[0, 0, 1], [0, 1, -1], [0, -1, -1]], dtype=np.float64)
    tris = np.zeros((2 * ROW_POSITIONS, 3, 3))
    tris[0::2] = big
    tris[1::2] = small
    tris[:, :, 0] = np.repeat(p, 2)[:, None]
    if alternate:
        odd = (np.arange(2 * ROW_POSITIONS) // 2) % 2 == 1
        tris[odd] = tris[odd][:, [0, 2, 1]]
    tris = tris.astype(dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1).astype(dtype)
    return tris, aabbs
