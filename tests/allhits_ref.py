"""The definition of the all-hits ray query bvhgpu_traverse_allhits_* (include/bvh_mi355x.h) applied to a CSR, and the
single-row scenes its tests share.  A member of ray i's list is a candidate iff its record's first scalar — the distance — is < tmax[i]
(strict, in T); row i is ALL candidates, in a stable ascending sort by distance (sort=True) or in list order (sort=False: the engine's
BVHGPU_ALLHITS_LIST_ORDER); the output is a CSR without padding.  tests/test_allhits_cpu.py pins allhits_match on hand-made rows, against
khits_ref.khits_match and the scenes on the oracle; tests/test_gpu_allhits.py compares the GPU against it byte for byte;
tools/allhits_bench.py times it as the host reduction a caller runs today."""
import numpy as np


def allhits_match(off, idx, records, tmax, sort=True):
    """the definition on a CSR (offsets, indices of FlatBvh::traverse's lists) and the per-member records[total, W] (distance first) →
    (offsets[n + 1] u32, shape[total'] u32, vals[total', W])"""
    n = len(off) - 1
    records = np.asarray(records)
    T = records.dtype
    counts = np.diff(off.astype(np.int64))
    row = np.repeat(np.arange(n), counts)
    t = np.full(n, np.inf, dtype=T) if tmax is None else np.asarray(tmax, dtype=T)
    dist = records[:, 0]
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(dist < t[row])[0]                               # strict, in T: a miss (+inf) and a NaN tmax admit nothing
    if sort:
        cand = cand[np.lexsort((dist[cand], row[cand]))]                  # by row, then distance; stable: equal distances keep list order
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row[cand], minlength=n), out=offsets[1:])
    assert offsets[-1] <= 0xFFFFFFFF
    return offsets.astype(np.uint32), np.ascontiguousarray(idx[cand], dtype=np.uint32), np.ascontiguousarray(records[cand])


def head_rows(offsets, shape, vals, k):
    """the first min(k, len) entries of every row as bvhgpu_traverse_khits_* lays them out: (vals[n, k, W], shape[n, k]) with its padding"""
    n = len(offsets) - 1
    o = offsets.astype(np.int64)
    lens = np.diff(o)
    W = vals.shape[1]
    out_v = np.zeros((n, k, W), dtype=vals.dtype)
    out_v[:, :, 0] = np.inf
    out_s = np.full((n, k), 0xFFFFFFFF, dtype=np.uint32)
    row = np.repeat(np.arange(n), lens)
    rank = np.arange(len(shape)) - np.repeat(o[:-1], lens)
    keep = rank < k
    out_v[row[keep], rank[keep]] = vals[keep]
    out_s[row[keep], rank[keep]] = shape[keep]
    return out_v, out_s


# ---- the single row: P positions p = 8 j along x, one shape each, every coordinate an integer below 2^24 (exact in f32) -----------------
def single_row(dtype, P, reverse=False):
    """dict(aabbs[P, 6], spheres[P, 4], tris[P, 3, 3]): box j = [8j, -1, -1 | 8j + 2, 1, 1], sphere j = {(8j + 1, 0, 0), 1}, and one triangle
    per position in the plane x = 8j, inside the box's face, whose front faces the rays of length_rays(..., reverse): toward -x, or toward
    +x with reverse (the leaf stage culls back faces).  A ray along the x axis has one candidate per position, for every leaf kind."""
    p = 8.0 * np.arange(P)
    aabbs = np.stack([p, -np.ones(P), -np.ones(P), p + 2, np.ones(P), np.ones(P)], axis=1).astype(dtype)
    spheres = np.stack([p + 1, np.zeros(P), np.zeros(P), np.ones(P)], axis=1).astype(dtype)
    tri = np.array([[0, 0, 1], [0, 1, -1], [0, -1, -1]], dtype=np.float64)      # front face toward -x (khits_ref.triangle_row's small one)
    if reverse:
        tri = tri[[0, 2, 1]]
    tris = np.tile(tri, (P, 1, 1))
    tris[:, :, 0] = p[:, None]
    return dict(aabbs=aabbs, spheres=spheres, tris=tris.astype(dtype))


def length_rays(orc, dtype, lengths, reverse=False, P=4096):
    """(rays, tmax) on single_row(dtype, P, reverse): ray r has exactly lengths[r] candidates, for the box, the sphere and the triangle stage.
    Forward: from x = -10 - (r mod 32) along +x; position j is met at 8j + 10 + (r mod 32) and tmax[r] = 8 m + 6 + (r mod 32) admits
    j < m (m = 0: tmax = 0).  reverse: from x = 8P + 100 + (r mod 32) along -x; the box and the sphere of position j are entered at
    8 (P - j) + 98 + (r mod 32), its triangle is met 2 later, and tmax[r] = 8 m + 102 + (r mod 32) admits j >= P - m — the LAST m members of
    the list, which comes in descending distance."""
    m = np.asarray(lengths, dtype=np.int64)
    assert m.min() >= 0 and m.max() <= P and 8 * P + 131 < 2 ** 24
    i = (np.arange(len(m)) % 32).astype(np.float64)
    o = np.zeros((len(m), 3))
    d = np.zeros((len(m), 3))
    if reverse:
        o[:, 0], d[:, 0] = 8 * P + 100 + i, -1
        tmax = 8.0 * m + 102 + i
    else:
        o[:, 0], d[:, 0] = -10 - i, 1
        tmax = 8.0 * m + 6 + i
    tmax[m == 0] = 0
    return orc.make_rays(o.astype(dtype), d.astype(dtype), dtype), tmax.astype(dtype)


def tier_lengths(lane_max, lds_max, P=4096):
    """the row lengths that cross every tier boundary of allhits.hip: every m in 0..300, 2^j - 1, 2^j, 2^j + 1 for j = 9..12 (capped at P),
    and both thresholds +-1"""
    ms = list(range(301))
    for j in range(9, 13):
        ms += [min(2 ** j + e, P) for e in (-1, 0, 1)]
    for t in (lane_max, lds_max):
        ms += [min(max(t + e, 0), P) for e in (-1, 0, 1) if min(max(t + e, 0), P) not in ms]
    return np.asarray(ms, dtype=np.int64)


def pair_row(dtype, P):
    """khits_ref.nested_pair_row's geometry at P positions: spheres[2P, 4] and their boxes — index 2j is {c = (8j + 3, 0, 0), r = 3}, index
    2j + 1 {c = (8j + 1, 0, 0), r = 1}; both start at x = 8j, so a ray along +x meets the pair at one distance"""
    p = 8.0 * np.arange(P)
    s = np.zeros((2 * P, 4))
    s[0::2, 0], s[0::2, 3] = p + 3, 3
    s[1::2, 0], s[1::2, 3] = p + 1, 1
    s = s.astype(dtype)
    aabbs = np.concatenate([s[:, :3] - s[:, 3:], s[:, :3] + s[:, 3:]], axis=1).astype(dtype)
    return s, aabbs


def pair_row_rays(orc, dtype, P):
    """khits_ref.row_rays for P positions: 32 rays from x = -10 - i along +x, then 32 from x = 8P + 100 + i along -x"""
    i = np.arange(32, dtype=np.float64)
    o = np.zeros((64, 3))
    o[:32, 0] = -10 - i
    o[32:, 0] = 8 * P + 100 + i
    d = np.zeros((64, 3))
    d[:32, 0] = 1
    d[32:, 0] = -1
    return orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)


def engine_thresholds(root):
    """(ALLHITS_LANE_ROW_MAX, ALLHITS_LDS_ROW_MAX) as bvh_amd/csrc/allhits.hip names them"""
    import os
    import re
    src = open(os.path.join(root, "bvh_amd", "csrc", "allhits.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1)) for name in ("ALLHITS_LANE_ROW_MAX", "ALLHITS_LDS_ROW_MAX"))
