"""Frustum culling with region_batch against the only thing a caller could do before it: query_batch("aabb") on the frusta's bounding boxes.

Scenes: create_n_cubes(10 000) (BASELINE.json configs[1]: 120 k triangles) and create_n_cubes(1 000 000) (12 M triangles).  Batches of 1, 6,
64 and 3 456 frusta whose eyes sit on a sphere of three half-extents around the scene and look at its centre; the field of view is found
by bisection so that a frustum sees about 1 %, 10 % and 50 % of the shapes.  Planes and boxes are in HBM.  Per combination:
  region        region_batch(tree, planes): count pass, scan, fill pass, offsets and indices copied to fresh tensors on the device
  region_count  the same with count_only=True
  aabb          query_batch("aabb", boxes, fetch=False) on the bounding boxes of the same frusta, and how many shapes it returns
and, for one-region batches, the bytes of the entry array over the call time as a share of the HBM peak (an upper bound of what the two
passes read: subtrees the region misses are jumped over; the 120 k scene's 3.7 MB array lives in L2 — the figure is then a rate, not an HBM share).
Host clock around calls that end in a device synchronise; warm-up, then the median, minimum and maximum of `--repeats` samples of `inner`
calls each (inner is chosen so that a sample is about 30 ms of work).  A combination whose result would exceed --max-total shapes is skipped.

    python tools/region_bench.py [--cubes 10000 1000000] [--batches 1 6 64 3456] [--fractions 0.01 0.1 0.5] [--repeats 10] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X


def eyes(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def frusta(dirs, centre, half, fov, frustum_planes):
    """(n, 6, 4) f32 planes and (n, 6) f32 bounding boxes of the frusta with eyes at centre + 3 half dirs, looking at the centre"""
    planes, boxes = [], []
    near, far = 0.05 * half, 8.0 * half
    for d in dirs:
        eye = centre + 3.0 * half * d
        up = (0.0, 1.0, 0.0) if abs(d[1]) < 0.9 else (1.0, 0.0, 0.0)
        planes.append(frustum_planes(eye, centre, up, fov, 1.0, near, far, np.float32))
        f = -d
        r = np.cross(f, up); r /= np.linalg.norm(r)
        u = np.cross(r, f)
        t = math.tan(math.radians(fov) / 2)
        corners = [eye + z * (f + sx * t * r + sy * t * u) for z in (near, far) for sx in (-1, 1) for sy in (-1, 1)]
        corners = np.array(corners)
        boxes.append(np.concatenate([corners.min(axis=0), corners.max(axis=0)]))
    return np.ascontiguousarray(np.stack(planes)), np.ascontiguousarray(np.array(boxes, dtype=np.float32))


def seen_share(planes, centres):
    s = centres @ planes[:, :3].T.astype(np.float64) + planes[:, 3].astype(np.float64)
    return float((s >= 0).all(axis=1).mean())


def fov_for(share, d, centre, half, centres, frustum_planes):
    lo, hi = 0.5, 150.0
    for _ in range(24):
        mid = (lo + hi) / 2
        p, _ = frusta([d], centre, half, mid, frustum_planes)
        if seen_share(p[0], centres) < share:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def timed(fn, sync, warmup, repeats):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    one = time.perf_counter() - t0
    inner = int(min(50, max(1, math.ceil(0.03 / max(one, 1e-6)))))
    if one > 0.5:   # (a box query on the 12 M-triangle scene takes seconds: three samples)
        repeats = min(repeats, 3)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), repeats=repeats, inner=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cubes", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 6, 64, 3456])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.01, 0.1, 0.5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--max-total", type=int, default=150_000_000, help="skip a combination that would return more shapes than this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, frustum_planes, region_batch, testbase as tb
    if bvh_amd.device_count() <= 0:
        raise SystemExit("region_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
    ctx = Context(0)
    res = dict(warmup=a.warmup, repeats=a.repeats, scenes=[])
    for cubes in a.cubes:
        _, aabbs = tb.create_n_cubes(cubes)
        n_shapes = len(aabbs)
        lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
        centre, half = (lo + hi) / 2, float((hi - lo).max()) / 2
        rng = np.random.default_rng(0)
        sample = aabbs[rng.integers(0, n_shapes, size=min(n_shapes, 200_000))].astype(np.float64)
        centres = (sample[:, :3] + sample[:, 3:]) / 2
        tree = Bvh.from_aabbs(aabbs, ctx).flatten()
        n_trav = max(2 * n_shapes - 2, 1)
        scene = dict(cubes=cubes, shapes=n_shapes, entries=n_trav, entry_bytes=n_trav * 32, rows=[])
        dirs = eyes(max(a.batches), 1)
        for share in a.fractions:
            fov = fov_for(share, dirs[0], centre, half, centres, frustum_planes)
            for nb in a.batches:
                planes, boxes = frusta(dirs[:nb], centre, half, fov, frustum_planes)
                tp, tb_ = torch.from_numpy(planes).cuda(), torch.from_numpy(boxes).cuda()
                row = dict(share_wanted=share, fov_deg=fov, regions=nb)
                try:
                    r = region_batch(tree, tp, count_only=True)
                except bvh_amd.BvhGpuError as e:      # (more than 2^32 - 1 shapes in one batch)
                    row["skipped"] = str(e)
                    scene["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    continue
                total = int(r["offsets"][-1].item())
                row.update(region_total=total, chunks=r["chunks"], chunk_entries=r["chunk_entries"], share_seen=total / (nb * n_shapes))
                if total > a.max_total:
                    row["skipped"] = "more shapes than --max-total"
                    scene["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    continue
                row["region_count"] = timed(lambda: region_batch(tree, tp, count_only=True), ctx.synchronize, a.warmup, a.repeats)
                row["region"] = timed(lambda: region_batch(tree, tp), ctx.synchronize, a.warmup, a.repeats)
                row["region_classify"] = timed(lambda: region_batch(tree, tp, classify=True), ctx.synchronize, a.warmup, a.repeats)
                try:
                    tree.query_batch("aabb", tb_, fetch=False)
                    aabb_total = tree._hits.info()["total"]
                    row["aabb_total"] = aabb_total
                    row["aabb_over_region"] = aabb_total / max(total, 1)
                    row["aabb"] = timed(lambda: tree.query_batch("aabb", tb_, fetch=False), ctx.synchronize, a.warmup, a.repeats)
                except bvh_amd.BvhGpuError as e:
                    row["aabb_error"] = str(e)
                if nb == 1:   # what the count and fill passes read at most (both walk the whole entry array once), over the call time
                    rate = 2 * scene["entry_bytes"] / (row["region"]["median_ms"] * 1e-3)
                    row["entry_bytes_x2_per_s"] = rate
                    row["share_of_hbm_peak_upper_bound"] = rate / HBM_PEAK_BYTES_PER_S
                scene["rows"].append(row)
                print(json.dumps(row), flush=True)
        res["scenes"].append(scene)
        tree.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
