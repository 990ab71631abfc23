"""Radius-search point queries (bvhgpu_within_*) on configs[1]'s scene (create_n_cubes(10000): 120 000 triangles), on tools/knn_bench.py's
protocol: 1 M points in HBM ("bounds" and "surface" clouds, fixed seeds), both shape distances, f32 and f64; a timing is the wall clock of
the whole synchronising call; the legs of one configuration take turns call by call in one process, after 2 warm-up calls each, median
of --reps (3 repetitions after 1 warm-up call where a leg's first call takes more than --slow-ms).

  python tools/within_bench.py [--reps 9] [--points 1000000] [--dtypes f32,f64] [--means 2,20,200] [--kinds 0,1] [--out profiles/r16_within_bench.json]

Radii: per cloud and shape distance, the scalar max_dist at which the mean row length of a 20 000-point sample is about 2, 20 and 200
(bisection on the radius with BVHGPU_WITHIN_COUNT_ONLY); the achieved mean and maximum of the whole batch are reported.

Legs (all on the same points and the same radius):
  within_sorted / within_list / within_count   within_batch, the default rows, BVHGPU_WITHIN_LIST_ORDER, BVHGPU_WITHIN_COUNT_ONLY
  ball                                         query_batch("ball"), result left in HBM: one walk, boxes only, no distances, no order
  knn_tree64                                   knearest_tree_batch(k = 64, max_dist): rows longer than 64 are cut (cut_rows says how many)
  host (shape distance 0, --host-points points) the ball CSR fetched, distances computed, filtered and sorted with numpy on the host, against
                                               within_batch on the same subset; once, not a median"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from knn_bench import timed_alternating  # noqa: E402


def calibrate(flat, sample, kind, target, lo, hi):
    """the radius in [lo, hi] at which the sample's mean row length is about `target` (the count is monotonic in the radius)"""
    for _ in range(40):
        mid = float(np.sqrt(lo * hi))
        off, _, _ = flat.within_batch(sample, mid, triangles=bool(kind), count_only=True)
        mean = float(off[-1].item()) / (len(off) - 1)
        if abs(mean - target) <= 0.03 * target:
            return mid
        if mean < target:
            lo = mid
        else:
            hi = mid
    return float(np.sqrt(lo * hi))


def host_reduce(off, idx, aabbs, pts, r):
    """what a caller of the ball query does today for shape distance 0: Aabb::min_distance_squared of every member, filter, stable sort"""
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    b, p = aabbs[idx], pts[rows]
    half = (b[:, 3:] - b[:, :3]) * aabbs.dtype.type(0.5)
    q = np.abs(p - (b[:, :3] + half)) - half
    q = np.where(q > 0, q, aabbs.dtype.type(0))
    d2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]
    keep = d2 <= r * r
    rows, d2, idx = rows[keep], d2[keep], idx[keep]
    order = np.lexsort((d2, rows))                           # stable: by row, then by distance, ties in list order
    counts = np.bincount(rows, minlength=len(off) - 1)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), idx[order], np.sqrt(d2[order])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--host-points", type=int, default=100_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--means", default="2,20,200")
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, testbase as tb
    tris32, aabbs32 = tb.create_n_cubes(10_000)
    lo, hi = aabbs32[:, :3].min(axis=0).astype(np.float64), aabbs32[:, 3:].max(axis=0).astype(np.float64)
    n = args.points
    rng = np.random.default_rng(0)
    clouds = {"bounds": rng.uniform(lo, hi, size=(n, 3)),
              "surface": tris32[rng.integers(0, len(tris32), n)].astype(np.float64).mean(axis=1) + rng.uniform(-0.5, 0.5, size=(n, 3))}
    means = [float(v) for v in args.means.split(",")]
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)

    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        ctx = Context(0)
        aabbs = aabbs32.astype(dtype)
        flat = Bvh.from_aabbs(aabbs, ctx).flatten()
        flat.set_triangles(tris32.astype(dtype))
        for cloud, pts in clouds.items():
            host_pts = pts.astype(dtype)
            tp = torch.from_numpy(host_pts).cuda()
            sample = tp[:: max(1, n // 20_000)].contiguous()
            for kind in [int(k) for k in args.kinds.split(",")]:
                for target in means:
                    r = calibrate(flat, sample, kind, target, 1e-3, float((hi - lo).max()))
                    off, _, _ = flat.within_batch(tp, r, triangles=bool(kind), count_only=True)
                    lens = (off[1:] - off[:-1])
                    total, longest = int(off[-1].item()), int(lens.max().item())
                    balls = torch.cat([tp, torch.full((n, 1), r, dtype=tp.dtype, device=tp.device)], dim=1).contiguous()
                    legs = {"within_sorted": lambda: flat.within_batch(tp, r, triangles=bool(kind)),
                            "within_list": lambda: flat.within_batch(tp, r, triangles=bool(kind), sort=False),
                            "within_count": lambda: flat.within_batch(tp, r, triangles=bool(kind), count_only=True),
                            "ball": lambda: flat.query_batch("ball", balls, fetch=False),
                            "knn_tree64": lambda: flat.knearest_tree_batch(tp, 64, triangles=bool(kind), max_dist=r)}
                    med, best, reps = timed_alternating(list(legs.values()), args.reps, args.slow_ms)
                    o, s, d = flat.within_batch(tp[:4096].contiguous(), r, triangles=bool(kind))
                    rows = torch.repeat_interleave(torch.arange(4096, device=o.device), (o[1:] - o[:-1]))
                    same_row = rows[1:] == rows[:-1]
                    assert bool((d[1:][same_row] >= d[:-1][same_row]).all()), "a row is not ascending"
                    flat.query_batch("ball", balls, fetch=False)
                    ball_total = flat._hits.info()["total"]
                    rec = dict(what="within", dtype=dn, points=cloud, n=n, kind=kind, target_mean=target, radius=round(r, 5),
                               mean_row=round(total / n, 3), max_row=longest, total=total, rows_over_32=int((lens > 32).sum().item()),
                               rows_over_2048=int((lens > 2048).sum().item()), cut_rows=int((lens > 64).sum().item()), ball_total=int(ball_total),
                               reps=reps)
                    for name, m, b in zip(legs, med, best):
                        rec[name + "_ms"] = round(m, 4)
                        rec[name + "_best_ms"] = round(b, 4)
                    rec["sorted_over_list"] = round(med[0] / med[1], 3)
                    rec["sorted_over_ball"] = round(med[0] / med[3], 3)
                    rec["mcandidates_per_s"] = round(total / med[0] * 1e-3, 1)
                    emit(rec)
                    if kind == 0 and args.host_points:
                        hn = min(args.host_points, n)
                        hp, hb = host_pts[:hn], np.concatenate([host_pts[:hn], np.full((hn, 1), r, dtype)], axis=1)
                        t0 = time.perf_counter()
                        bo, bi = flat.query_batch("ball", hb)
                        got = host_reduce(np.asarray(bo), np.asarray(bi), aabbs, hp, dtype(r))
                        host_ms = (time.perf_counter() - t0) * 1e3
                        flat.within_batch(hp, r)
                        t0 = time.perf_counter()
                        wo, ws, wd = flat.within_batch(hp, r)
                        dev_ms = (time.perf_counter() - t0) * 1e3
                        emit(dict(what="host_reduce", dtype=dn, points=cloud, n=hn, kind=0, target_mean=target, radius=round(r, 5),
                                  host_ms=round(host_ms, 3), within_host_memory_ms=round(dev_ms, 3), host_over_within=round(host_ms / dev_ms, 1),
                                  offsets_equal=bool(np.array_equal(got[0], wo)), distances_equal=bool(got[2].tobytes() == wd.tobytes())))


if __name__ == "__main__":
    main()
