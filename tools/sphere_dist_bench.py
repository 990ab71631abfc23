"""The sphere kind of the point families (bvhgpu_knearest_sphere_* / _knearest_tree_sphere_* / _within_sphere_*) beside kinds
0 (the shape's box) and 1 (its triangle) of the unsuffixed entries, on configs[1]'s scene (create_n_cubes(10000): 120 000 shapes) with the
sphere inscribed in every shape box, 1 M points in HBM drawn uniformly over the scene's bounds (fixed seed), f32 and f64.

  python tools/sphere_dist_bench.py [--points 1000000] [--dtypes f32,f64] [--ks 1,8,64] [--mean 20] [--samples 10] [--warmup 3]

Queries: knearest and knearest_tree at every k of --ks; within (sorted rows) at the radius whose mean SPHERE row over a 20 000-point
sample is about --mean (bisection with COUNT_ONLY), the same radius for all three kinds — their mean rows are reported.
Timing: the host clock around one call that ends in a device synchronise; the three kinds of one query take turns call by call in this
process, --warmup calls each first, then --samples samples each: median and range in ms.  One JSON line per query."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating(legs, warmup, samples, sync):
    """legs: {name: callable}; -> {name: sorted list of ms}"""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
            sync()
    out = {name: [] for name in legs}
    for _ in range(samples):
        for name, fn in legs.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return {name: sorted(v) for name, v in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--mean", type=float, default=20.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, testbase as tb
    tris32, aabbs32 = tb.create_n_cubes(10_000)
    lo, hi = aabbs32[:, :3].min(axis=0).astype(np.float64), aabbs32[:, 3:].max(axis=0).astype(np.float64)
    n = args.points
    pts64 = np.random.default_rng(0).uniform(lo, hi, size=(n, 3))
    sync = torch.cuda.synchronize

    def emit(rec, times):
        for name, v in times.items():
            rec[name + "_ms"] = round(float(np.median(v)), 4)
            rec[name + "_range_ms"] = [round(v[0], 4), round(v[-1], 4)]
        rec["sphere_over_box"] = round(rec["sphere_ms"] / rec["box_ms"], 3)
        rec["sphere_over_triangle"] = round(rec["sphere_ms"] / rec["triangle_ms"], 3)
        print(json.dumps(rec), flush=True)

    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        aabbs = aabbs32.astype(dtype)
        bvh = Bvh.from_aabbs(aabbs, Context(0))
        bvh.set_triangles(tris32.astype(dtype))
        c = (aabbs[:, :3] + aabbs[:, 3:]) * dtype(0.5)
        r = (aabbs[:, 3:] - aabbs[:, :3]).min(axis=1) * dtype(0.5)
        bvh.set_spheres(np.ascontiguousarray(np.concatenate([c, r[:, None]], axis=1)))
        flat = bvh.flatten()
        tp = torch.from_numpy(pts64.astype(dtype)).cuda()
        base = dict(dtype=dn, n=n, samples=args.samples, warmup=args.warmup)
        for k in [int(v) for v in args.ks.split(",")]:
            emit(dict(base, what="knearest", k=k),
                 alternating({"box": lambda: flat.knearest_batch(tp, k), "triangle": lambda: flat.knearest_batch(tp, k, triangles=True),
                              "sphere": lambda: flat.knearest_sphere_batch(tp, k)}, args.warmup, args.samples, sync))
            emit(dict(base, what="knearest_tree", k=k),
                 alternating({"box": lambda: bvh.knearest_tree_batch(tp, k), "triangle": lambda: bvh.knearest_tree_batch(tp, k, triangles=True),
                              "sphere": lambda: bvh.knearest_tree_sphere_batch(tp, k)}, args.warmup, args.samples, sync))
        sample = tp[:: max(1, n // 20_000)].contiguous()
        rlo, rhi = 1e-3, float((hi - lo).max())
        for _ in range(40):                                   # the count is monotonic in the radius
            radius = float(np.sqrt(rlo * rhi))
            off, _, _ = flat.within_sphere_batch(sample, radius, count_only=True)
            mean = float(off[-1].item()) / (len(off) - 1)
            if abs(mean - args.mean) <= 0.03 * args.mean:
                break
            rlo, rhi = (radius, rhi) if mean < args.mean else (rlo, radius)
        legs = {"box": lambda: flat.within_batch(tp, radius), "triangle": lambda: flat.within_batch(tp, radius, triangles=True),
                "sphere": lambda: flat.within_sphere_batch(tp, radius)}
        rec = dict(base, what="within", radius=round(radius, 5))
        for name, fn in legs.items():
            off = fn()[0]
            rec[name + "_mean_row"] = round(float(off[-1].item()) / n, 3)
            rec[name + "_max_row"] = int((off[1:] - off[:-1]).max().item())
        emit(rec, alternating(legs, args.warmup, args.samples, sync))


if __name__ == "__main__":
    main()
