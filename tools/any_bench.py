"""Shadow rays on configs[1]'s scene (create_n_cubes(10000): 120 000 triangles): any_hits (bvhgpu_traverse_any_*) against closest_hits on
the same segments, f32 and f64, each walk forced and the default; device-synchronised wall clock after warm-up, median of --reps.

  python tools/any_bench.py [--reps 7] [--shadow 1000000] [--dtypes f32,f64] [--walks binary,...,default] [--out profiles/any_bench.json]

Workload: the bench stream itself (create_ray, seed 0) almost never meets a triangle of this sparse scene (7 closest hits in its first
50 M rays), so its rays keep their origins and are re-aimed at the centre of a random cube (seeded, +-0.6 jitter); closest_hits gives
the hit points, chunks of 1 M rays until --shadow of them are collected.  From each hit point a ray is aimed at a fixed point light above
the scene's bounds, with tmax = the distance to the light (Ray::new normalises the direction).  Every timed any-hit result is checked against the definition applied to the TRIANGLES output (per-candidate
Intersection, CSR order) of the same rays: the first candidate with distance < tmax.  Prints one JSON line per dtype and walk, with the
occluded fraction."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE = 0xFFFFFFFF
WALKS = [("binary", {0: 0}), ("binary_lds", {0: 2, 3: 0}), ("wide_whole", {0: 3, 1: 0}), ("wide_items", {0: 3, 1: 2}), ("default", {})]


def first_match(off, idx, isect, tmax):
    """per CSR row the first j with isect[j, 0] < tmax[row] → shape[n] (NONE: not occluded)"""
    n = len(off) - 1
    counts = np.diff(off.astype(np.int64))
    total = len(isect)
    ok = isect[:, 0] < np.repeat(np.asarray(tmax, dtype=isect.dtype), counts)
    pos = np.where(ok, np.arange(total), total)
    first = np.full(n, total, dtype=np.int64)
    rows = counts > 0
    if total:
        first[rows] = np.minimum.reduceat(pos, off[:-1].astype(np.int64)[rows])
    shape = np.full(n, NONE, dtype=np.uint32)
    found = first < total
    shape[found] = idx[first[found]]
    return shape


def shadow_batch(flat, tris, dtype, n_shadow, bounds, torch):
    """hit points of the bench stream and the segments from them to the light: (RayBatch in HBM, tmax tensor, tmax host, stream rays used)"""
    from bvh_amd import RayBatch
    from oracle import orc
    lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
    light = np.array([(lo[0] + hi[0]) / 2, hi[1] + 0.25 * (hi[1] - lo[1]), (lo[2] + hi[2]) / 2])
    rng = np.random.default_rng(0)
    centres = tris.reshape(-1, 36, 3).astype(np.float64).mean(axis=1)
    pts, first = [], 0
    while sum(len(p) for p in pts) < n_shadow and first < 20_000_000:
        stream = orc.create_rays(first, 1_000_000, dtype=dtype)   # = bvhgpu_gen_rays_* (tests/test_abi_cpu.py)
        target = centres[rng.integers(0, len(centres), size=len(stream))] + rng.uniform(-0.6, 0.6, size=(len(stream), 3))
        rays = RayBatch.new(stream["o"], (target - stream["o"].astype(np.float64)).astype(dtype), dtype).host
        isect, shape, _ = flat.closest_hits(RayBatch(len(rays), dtype, host=rays))
        hit = shape != NONE
        p = rays["o"][hit].astype(np.float64) + isect[hit, :1].astype(np.float64) * rays["d"][hit].astype(np.float64)
        pts.append(p)
        first += 1_000_000
    p = np.concatenate(pts)[:n_shadow]
    to_light = light[None, :] - p
    rb_host = RayBatch.new(p.astype(dtype), to_light.astype(dtype), dtype)
    tmax = np.linalg.norm(to_light, axis=1).astype(dtype)
    dev = torch.from_numpy(np.ascontiguousarray(rb_host.host).view(np.uint8).copy()).cuda()
    return RayBatch.from_device(dev, len(p), dtype), dev, torch.from_numpy(tmax.copy()).cuda(), tmax, rb_host, first


def timed(fn, reps, torch):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shadow", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--walks", default=",".join(w for w, _ in WALKS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, testbase as tb
    tris32, aabbs32 = tb.create_n_cubes(10_000)
    bounds = np.concatenate([aabbs32[:, :3].min(axis=0), aabbs32[:, 3:].max(axis=0)])
    records = []
    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
        ctx0 = Context(0)
        flat0 = Bvh.from_aabbs(aabbs, ctx0).flatten()
        flat0.set_triangles(tris)
        rb, _keep, tdev, tmax, rb_host, used = shadow_batch(flat0, tris, dtype, args.shadow, bounds, torch)
        # the definition, from the TRIANGLES output of the same rays
        off, idx, isect, _ = flat0.intersect_triangles(rb_host)
        want = first_match(off, idx, isect, tmax)
        occluded = float((want != NONE).mean())
        for walk, tune in [w for w in WALKS if w[0] in args.walks.split(",")]:
            ctx = Context(0)
            for k, v in tune.items():
                ctx.set_tuning(k, v)
            flat = Bvh.from_aabbs(aabbs, ctx).flatten()
            flat.set_triangles(tris)
            ms_any, best_any = timed(lambda: flat.any_hits(rb, tdev, fetch=False), args.reps, torch)
            kernel_any = flat.query_kernel()
            _, shape = flat.any_hits(rb, tdev)
            assert np.array_equal(shape, want), f"{dn} {walk}: any_hits differs from the definition"
            ms_cl, best_cl = timed(lambda: flat.closest_hits(rb, fetch=False), args.reps, torch)
            kernel_cl = flat.query_kernel()
            rec = dict(dtype=dn, walk=walk, shadow_rays=len(tmax), stream_rays=used, occluded_fraction=round(occluded, 4),
                       any_ms=round(ms_any, 4), any_best_ms=round(best_any, 4), any_kernel=kernel_any,
                       closest_ms=round(ms_cl, 4), closest_best_ms=round(best_cl, 4), closest_kernel=kernel_cl,
                       closest_over_any=round(ms_cl / ms_any, 3), any_rays_per_s=round(len(tmax) / (ms_any * 1e-3)))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
