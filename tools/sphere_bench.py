"""Sphere-hit rays on a scene of sphere clusters: closest_sphere_hits / first_sphere_hits (bvhgpu_traverse_sphere_*) against the box queries on
the same tree and rays (the same walk with a cheaper leaf stage) and against what a caller of the reference's examples/simple.rs does today —
the CSR copied to the host and the ray-sphere test run over it there.  tools/box_bench.py's protocol: f32 and f64, each walk forced and the
default; wall clock of whole synchronising calls after warm-up, median of --reps.

  python tools/sphere_bench.py [--legs sphere,box,csr] [--reps 9] [--rays 1000000] [--clusters 10000] [--dtypes f32,f64]
                               [--walks binary,...,default] [--out profiles/sphere_bench.json]

Workload: tests/sphere_ref.py's scene at bench size — `--clusters` clusters of 12 overlapping spheres (r in [0.3, 0.8]) in [-1e3, 1e3]^3, the
tree built from the spheres' AABBs; rays from [-2e3, 2e3]^3 aimed at a cluster (a tenth in random directions); tmax = the nearest sphere
distance x U(0.3, 1.7).  Legs:
  sphere  closest_sphere_hits and first_sphere_hits with that tmax (rays and tmax in HBM, nothing fetched); each result is checked against
          sphere_ref.sphere_match on the CSR of the same rays;
  box     closest_box_hits and first_box_hits on the same tree, rays and tmax;
  csr     traverse_batch fetched to the host plus sphere_ref.sphere_match (closest) there.
The box and csr legs use nothing the sphere entry points added: with tests/sphere_ref.py beside it this tool also runs from a checkout that
predates them (--legs box,csr).  Prints one JSON line per leg, dtype and walk."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NONE = 0xFFFFFFFF
WALKS = [("binary", {0: 0}), ("binary_lds", {0: 2, 3: 0}), ("wide_whole", {0: 3, 1: 0}), ("wide_items", {0: 3, 1: 2}), ("default", {})]


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
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="sphere,box,csr")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--walks", default=",".join(w for w, _ in WALKS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch

    from bvh_amd import Bvh, Context, RayBatch
    from sphere_ref import cluster_scene, sphere_match, tmax_draw
    records = []
    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        centres, spheres = cluster_scene(dtype, args.clusters)
        r = spheres[:, 3:4]
        aabbs = np.ascontiguousarray(np.concatenate([spheres[:, :3] - r, spheres[:, :3] + r], axis=1))   # (= bvh_amd.spheres_aabbs)
        rng = np.random.default_rng(0)
        n = args.rays
        o = rng.uniform(-2e3, 2e3, size=(n, 3)).astype(dtype)
        target = centres[rng.integers(0, len(centres), size=n)] + rng.uniform(-0.8, 0.8, size=(n, 3))
        d = (target - o).astype(dtype)
        d[: n // 10] = rng.normal(size=(n // 10, 3))
        host = RayBatch.new(o, d, dtype)
        rays = host.host
        flat0 = Bvh.from_aabbs(aabbs, Context(0)).flatten()
        off, idx, _, _ = flat0.traverse_batch(host)
        nearest = sphere_match(off, idx, rays, spheres, None, False)
        tmax = tmax_draw(rng, nearest[0][:, 0], dtype)
        want = {first: sphere_match(off, idx, rays, spheres, tmax, first) for first in (False, True)}
        common = dict(dtype=dn, rays=n, spheres=len(spheres), csr_hits=int(off[-1]), rays_hitting_a_sphere=round(float((nearest[1] != NONE).mean()), 4),
                      rays_with_a_candidate=round(float((want[False][1] != NONE).mean()), 4))
        dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
        rb = RayBatch.from_device(dev, n, dtype)
        tdev = torch.from_numpy(tmax.copy()).cuda()
        for walk, tune in [w for w in WALKS if w[0] in args.walks.split(",")]:
            ctx = Context(0)
            for k, v in tune.items():
                ctx.set_tuning(k, v)
            flat = Bvh.from_aabbs(aabbs, ctx).flatten()
            recs = []
            if "sphere" in legs:
                flat.set_spheres(spheres)
                for name, first in (("sphere_closest", False), ("sphere_first", True)):
                    ask = flat.first_sphere_hits if first else flat.closest_sphere_hits
                    ms, best = timed(lambda: ask(rb, tdev, fetch=False), args.reps, torch)
                    kernel = flat.query_kernel()
                    hit, shape = ask(rb, tdev)
                    assert hit.tobytes() == want[first][0].tobytes() and np.array_equal(shape, want[first][1]), f"{dn} {walk} {name}: differs from the definition"
                    recs.append(dict(leg=name, ms=ms, best_ms=best, kernel=kernel))
            if "box" in legs:
                for name, first in (("box_closest", False), ("box_first", True)):
                    ask = flat.first_box_hits if first else flat.closest_box_hits
                    ms, best = timed(lambda: ask(rb, tdev, fetch=False), args.reps, torch)
                    recs.append(dict(leg=name, ms=ms, best_ms=best, kernel=flat.query_kernel()))
            if "csr" in legs:
                def by_hand():
                    o_, i_, _, _ = flat.traverse_batch(rb)
                    return sphere_match(o_, i_, rays, spheres, tmax, False)
                ms, best = timed(by_hand, args.reps, torch)
                kernel = flat.query_kernel()
                ms_walk, _ = timed(lambda: flat.traverse_batch(rb, fetch=False), args.reps, torch)
                recs.append(dict(leg="csr_plus_numpy", ms=ms, best_ms=best, kernel=kernel, of_which_device_ms=ms_walk))
            for r_ in recs:
                rec = dict(common, walk=walk, **r_)
                records.append(rec)
                print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
