"""Host cost of the Python layer: wall clock of the whole synchronising call for a batch so small that Python dominates — 256 host rays
(or points) on configs[1]'s scene (create_n_cubes(10000): 120 000 triangles), f32.  Median and minimum of --calls calls after --warmup,
in microseconds, for traverse_batch, closest_hits, any_hits with a tmax array, khits_batch(k=8) and within_batch on the tree, and for
closest_hits, khits_batch(k=8), within_batch and region_batch on an Instances set of two instances of that tree.

  python tools/api_overhead_bench.py [--calls 300] [--warmup 30] [--n 256] [--label new] [--out runs.json] [--root other/checkout]

The device work of a call does not depend on the host layers (bvh_amd/*.py, csrc/capi.hip), so two runs of this file differ by what those
do on the host; compare a change of them as parent / new / parent in one session on one machine (--label names the run, --out appends
its record to a JSON list, --root is the built checkout whose bvh_amd is measured: this file's own by default, so one copy of the tool
measures both).  Prints one JSON line.  profiles/api_marshal_overhead.json was put together by hand from such records (the *_median
fields, as *_us) and the `value` and `ms_per_step` of the default bench.py line of the same runs; profiles/host_layers_overhead.json is
the --out file of one such session as it is."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(ts)), 2), round(float(min(ts)), 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    from bvh_amd import Bvh, Context, Instances, RayBatch, aabb_planes, testbase as tb
    tris, aabbs = tb.create_n_cubes(10_000)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    rng = np.random.default_rng(0)
    centres = tris.reshape(-1, 36, 3).mean(axis=1)
    origins = rng.uniform(lo, hi, size=(args.n, 3)).astype(np.float32)
    targets = centres[rng.integers(0, len(centres), size=args.n)]       # every ray is aimed at a cube, so the leaf stages have work
    ctx = Context(0)
    flat = Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    rays = RayBatch.new(origins, (targets - origins).astype(np.float32), np.float32, ctx)
    tmax = np.linalg.norm(targets - origins, axis=1).astype(np.float32)
    points = (targets + rng.uniform(-1, 1, size=(args.n, 3))).astype(np.float32)
    max_dist = np.full(args.n, 4.0, dtype=np.float32)
    shift = np.array([0.0, 0.0, float(hi[2] - lo[2]) + 10.0])
    pose = np.stack([np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([np.eye(3), shift[:, None]])]).astype(np.float32)
    inst = Instances([flat], [0, 0], pose, ctx)                         # the scene and a copy of it beside it
    planes = np.stack([aabb_planes(p - 4.0, p + 4.0, np.float32) for p in points])
    cases = {
        "traverse_batch": lambda: flat.traverse_batch(rays),
        "closest_hits": lambda: flat.closest_hits(rays),
        "any_hits_tmax": lambda: flat.any_hits(rays, tmax),
        "khits_batch_k8": lambda: flat.khits_batch(rays, 8, "triangle"),
        "within_batch": lambda: flat.within_batch(points, max_dist),
        "instances_closest_hits": lambda: inst.closest_hits(rays),
        "instances_khits_batch_k8": lambda: inst.khits_batch(rays, 8),
        "instances_within_batch": lambda: inst.within_batch(points, max_dist),
        "instances_region_batch": lambda: inst.region_batch(planes),
    }
    rec = dict(label=args.label, n=args.n, calls=args.calls, unit="us")
    for name, fn in cases.items():
        rec[name + "_median"], rec[name + "_min"] = timed(fn, args.calls, args.warmup)
    inst.close()
    print(json.dumps(rec), flush=True)
    if args.out:
        runs = json.load(open(args.out)) if os.path.exists(args.out) else []
        with open(args.out, "w") as f:
            json.dump(runs + [rec], f, indent=1)


if __name__ == "__main__":
    main()
