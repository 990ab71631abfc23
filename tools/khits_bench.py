"""Multi-hit rays on the scene of sphere clusters: khits_batch (bvhgpu_traverse_khits_*) against the closest-hit queries on the same tree and
rays — forced to the binary walk, which is the same walk without a list, and at default dispatch — and against what a caller does today: the
CSR copied to the host and reduced there with khits_ref.khits_match.  tools/sphere_bench.py's scene and protocol: f32 and f64, wall clock of
whole synchronising calls after warm-up, median of --reps, the legs alternated inside one process.

  python tools/khits_bench.py [--reps 9] [--host-reps 3] [--rays 1000000] [--clusters 10000] [--dtypes f32,f64] [--ks 1,4,16,64]
                              [--out profiles/khits_bench.json]

Workload: `--clusters` clusters of 12 overlapping spheres in [-1e3, 1e3]^3, the tree built from the spheres' AABBs; rays from [-2e3, 2e3]^3
aimed at a cluster (a tenth in random directions); no segment end (tmax None: every hit along the ray is a candidate).  Rays in HBM, results
left in HBM.  Legs:
  khits_<leaf>_k<k>        khits_batch, leaf sphere and box;
  closest_<leaf>_binary    closest_sphere_hits / closest_box_hits with BVHGPU_TUNE_TRAVERSE_VARIANT = 0, nothing fetched;
  closest_<leaf>_default   the same at default dispatch;
  csr_host_<leaf>_k4       traverse_batch fetched to the host (with t-slices for box), the records and khits_match there (--host-reps calls).
The khits rows of k = 4 are checked against khits_match on the CSR of the same rays.  Prints one JSON line per leg and dtype."""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, RayBatch
    from khits_ref import candidate_counts, khits_match
    from sphere_ref import cluster_scene, list_hits
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
        trees = {}
        for walk, tune in (("binary", {0: 0}), ("default", {})):
            ctx = Context(0)
            for k, v in tune.items():
                ctx.set_tuning(k, v)
            trees[walk] = Bvh.from_aabbs(aabbs, ctx).flatten()
            trees[walk].set_spheres(spheres)
        flat = trees["default"]
        dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
        rb = RayBatch.from_device(dev, n, dtype)

        def host_reduce(leaf):
            off, idx, ts, _ = flat.traverse_batch(rb, want_t=(leaf == "box"))
            rec = ts if leaf == "box" else list_hits(off, idx, rays, spheres)
            return off, idx, rec, khits_match(off, idx, rec, None, 4)

        legs, common = {}, dict(dtype=dn, rays=n, spheres=len(spheres))
        for leaf in ("sphere", "box"):
            off, idx, rec, want = host_reduce(leaf)
            c = candidate_counts(off, rec)
            common.update({"csr_hits": int(off[-1]), f"{leaf}_candidates_mean": round(float(c.mean()), 3), f"{leaf}_candidates_max": int(c.max()),
                           f"{leaf}_rays_over_4": round(float((c > 4).mean()), 4)})
            vals, shape = flat.khits_batch(rb, 4, leaf)
            assert vals.cpu().numpy().tobytes() == want[0].tobytes(), f"{dn} {leaf}: values differ from the definition"
            assert shape.cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes(), f"{dn} {leaf}: shapes differ from the definition"
            for k in [int(x) for x in args.ks.split(",")]:
                legs[f"khits_{leaf}_k{k}"] = (lambda leaf=leaf, k=k: flat.khits_batch(rb, k, leaf))
            ask = {w: (t.closest_sphere_hits if leaf == "sphere" else t.closest_box_hits) for w, t in trees.items()}
            legs[f"closest_{leaf}_binary"] = (lambda ask=ask: ask["binary"](rb, None, fetch=False))
            legs[f"closest_{leaf}_default"] = (lambda ask=ask: ask["default"](rb, None, fetch=False))
        times = {name: [] for name in legs}
        for fn in legs.values():                                          # warm-up
            fn(); fn()
        for _ in range(args.reps):                                        # the legs alternated
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for leaf in ("sphere", "box"):
            ts = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host_reduce(leaf)
                ts.append((time.perf_counter() - t0) * 1e3)
            times[f"csr_host_{leaf}_k4"] = ts
        for name, ts in times.items():
            rec = dict(common, leg=name, ms=round(float(np.median(ts)), 4), best_ms=round(float(min(ts)), 4), calls=len(ts))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
