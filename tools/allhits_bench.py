"""All-hits rays on the scene of sphere clusters: allhits_batch (bvhgpu_traverse_allhits_*), sorted and in list order, against the only
device-side way to get whole rows before it — khits_batch with a k that holds every row of this scene (k = 16 and k = 64: at most 20
candidates per ray) — against the plain binary walk (closest_*_hits with BVHGPU_TUNE_TRAVERSE_VARIANT = 0), and against what a caller does
today: the CSR copied to the host and reduced there with allhits_ref.allhits_match.  tools/khits_bench.py's scene and protocol: f32 and f64,
wall clock of whole synchronising calls after warm-up, median of --reps, the legs alternated inside one process.

  python tools/allhits_bench.py [--reps 9] [--host-reps 3] [--rays 1000000] [--clusters 10000] [--dtypes f32,f64] [--out profiles/allhits_bench.json]

Workload: `--clusters` clusters of 12 overlapping spheres in [-1e3, 1e3]^3, the tree built from the spheres' AABBs; rays from [-2e3, 2e3]^3
aimed at a cluster (a tenth in random directions); no segment end.  Rays in HBM, results left in HBM.  Legs:
  allhits_<leaf>_sorted    allhits_batch, leaf sphere and box (the CSR fetched into torch tensors on the device);
  allhits_<leaf>_list      the same with sort=False (BVHGPU_ALLHITS_LIST_ORDER);
  khits_<leaf>_k<k>        khits_batch, k = 16 and 64;
  closest_<leaf>_binary    closest_sphere_hits / closest_box_hits on the binary walk, nothing fetched: one walk without a list;
  csr_host_<leaf>          traverse_batch fetched to the host (with t-slices for box), the records and allhits_match there (--host-reps calls).
The sorted rows are checked against allhits_match on the CSR of the same rays and, head by head, against khits_batch k = 64.  Prints one
JSON line per leg and dtype."""
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, RayBatch
    from allhits_ref import allhits_match, head_rows
    from khits_ref import candidate_counts
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
            return off, idx, rec, allhits_match(off, idx, rec, None, True)

        legs, common = {}, dict(dtype=dn, rays=n, spheres=len(spheres))
        for leaf in ("sphere", "box"):
            off, idx, rec, want = host_reduce(leaf)
            c = candidate_counts(off, rec)
            common.update({"csr_hits": int(off[-1]), f"{leaf}_candidates_mean": round(float(c.mean()), 3), f"{leaf}_candidates_max": int(c.max()),
                           f"{leaf}_rays_over_4": round(float((c > 4).mean()), 4)})
            o, s, v = flat.allhits_batch(rb, leaf)
            o, s, v = o.cpu().numpy().astype(np.uint32), s.cpu().numpy().view(np.uint32), v.cpu().numpy()
            assert o.tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes(), f"{dn} {leaf}: rows differ from the definition"
            assert v.tobytes() == want[2].tobytes(), f"{dn} {leaf}: values differ from the definition"
            kv, ks = flat.khits_batch(rb, 64, leaf)
            hv, hs = head_rows(o, s, v, 64)
            assert kv.cpu().numpy().tobytes() == hv.tobytes() and ks.cpu().numpy().view(np.uint32).tobytes() == hs.tobytes(), f"{dn} {leaf}: khits k = 64 differs"
            common[f"{leaf}_total"] = int(o[-1])
            legs[f"allhits_{leaf}_sorted"] = (lambda leaf=leaf: flat.allhits_batch(rb, leaf))
            legs[f"allhits_{leaf}_list"] = (lambda leaf=leaf: flat.allhits_batch(rb, leaf, None, False))
            for k in (16, 64):
                legs[f"khits_{leaf}_k{k}"] = (lambda leaf=leaf, k=k: flat.khits_batch(rb, k, leaf))
            ask = {w: (t.closest_sphere_hits if leaf == "sphere" else t.closest_box_hits) for w, t in trees.items()}
            legs[f"closest_{leaf}_binary"] = (lambda ask=ask: ask["binary"](rb, None, fetch=False))
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
            times[f"csr_host_{leaf}"] = ts
        for name, ts in times.items():
            rec = dict(common, leg=name, ms=round(float(np.median(ts)), 4), best_ms=round(float(min(ts)), 4), calls=len(ts))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
