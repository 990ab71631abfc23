"""Box-hit rays on configs[1]'s scene (create_n_cubes(10000): 120 000 triangle boxes): closest_box_hits / first_box_hits
(bvhgpu_traverse_box_*) against what gives a comparable answer without them — closest_hits / any_hits with triangles set, and the CSR with
t-slices copied to the host and reduced there with numpy.  f32 and f64, each walk forced and the default; wall clock of whole synchronising
calls after warm-up, median of --reps.

  python tools/box_bench.py [--legs box,tri,csr] [--reps 9] [--rays 1000000] [--dtypes f32,f64] [--walks binary,...,default] [--out profiles/box_bench.json]

Workload: tools/any_bench.py's re-aimed stream — the bench stream's rays (create_ray, seed 0) keep their origins and are aimed at the centre
of a random cube (seeded, +-0.6 jitter).  tmax is drawn around the nearest box entry (x U(0.3, 1.7), 2e5 where the ray meets no box), from
the CSR with t-slices of the same rays, so that every leg and every checkout of the repository sees the same segments.  Legs:
  box  closest_box_hits and first_box_hits with that tmax (rays and tmax in HBM, nothing fetched); each result is checked against the
       definition applied to the CSR with t-slices;
  tri  closest_hits and any_hits(tmax) on the same rays with the cubes' triangles set;
  csr  traverse_batch(want_t=True) fetched to the host plus the numpy reduction to one record per ray (closest): what a caller without the
       box entry points has to do.
The tri and csr legs use nothing the box entry points added, so they also run from a checkout that predates them.  Prints one JSON line per
leg, dtype and walk."""
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


def box_match(off, idx, ts, tmax, first):
    """(a copy of tests/test_box_hit_cpu.py's box_match, kept in step with it: this tool also runs from a checkout that predates that file)
    the definition on a CSR with t-slices → (slice[n,2], shape[n]): candidates enter before tmax (strict); closest: the smallest entry,
    the first of the row on ties; first: the first of the row"""
    n = len(off) - 1
    counts = np.diff(off.astype(np.int64))
    total = len(ts)
    starts = off[:-1].astype(np.int64)
    rows = counts > 0
    with np.errstate(invalid="ignore"):
        ok = ts[:, 0] < np.repeat(np.asarray(tmax, dtype=ts.dtype), counts)
    if not first and total:
        masked = np.where(ok, ts[:, 0], np.inf).astype(ts.dtype)
        rowmin = np.full(n, np.inf, dtype=ts.dtype)
        rowmin[rows] = np.minimum.reduceat(masked, starts[rows])
        ok &= ts[:, 0] == np.repeat(rowmin, counts)
    pos = np.where(ok, np.arange(total), total)
    win = np.full(n, total, dtype=np.int64)
    if total:
        win[rows] = np.minimum.reduceat(pos, starts[rows])
    found = win < total
    out = np.zeros((n, 2), dtype=ts.dtype)
    out[:, 0] = np.inf
    out[found] = ts[win[found]]
    shape = np.full(n, NONE, dtype=np.uint32)
    shape[found] = idx[win[found]]
    return out, shape


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
    ap.add_argument("--legs", default="box,tri,csr")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--walks", default=",".join(w for w, _ in WALKS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch

    from bvh_amd import Bvh, Context, RayBatch, testbase as tb
    from oracle import orc
    tris32, aabbs32 = tb.create_n_cubes(10_000)
    records = []
    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        tris, aabbs = tris32.astype(dtype), aabbs32.astype(dtype)
        rng = np.random.default_rng(0)
        centres = tris.reshape(-1, 36, 3).astype(np.float64).mean(axis=1)
        stream = orc.create_rays(0, args.rays, dtype=dtype)   # = bvhgpu_gen_rays_* (tests/test_abi_cpu.py)
        target = centres[rng.integers(0, len(centres), size=len(stream))] + rng.uniform(-0.6, 0.6, size=(len(stream), 3))
        host = RayBatch.new(stream["o"], (target - stream["o"].astype(np.float64)).astype(dtype), dtype)
        n = host.n
        flat0 = Bvh.from_aabbs(aabbs, Context(0)).flatten()
        off, idx, ts, _ = flat0.traverse_batch(host, want_t=True)
        nearest = box_match(off, idx, ts, np.full(n, np.inf, dtype), False)[0][:, 0].astype(np.float64)
        tmax = (np.where(np.isfinite(nearest), nearest, 2e5) * rng.uniform(0.3, 1.7, size=n)).astype(dtype)
        want = {first: box_match(off, idx, ts, tmax, first) for first in (False, True)}
        common = dict(dtype=dn, rays=n, csr_hits=int(off[-1]), rays_with_a_box=round(float((off[1:] > off[:-1]).mean()), 4),
                      rays_with_a_candidate=round(float((want[False][1] != NONE).mean()), 4))
        dev = torch.from_numpy(np.ascontiguousarray(host.host).view(np.uint8).copy()).cuda()
        rb = RayBatch.from_device(dev, n, dtype)
        tdev = torch.from_numpy(tmax.copy()).cuda()
        for walk, tune in [w for w in WALKS if w[0] in args.walks.split(",")]:
            ctx = Context(0)
            for k, v in tune.items():
                ctx.set_tuning(k, v)
            flat = Bvh.from_aabbs(aabbs, ctx).flatten()
            recs = []
            if "box" in legs:
                for name, first in (("box_closest", False), ("box_first", True)):
                    ask = flat.first_box_hits if first else flat.closest_box_hits
                    ms, best = timed(lambda: ask(rb, tdev, fetch=False), args.reps, torch)
                    kernel = flat.query_kernel()
                    sl, shape = ask(rb, tdev)
                    assert sl.tobytes() == want[first][0].tobytes() and np.array_equal(shape, want[first][1]), f"{dn} {walk} {name}: differs from the definition"
                    recs.append(dict(leg=name, ms=ms, best_ms=best, kernel=kernel))
            if "csr" in legs:
                def by_hand():
                    o, i, t, _ = flat.traverse_batch(rb, want_t=True)
                    return box_match(o, i, t, tmax, False)
                ms, best = timed(by_hand, args.reps, torch)
                kernel = flat.query_kernel()
                ms_walk, _ = timed(lambda: flat.traverse_batch(rb, want_t=True, fetch=False), args.reps, torch)
                recs.append(dict(leg="csr_t_slice_plus_numpy", ms=ms, best_ms=best, kernel=kernel, of_which_device_ms=ms_walk))
            if "tri" in legs:
                flat.set_triangles(tris)
                ms, best = timed(lambda: flat.closest_hits(rb, fetch=False), args.reps, torch)
                recs.append(dict(leg="triangle_closest", ms=ms, best_ms=best, kernel=flat.query_kernel()))
                ms, best = timed(lambda: flat.any_hits(rb, tdev, fetch=False), args.reps, torch)
                recs.append(dict(leg="triangle_any", ms=ms, best_ms=best, kernel=flat.query_kernel()))
            for r in recs:
                rec = dict(common, walk=walk, **r)
                records.append(rec)
                print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
