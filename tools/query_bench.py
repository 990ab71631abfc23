"""AABB / point / ball query batches on configs[1]'s scene (create_n_cubes(10000): 120 000 triangles), f32 and f64, each batch with each
walk forced (BVHGPU_TUNE_QUERY_VARIANT 0 = binary, 1 = wide): device-synchronised wall clock after warm-up, median of --reps.

  python tools/query_bench.py [--reps 7] [--sizes 256,1000,4000,16000,64000,250000,1000000] [--out profiles/query_bench.json]

Batches: self-overlap (120 k AABB queries = the shapes' own boxes), 1 M seeded random small boxes, 1 M seeded points, 1 M seeded balls;
then the small-box / point / ball batches at the sizes of --sizes (the crossover that sets knob 22's default).  Every timed pair
is checked: both walks return byte-equal CSR.  Prints ms, queries/s and hits/s per walk, one JSON line per batch."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOB = 22


def seeded(kind: str, n: int, aabbs: np.ndarray, dtype, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    c = rng.uniform(lo, hi, size=(n, 3))
    near = rng.integers(0, len(aabbs), size=n // 2)   # half of them near a random shape (the cubes fill little of the volume)
    b = aabbs[near].astype(np.float64)
    c[:n // 2] = (b[:, :3] + b[:, 3:]) * 0.5 + rng.normal(size=(n // 2, 3)) * (b[:, 3:] - b[:, :3])
    if kind == "point":
        return c.astype(dtype)
    e = rng.uniform(0.0, 0.01, size=(n, 3)) * (hi - lo)   # up to 1 % of the scene per half-extent
    if kind == "aabb":
        return np.concatenate([c - e, c + e], axis=1).astype(dtype)
    return np.concatenate([c, e[:, :1]], axis=1).astype(dtype)


def time_batch(bvh, kind, q, reps, torch):
    """device-resident queries, fetch=False: the call returns when the CSR is complete in HBM (it synchronises the stream)"""
    for _ in range(2):
        bvh.query_batch(kind, q, fetch=False)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bvh.query_batch(kind, q, fetch=False)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="256,1000,4000,16000,64000,250000,1000000")
    ap.add_argument("--out", default="")
    ap.add_argument("--dtypes", default="f32,f64")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, testbase as tb
    ctx = Context(0)
    _, base = tb.create_n_cubes(10_000)
    records = []
    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        aabbs = base.astype(dtype)
        bvh = Bvh.from_aabbs(aabbs, ctx)
        bvh.flatten_in_place()
        batches = [("self", "aabb", None)]
        for kind in ("aabb", "point", "ball"):
            batches.append((f"{kind}_1M", kind, seeded(kind, 1_000_000, aabbs, dtype, 1)))
        for size in [int(s) for s in args.sizes.split(",") if s]:
            if size == 1_000_000:
                continue
            for kind in ("aabb", "point", "ball"):
                batches.append((f"{kind}_{size}", kind, seeded(kind, size, aabbs, dtype, 2)))
        for name, kind, qh in batches:
            q = None if qh is None else torch.from_numpy(qh).cuda()
            n = len(aabbs) if qh is None else len(qh)
            rec = dict(dtype=dn, batch=name, kind=kind, queries=n)
            csr = []
            for knob, walk in ((0, "binary"), (1, "wide")):
                ctx.set_tuning(KNOB, knob)
                ms, best = time_batch(bvh, kind, q, args.reps, torch)
                off, idx = bvh.query_batch(kind, q)
                csr.append((off.tobytes(), idx.tobytes()))
                rec[walk] = dict(ms=round(ms, 4), best_ms=round(best, 4), queries_per_s=round(n / (ms * 1e-3)),
                                 hits_per_s=round(len(idx) / (ms * 1e-3)), kernel=bvh.query_kernel())
                rec["hits"] = int(len(idx))
            ctx.set_tuning(KNOB, -1)
            assert csr[0] == csr[1], f"{dn} {name}: the two walks differ"
            rec["wide_over_binary"] = round(rec["binary"]["ms"] / rec["wide"]["ms"], 3)
            records.append(rec)
            print(json.dumps(rec), flush=True)
        bvh.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
