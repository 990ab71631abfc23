"""k-nearest point queries (bvhgpu_knearest_*) on configs[1]'s scene (create_n_cubes(10000): 120 000 triangles): time against k for two point
distributions, both shape distances, f32 and f64; and k = 1 against bvhgpu_nearest_* on the same points.

  python tools/knn_bench.py [--reps 9] [--points 1000000] [--dtypes f32,f64] [--ks 1,4,8,16,32,64] [--out profiles/knn_bench.json]
                            [--form flat|tree|both] [--radius R]
  rocprofv3 --kernel-trace --stats -d DIR -o out -- python tools/knn_bench.py --reps 1 --no-ratio      (a trace run of its own)
  python tools/knn_bench.py --summarise DIR/.../out_results.db out.md ["the command line traced"]      (its per-kernel table, one row per k)

Points (fixed seeds): "bounds" = uniform in the scene's bounds (most of them far from every shape: the bound of a full list stays loose
and the fixed-order descent prunes badly); "surface" = centroids of random triangles with a +-0.5 jitter (the use of a point cloud or a
contact query).  The points live in HBM (torch tensors in, torch tensors out); a timing is the wall clock of the whole call, which returns
when the rows are complete, after 2 warm-up calls, median of --reps.  A configuration whose first call takes more than --slow-ms runs
3 repetitions after 1 warm-up call instead.  k = 1 against bvhgpu_nearest_*: both through the C ABI on the same device buffers,
alternating in one process, bvhgpu_nearest_* followed by bvhgpu_synchronize (it does not wait on its own).

--form: "flat" (default) times bvhgpu_knearest_*, "tree" the nearest-first descent bvhgpu_knearest_tree_*, "both" the two alternating call
by call in one process (records "flat_vs_tree": both medians and tree_over_flat = tree ms / flat ms, below 1 where the tree form wins).
The tree form is also timed with a limit (radius_ms): max_dist = --radius for every point, or by default the median k = 1 distance of
the cloud for that shape distance — a typical nearest-neighbour spacing, so about half of the rows stay empty."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(db_path: str, out_path: str, command: str = "tools/knn_bench.py --reps 1 --no-ratio") -> None:
    """per-kernel table of a rocprofv3 rocpd database; k_knearest's and k_knearest_tree's launches are told apart by workgroup and LDS size (= block x k x (sizeof(T) + 4))"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute(
        "select name, workgroup_x, lds_size, count(*), sum(duration), avg(duration), min(duration), max(duration), max(vgpr_count), "
        "max(sgpr_count), max(grid_x) from kernels group by name, workgroup_x, lds_size order by name, lds_size / workgroup_x").fetchall()
    total = sum(r[4] for r in rows) or 1
    with open(out_path, "w") as f:
        f.write(f"# {command}, per kernel\n\nsource: `rocprofv3 --kernel-trace --stats` (rocpd database → `kernels` "
                "view); durations in µs; k = LDS B / (wg x 8) for `<float, ...>`, / (wg x 12) for `<double, ...>`.  Every configuration also makes one "
                "4 096-point call (the tool's ascending-rows check): that is the min column, the 1 M-point calls are the max column\n\n")
        f.write("| kernel | wg | LDS B | calls | total µs | avg µs | min µs | max µs | % | VGPR | SGPR | max grid |\n")
        f.write("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for n, wx, lds, c, s, a, mn, mx, vg, sg, gx in rows:
            short = n.split("(")[0].replace("void ", "")
            f.write(f"| `{short}` | {wx} | {lds} | {c} | {s / 1e3:.1f} | {a / 1e3:.2f} | {mn / 1e3:.2f} | {mx / 1e3:.2f} | "
                    f"{100 * s / total:.1f} | {vg} | {sg} | {gx} |\n")
    print(open(out_path).read())


def timed_alternating(fns, reps: int, slow_ms: float):
    """the protocol of timed() for several calls that take turns → ([median ms per call], [best ms per call], reps)"""
    firsts = []
    for fn in fns:
        t0 = time.perf_counter()
        fn()
        firsts.append((time.perf_counter() - t0) * 1e3)
    if max(firsts) > slow_ms:
        reps = min(reps, 3)
    else:
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts], [float(min(t)) for t in ts], reps


def timed(fn, reps: int, slow_ms: float):
    t0 = time.perf_counter()
    fn()
    first = (time.perf_counter() - t0) * 1e3
    if first > slow_ms:
        reps = min(reps, 3)
    else:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), reps


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
        summarise(*sys.argv[2:5])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--ks", default="1,4,8,16,32,64")
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--no-ratio", action="store_true")
    ap.add_argument("--form", choices=["flat", "tree", "both"], default="flat")
    ap.add_argument("--radius", type=float, default=0.0, help="max_dist of the tree form's radius column; 0 = the cloud's median k = 1 distance")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from bvh_amd import Bvh, Context, _lib, testbase as tb
    lib = _lib.load()
    tris32, aabbs32 = tb.create_n_cubes(10_000)
    lo, hi = aabbs32[:, :3].min(axis=0).astype(np.float64), aabbs32[:, 3:].max(axis=0).astype(np.float64)
    n = args.points
    rng = np.random.default_rng(0)
    clouds = {"bounds": rng.uniform(lo, hi, size=(n, 3)),
              "surface": tris32[rng.integers(0, len(tris32), n)].astype(np.float64).mean(axis=1) + rng.uniform(-0.5, 0.5, size=(n, 3))}
    ks = [int(k) for k in args.ks.split(",")]
    records = []
    for dn in args.dtypes.split(","):
        dtype = np.float32 if dn == "f32" else np.float64
        ctx = Context(0)
        flat = Bvh.from_aabbs(aabbs32.astype(dtype), ctx).flatten()
        flat.set_triangles(tris32.astype(dtype))
        for cloud, pts in clouds.items():
            tp = torch.from_numpy(pts.astype(dtype)).cuda()
            for kind in (0, 1):
                if not args.no_ratio:
                    # k = 1 against bvhgpu_nearest_*: the C ABI on the same buffers, alternating
                    s1 = torch.empty(n, dtype=torch.int32, device="cuda"); d1 = torch.empty(n, dtype=tp.dtype, device="cuda")
                    s2 = torch.empty(n, dtype=torch.int32, device="cuda"); d2 = torch.empty(n, dtype=tp.dtype, device="cuda")
                    knn = getattr(lib, f"bvhgpu_knearest_{dn}")
                    nst = getattr(lib, f"bvhgpu_nearest_{dn}")

                    def call_knn():
                        _lib.check(knn(flat._t, _lib.ptr(tp.data_ptr()), n, _lib.DEVICE, kind, 1, _lib.ptr(s1.data_ptr()), _lib.ptr(d1.data_ptr())), ctx._h)

                    def call_nearest():
                        _lib.check(nst(flat._t, _lib.ptr(tp.data_ptr()), n, _lib.DEVICE, kind, _lib.ptr(s2.data_ptr()), _lib.ptr(d2.data_ptr())), ctx._h)
                        ctx.synchronize()

                    call_knn(); call_nearest()
                    assert torch.equal(s1, s2) and torch.equal(d1.view(torch.uint8), d2.view(torch.uint8)), "k = 1 differs from bvhgpu_nearest_*"
                    ta, tb_ = [], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter(); call_knn(); ta.append((time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter(); call_nearest(); tb_.append((time.perf_counter() - t0) * 1e3)
                    rec = dict(what="k1_vs_nearest", dtype=dn, points=cloud, n=n, kind=kind, knearest_k1_ms=round(float(np.median(ta)), 4),
                               nearest_ms=round(float(np.median(tb_)), 4), ratio=round(float(np.median(ta) / np.median(tb_)), 4), reps=args.reps)
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
                if args.form != "flat":
                    radius = args.radius
                    if radius <= 0:
                        _, d1t = flat.knearest_tree_batch(tp, 1, triangles=bool(kind))
                        radius = float(d1t.median().item())
                    for k in ks:
                        calls = [lambda: flat.knearest_tree_batch(tp, k, triangles=bool(kind)),
                                 lambda: flat.knearest_tree_batch(tp, k, triangles=bool(kind), max_dist=radius)]
                        if args.form == "both":
                            calls.insert(0, lambda: flat.knearest_batch(tp, k, triangles=bool(kind)))
                        med, best, reps = timed_alternating(calls, args.reps, args.slow_ms)
                        st, dt = flat.knearest_tree_batch(tp[:4096], k, triangles=bool(kind))
                        sr, dr = flat.knearest_tree_batch(tp[:4096], k, triangles=bool(kind), max_dist=radius)
                        dd = dt.cpu().numpy()
                        assert (dd[:, 1:] >= dd[:, :-1]).all(), "a row is not ascending"
                        rec = dict(what="flat_vs_tree" if args.form == "both" else "tree_time_vs_k", dtype=dn, points=cloud, n=n, kind=kind, k=k,
                                   tree_ms=round(med[-2], 4), tree_best_ms=round(best[-2], 4), radius=round(radius, 4), radius_ms=round(med[-1], 4),
                                   radius_fill=round(float((sr != -1).float().mean().item()), 4), reps=reps,
                                   tree_mpoints_per_s=round(n / med[-2] * 1e-3, 2), mean_dist_kth=round(float(dd[:, -1].mean()), 3))
                        if args.form == "both":
                            sf, df = flat.knearest_batch(tp[:4096], k, triangles=bool(kind))
                            rec.update(flat_ms=round(med[0], 4), flat_best_ms=round(best[0], 4), tree_over_flat=round(med[1] / med[0], 4),
                                       flat_over_tree=round(med[0] / med[1], 2),
                                       sample_distances_equal=bool(torch.equal(df.view(torch.uint8), dt.view(torch.uint8))),
                                       sample_shapes_equal=bool(torch.equal(sf, st)))
                        records.append(rec)
                        print(json.dumps(rec), flush=True)
                    continue
                for k in ks:
                    ms, best, reps = timed(lambda: flat.knearest_batch(tp, k, triangles=bool(kind)), args.reps, args.slow_ms)
                    s, d = flat.knearest_batch(tp[:4096], k, triangles=bool(kind))
                    dd = d.cpu().numpy()
                    assert (dd[:, 1:] >= dd[:, :-1]).all(), "a row is not ascending"
                    rec = dict(what="time_vs_k", dtype=dn, points=cloud, n=n, kind=kind, k=k, ms=round(ms, 4), best_ms=round(best, 4), reps=reps,
                               mpoints_per_s=round(n / ms * 1e-3, 2), mean_dist_kth=round(float(dd[:, -1].mean()), 3))
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
