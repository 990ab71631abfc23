"""Nearest-first k-nearest over an instanced scene (Instances.knearest_tree_batch) against the flat form (Instances.knearest_batch) and
against the flattened scene: tools/instances_knn_bench.py's scene (64 instances of the 120 k-triangle cube tree on a 4 x 4 x 4 grid,
random rotations, f32) and DESIGN.md §4o's protocol — points in HBM drawn uniformly over the grid's bounds, the host clock around one
call ending in a device synchronise, one warm-up call of each form, then the samples of the flat and the tree form ALTERNATING in one
process, the median of the samples with its range.

Rows, for every point count and every k: the flat form, the tree form, knearest_tree_batch(triangles=True) on ONE tree over the same
7.7 M world-space triangles, and the tree form with max_dist set to the cloud's median k = 1 distance; whether the two forms' distances
agree bit for bit; then the tree form alone at --big points (the flat form needs seconds per call whatever the point count, so it is never
run there).  Every row is printed as soon as it is measured.

    python tools/instances_knn_tree_bench.py [--points 16384 131072] [--big 1000000] [--k 1 8 64] [--samples 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), samples=len(ms))


def alternating(fns, sync, samples):
    """{name: per-call milliseconds}: one warm-up call of each, then `samples` rounds in which every fn is called once, in turn"""
    for fn in fns.values():
        fn()
    sync()
    ms = {name: [] for name in fns}
    for _ in range(samples):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[16_384, 131_072])
    ap.add_argument("--big", type=int, default=1_000_000, help="the tree form alone at this many points (0: skip)")
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--no-flat", action="store_true", help="leave the flat form out (it takes seconds per call)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, testbase as tb
    from instances_bench import rotations
    from instances_knn_bench import block_lds
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_knn_tree_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
    ctx = Context(0)
    half = np.float32(a.half_extent)
    tris, aabbs = tb.create_n_cubes(a.cubes, np.array([-half] * 3 + [half] * 3, dtype=np.float32))
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    centre, extent = (lo + hi) / 2, float((hi - lo).max())
    g = a.grid
    n = g ** 3
    R = rotations(n, 1)
    cells = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(n, 3) * (2 * extent)
    x = np.zeros((n, 3, 4))
    x[:, :, :3] = R
    x[:, :, 3] = cells + centre - np.einsum("nij,j->ni", R, centre)      # rotate about the tree's centre, then onto the grid cell
    x32 = np.ascontiguousarray(x.astype(np.float32))

    member = Bvh.from_aabbs(aabbs, ctx).flatten()
    member.set_triangles(tris)
    inst = Instances([member], np.zeros(n, dtype=np.uint32), x32, ctx)
    wb = inst.world_boxes
    blo, bhi = wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)
    rng = np.random.default_rng(3)
    cloud = (blo + rng.random((max(a.points + [a.big]), 3)) * (bhi - blo)).astype(np.float32)

    world = np.einsum("nij,tvj->ntvi", x32[:, :, :3], tris) + x32[:, None, None, :, 3]
    world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(np.float32))
    flat = Bvh.from_aabbs(tb.triangles_aabbs(world), ctx).flatten()
    flat.set_triangles(world)

    res = dict(instances=n, member_triangles=int(len(tris)), flattened_triangles=int(n * len(tris)), samples=a.samples, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    for count in a.points:
        pts = torch.from_numpy(cloud[:count]).cuda()
        _, _, d1 = inst.knearest_tree_batch(pts, 1)
        radius = float(d1[:, 0].median().item())                 # the cloud's median k = 1 distance
        for k in a.k:
            lanes, lds = block_lds(k)
            row = dict(points=count, k=k, block=lanes, lds_bytes=lds, max_dist=radius)
            fns = {} if a.no_flat else {"flat_form": lambda: inst.knearest_batch(pts, k)}
            fns["tree_form"] = lambda: inst.knearest_tree_batch(pts, k)
            row.update(alternating(fns, ctx.synchronize, a.samples))
            print(json.dumps(row), flush=True)
            row.update(alternating({"flattened_scene_tree_form": lambda: flat.knearest_tree_batch(pts, k, triangles=True),
                                    "tree_form_max_dist": lambda: inst.knearest_tree_batch(pts, k, radius)}, ctx.synchronize, a.samples))
            _, _, dt = inst.knearest_tree_batch(pts, k)
            _, df = flat.knearest_tree_batch(pts, k, triangles=True)
            row["same_distance_share_flattened"] = float((dt == df).float().mean().item())
            if not a.no_flat:
                _, _, di = inst.knearest_batch(pts, k)
                row["distances_equal_flat_form"] = bool((dt == di).all().item())
            _, _, dm = inst.knearest_tree_batch(pts, k, radius)
            row["filled_share_max_dist"] = float(torch.isfinite(dm).float().mean().item())
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if a.big:
        pts = torch.from_numpy(cloud[:a.big]).cuda()
        for k in a.k:
            row = dict(points=a.big, k=k)
            row.update(alternating({"tree_form": lambda: inst.knearest_tree_batch(pts, k),
                                    "flattened_scene_tree_form": lambda: flat.knearest_tree_batch(pts, k, triangles=True)}, ctx.synchronize, a.samples))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
