"""k-nearest over an instanced scene against the flattened scene: tools/instances_bench.py's scene (64 instances of the 120 k-triangle cube
tree on a 4 x 4 x 4 grid, random rotations) and its protocol (the host clock around `inner` calls ending in a device synchronise,
warm-ups, the median of the repeats with its range), 1 M points in HBM drawn uniformly over the grid's bounds.

Rows, for every k: Instances.knearest_batch, and knearest_batch(triangles=True) on ONE tree over the same 7.7 M world-space triangles;
the block size and the bytes of LDS the instance kernel is launched with at that k (the block rule of bvh_amd/csrc/instances_knn.hip
restated here); and how far the two answers agree (the distances, bit for bit — the pairs of a tie may differ, the two walks meeting
them in another order).  Every row is printed as soon as it is measured.  One instanced call takes seconds on this scene whatever the
point count (the list-order walk waits for its slowest lanes), so keep --repeats and --inner small and run it unbuffered.

    python tools/instances_knn_bench.py [--points 1000000] [--k 1 8 64] [--cubes 10000] [--grid 4] [--warmup 1] [--repeats 5] [--inner 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def block_lds(k, itemsize=4):
    """instances_knn_block: the largest of 256 / 128 / 64 lanes whose lists (k x (sizeof(T) + 8) bytes a lane) fit 32 KB, else 64 lanes"""
    per_lane = k * (itemsize + 8)
    lanes = 256 if 256 * per_lane <= 32 * 1024 else 128 if 128 * per_lane <= 32 * 1024 else 64
    return lanes, lanes * per_lane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, testbase as tb
    from instances_bench import rotations, timed
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_knn_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
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
    pts = torch.from_numpy((blo + rng.random((a.points, 3)) * (bhi - blo)).astype(np.float32)).cuda()

    world = np.einsum("nij,tvj->ntvi", x32[:, :, :3], tris) + x32[:, None, None, :, 3]
    world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(np.float32))
    flat = Bvh.from_aabbs(tb.triangles_aabbs(world), ctx).flatten()
    flat.set_triangles(world)

    res = dict(instances=n, member_triangles=int(len(tris)), flattened_triangles=int(n * len(tris)), points=a.points, warmup=a.warmup,
               repeats=a.repeats, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    run = lambda fn: timed(fn, ctx.synchronize, a.warmup, a.repeats, a.inner)   # noqa: E731
    for k in a.k:
        lanes, lds = block_lds(k)
        row = dict(k=k, block=lanes, lds_bytes=lds)
        row["instances_knearest"] = run(lambda: inst.knearest_batch(pts, k))
        print(json.dumps(row), flush=True)
        row["flattened_knearest"] = run(lambda: flat.knearest_batch(pts, k, triangles=True))
        _, _, di = inst.knearest_batch(pts, k)
        _, df = flat.knearest_batch(pts, k, triangles=True)
        row["same_distance_share"] = float((di == df).float().mean().item())
        row["max_relative_distance_gap"] = float(((di - df).abs() / df.clamp_min(1e-30)).max().item())
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
