"""All-hits over an instanced scene against its floor and against the flattened scene: tools/instances_bench.py's scene (64 instances of the
120 k-triangle cube tree on a 4 x 4 x 4 grid, random rotations) and its aimed rays (1 M rays in HBM, each towards the centroid of a random
world-space triangle), its protocol (the host clock around `inner` calls ending in a device synchronise, warm-ups, the median of the repeats
with its range).

Rows: Instances.allhits_batch sorted, in list order and count-only; Instances.closest_hits on the same set and rays (the same walk with no
rows to write: the floor of one pass); allhits_batch(leaf="triangle") on ONE tree over the same 7.7 M world-space triangles.  Also the
mean and the longest row.

    python tools/instances_allhits_bench.py [--rays 1000000] [--cubes 10000] [--grid 4] [--warmup 3] [--repeats 10] [--inner 20] [--out FILE.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, RayBatch, testbase as tb
    from instances_bench import rotations, timed
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_allhits_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
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

    world = np.einsum("nij,tvj->ntvi", x32[:, :, :3], tris) + x32[:, None, None, :, 3]
    world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(np.float32))

    wb = inst.world_boxes
    bounds = np.concatenate([wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)]).astype(np.float32)
    buf = torch.empty(a.rays * 36, dtype=torch.uint8, device="cuda")
    RayBatch.generate(0, a.rays, bounds, buf, np.float32, ctx)
    rng = np.random.default_rng(2)
    o = np.frombuffer(buf[: a.rays * 36].cpu().numpy().tobytes(), dtype=bvh_amd._lib.RAY_F32)["o"].copy()
    target = world[rng.integers(0, len(world), size=a.rays)].mean(axis=1)
    aimed_host = RayBatch.new(o, target - o, np.float32, ctx).host
    buf2 = torch.from_numpy(aimed_host.view(np.uint8).copy()).cuda()
    aimed = RayBatch.from_device(buf2, a.rays, np.float32)

    res = dict(instances=n, member_triangles=int(len(tris)), flattened_triangles=int(len(world)), rays=a.rays, warmup=a.warmup, repeats=a.repeats)
    run = lambda fn: timed(fn, ctx.synchronize, a.warmup, a.repeats, a.inner)
    res["instances_allhits_sorted"] = run(lambda: inst.allhits_batch(aimed))
    res["instances_allhits_list_order"] = run(lambda: inst.allhits_batch(aimed, sort=False))
    res["instances_allhits_count_only"] = run(lambda: inst.allhits_batch(aimed, count_only=True))
    res["instances_closest"] = run(lambda: inst.closest_hits(aimed))
    lens = np.diff(inst.allhits_batch(aimed, count_only=True)["offsets"].cpu().numpy())
    res["rows"] = dict(total=int(lens.sum()), mean=float(lens.mean()), max=int(lens.max()), empty=int((lens == 0).sum()))
    flat = Bvh.from_aabbs(tb.triangles_aabbs(world), ctx).flatten()
    flat.set_triangles(world)
    res["flattened_allhits_sorted"] = run(lambda: flat.allhits_batch(aimed, "triangle"))
    flens = np.diff(flat.allhits_batch(aimed, "triangle")[0].cpu().numpy())
    res["flattened_rows"] = dict(total=int(flens.sum()), mean=float(flens.mean()), max=int(flens.max()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
