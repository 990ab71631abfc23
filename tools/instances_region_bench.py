"""Frustum culling of an instanced scene with Instances.region_batch against what a caller had to do before it: region_batch on ONE tree over
the flattened scene's world-space triangles, plus that tree's rebuild.

Scene: tools/instances_bench.py's — 64 instances of the 120 k-triangle cube tree on a 4 x 4 x 4 grid at twice the tree's extent, random
rotations.  Batches of 1 and 64 frusta whose eyes sit on a sphere of three half-extents around the grid and look at its centre; the field of
view is found by bisection so that a frustum sees about 1 %, 10 % and 50 % of the (world-space) shapes.  Planes are in HBM.  Per combination:
  full / count / classify / instances_only   Instances.region_batch with those flags
  flattened                                  bvh_amd.region_batch over the flattened scene with the same planes
and the counts: pairs P (the instances_only total), units (P x the chunks per pair), shapes returned, and their ratio to the flattened
scene's (not 1: the member's boxes are tested in their own frame, the flattened scene's are world-space boxes around rotated triangles).
Once per run: Instances.update (the re-pose) against the flattened tree's rebuild + flatten.
Host clock around calls that end in a device synchronise; warm-up, then the median, minimum and maximum of `--repeats` samples of `inner`
calls each (inner is chosen so that a sample is about 30 ms of work).

    python tools/instances_region_bench.py [--cubes 10000] [--grid 4] [--batches 1 64] [--fractions 0.01 0.1 0.5] [--repeats 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from instances_bench import rotations                                  # noqa: E402
from region_bench import eyes, fov_for, frusta, timed                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.01, 0.1, 0.5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, frustum_planes, region_batch, testbase as tb
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_region_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
    ctx = Context(0)
    tris, aabbs = tb.create_n_cubes(a.cubes)
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    centre, extent = (lo + hi) / 2, float((hi - lo).max())
    g = a.grid
    n = g ** 3
    R = rotations(n, 1)
    cells = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(n, 3) * (2 * extent)
    x = np.zeros((n, 3, 4))
    x[:, :, :3] = R
    x[:, :, 3] = cells + centre - np.einsum("nij,j->ni", R, centre)
    x32 = np.ascontiguousarray(x.astype(np.float32))

    member = Bvh.from_aabbs(aabbs, ctx).flatten()
    member.set_triangles(tris)
    inst = Instances([member], np.zeros(n, dtype=np.uint32), x32, ctx)
    world = np.einsum("nij,tvj->ntvi", x32[:, :, :3], tris) + x32[:, None, None, :, 3]
    world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(np.float32))
    world_aabbs = tb.triangles_aabbs(world)
    flat_bvh = Bvh.from_aabbs(world_aabbs, ctx)
    flat = flat_bvh.flatten()
    dev_aabbs = torch.from_numpy(world_aabbs).cuda()
    n_member = max(2 * len(aabbs) - 2, 1)

    wb = inst.world_boxes.astype(np.float64)
    glo, ghi = wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)
    gcentre, ghalf = (glo + ghi) / 2, float((ghi - glo).max()) / 2
    rng = np.random.default_rng(0)
    sample = world_aabbs[rng.integers(0, len(world_aabbs), size=200_000)].astype(np.float64)
    centres = (sample[:, :3] + sample[:, 3:]) / 2

    res = dict(instances=n, member_shapes=int(len(aabbs)), flattened_shapes=int(len(world_aabbs)), member_entries=n_member, warmup=a.warmup,
               repeats=a.repeats, rows=[])
    dirs = eyes(max(a.batches), 1)
    sync = ctx.synchronize
    for share in a.fractions:
        fov = fov_for(share, dirs[0], gcentre, ghalf, centres, frustum_planes)
        for nb in a.batches:
            planes, _ = frusta(dirs[:nb], gcentre, ghalf, fov, frustum_planes)
            tp = torch.from_numpy(planes).cuda()
            row = dict(share_wanted=share, fov_deg=fov, regions=nb)
            pairs = int(inst.region_batch(tp, count_only=True, instances_only=True)["offsets"][-1].item())
            total = int(inst.region_batch(tp, count_only=True)["offsets"][-1].item())
            flat_total = int(region_batch(flat, tp, count_only=True)["offsets"][-1].item())
            per = -(-8192 // max(pairs, 1))
            ce = max(-(-(-(-n_member // per)) // 64) * 64, 1024)
            row.update(pairs=pairs, chunks_per_pair=-(-n_member // ce), units=pairs * -(-n_member // ce), shapes=total, flattened_shapes=flat_total,
                       shapes_over_flattened=total / max(flat_total, 1))
            row["full"] = timed(lambda: inst.region_batch(tp), sync, a.warmup, a.repeats)
            row["count"] = timed(lambda: inst.region_batch(tp, count_only=True), sync, a.warmup, a.repeats)
            row["classify"] = timed(lambda: inst.region_batch(tp, classify=True), sync, a.warmup, a.repeats)
            row["instances_only"] = timed(lambda: inst.region_batch(tp, instances_only=True), sync, a.warmup, a.repeats)
            row["flattened"] = timed(lambda: region_batch(flat, tp), sync, a.warmup, a.repeats)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    res["instances_update"] = timed(lambda: inst.update(x32), sync, a.warmup, a.repeats)
    res["flattened_rebuild"] = timed(lambda: flat_bvh.rebuild(dev_aabbs, flatten=True), sync, a.warmup, a.repeats)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
