"""Radius search over an instanced scene against the flattened scene: tools/instances_bench.py's scene (64 instances of the 120 k-triangle
cube tree on a 4 x 4 x 4 grid, random rotations) and its protocol (the host clock around `inner` calls ending in a device synchronise,
warm-ups, the median of the repeats with its range), 1 M points in HBM drawn uniformly over the grid's bounds and ONE radius for all of
them, chosen by a few count-only calls on the first 65 536 points so that the mean row is about `--mean-row`.

Rows: Instances.within_batch sorted, in list order and count-only; Instances.update (the re-pose); within_batch(triangles=True) on ONE tree
over the same 7.7 M world-space triangles, and that tree's rebuild.  Also the row statistics of both scenes, which sort tier the rows fall
into, and what the object-frame slack costs on a sample of the points: the instances a point enters (the top level's rows, from a tree over
the world boxes) and the member triangles it tests there (the shapes whose own box lies within r * ||Y||_F of the object-frame point, which
are the leaf entries the member walk accepts), beside the candidates it keeps.

    python tools/instances_within_bench.py [--points 1000000] [--mean-row 20] [--cubes 10000] [--grid 4] [--warmup 3] [--repeats 10] [--inner 20] [--out FILE.json]
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
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--mean-row", type=float, default=20.0)
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--sample", type=int, default=65536, help="points of the radius search and of the visit statistics")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, testbase as tb
    from instances_bench import rotations, timed
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_within_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
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
    pts_host = (blo + rng.random((a.points, 3)) * (bhi - blo)).astype(np.float32)
    pts = torch.from_numpy(pts_host).cuda()
    ns = min(a.sample, a.points)
    sample = pts[:ns].contiguous()

    # the radius: rows grow like r^3 in a uniform cloud, so a few corrected steps land near the wanted mean
    r = 0.02 * extent
    for _ in range(8):
        mean = float(np.diff(inst.within_batch(sample, float(r), count_only=True)["offsets"].cpu().numpy()).mean())
        if mean > 0 and abs(mean / a.mean_row - 1) < 0.03:
            break
        r *= 2.0 if mean == 0 else float(np.clip((a.mean_row / mean) ** (1 / 3), 0.5, 2.0))
    r = float(np.float32(r))

    res = dict(instances=n, member_triangles=int(len(tris)), flattened_triangles=int(n * len(tris)), points=a.points, radius=r, extent=extent,
               warmup=a.warmup, repeats=a.repeats)
    run = lambda fn, inner=a.inner: timed(fn, ctx.synchronize, a.warmup, a.repeats, inner)   # noqa: E731
    res["instances_within_sorted"] = run(lambda: inst.within_batch(pts, r))
    res["instances_within_list_order"] = run(lambda: inst.within_batch(pts, r, sort=False))
    res["instances_within_count_only"] = run(lambda: inst.within_batch(pts, r, count_only=True))
    res["instances_update"] = run(lambda: inst.update(x32))
    lens = np.diff(inst.within_batch(pts, r, count_only=True)["offsets"].cpu().numpy())
    import re
    src = open(os.path.join(ROOT, "bvh_amd", "csrc", "instances_within.hip")).read()
    lane_max, lds_max = (int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))
                         for name in ("INST_WITHIN_LANE_ROW_MAX", "INST_WITHIN_LDS_ROW_MAX"))
    res["rows"] = dict(total=int(lens.sum()), mean=float(lens.mean()), max=int(lens.max()), empty=int((lens == 0).sum()),
                       lane_tier=int(((lens >= 1) & (lens <= lane_max)).sum()), lds_tier=int(((lens > lane_max) & (lens <= lds_max)).sum()),
                       global_tier=int((lens > lds_max).sum()), lane_row_max=lane_max, lds_row_max=lds_max)

    # ---- what the slack costs, on the sample: instances entered, member triangles tested, candidates kept
    top = Bvh.from_aabbs(wb, ctx).flatten()
    toff, tinst, _ = top.within_batch(sample, r, sort=False)
    toff, tinst = toff.cpu().numpy().astype(np.int64), tinst.cpu().numpy().astype(np.int64)
    point_of = np.repeat(np.arange(ns), np.diff(toff))
    y = np.transpose(R, (0, 2, 1))                                        # rotations: Y = R^T, ||Y||_F^2 = 3
    y3 = -np.einsum("nij,nj->ni", y, x[:, :, 3])
    tested = 0
    for i in range(n):
        sel = point_of[tinst == i]
        if len(sel) == 0:
            continue
        q = pts_host[sel].astype(np.float64) @ y[i].T + y3[i]
        qd = torch.from_numpy(np.ascontiguousarray(q.astype(np.float32))).cuda()
        tested += int(member.within_batch(qd, float(np.float32(r * np.sqrt(3.0))), count_only=True)[0][-1])
    kept = int(np.diff(inst.within_batch(sample, r, count_only=True)["offsets"].cpu().numpy()).sum())
    res["visits"] = dict(sample=ns, instances_entered_per_point=len(tinst) / ns, triangles_tested_per_point=tested / ns,
                         candidates_per_point=kept / ns)

    # ---- the flattened scene: one tree over the world-space triangles
    world = np.einsum("nij,tvj->ntvi", x32[:, :, :3], tris) + x32[:, None, None, :, 3]
    world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(np.float32))
    world_aabbs = tb.triangles_aabbs(world)
    flat_bvh = Bvh.from_aabbs(world_aabbs, ctx)
    flat = flat_bvh.flatten()
    flat.set_triangles(world)
    res["flattened_within_sorted"] = run(lambda: flat.within_batch(pts, r, triangles=True))
    res["flattened_within_count_only"] = run(lambda: flat.within_batch(pts, r, triangles=True, count_only=True))
    flens = np.diff(flat.within_batch(pts, r, triangles=True, count_only=True)[0].cpu().numpy())
    res["flattened_rows"] = dict(total=int(flens.sum()), mean=float(flens.mean()), max=int(flens.max()), same_lengths_share=float((flens == lens).mean()))
    dev_aabbs = torch.from_numpy(world_aabbs).cuda()
    res["flattened_rebuild"] = run(lambda: flat_bvh.rebuild(dev_aabbs, flatten=True), max(1, a.inner // 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
