"""What the leaf kind of an instance set costs: closest_hits on ONE scene for the TRIANGLE, BOX and SPHERE sets over the same member boxes
and poses.

The scene is tools/instances_bench.py's: 64 instances of the 120 k-shape cube tree on a 4 x 4 x 4 grid at twice the tree's extent, random
rotations, 1 M rays in HBM.  The member's shapes are the cubes' triangles; the BOX set tests each triangle's own box, the SPHERE set the sphere
inscribed in that box (centre of the box, the smallest half extent — a flat box gives a sphere of radius 0 that nothing hits, so a sphere
of a quarter of the largest extent stands in for it).  Two ray batches, as there: the bench stream over the grid's bounds (crosses world
boxes, hits next to nothing) and the same origins aimed at random world-space triangles.

Host clock around `inner` calls that end in a device synchronise; warm-up calls, then the median and the range of the samples.
--kinds triangle runs on a tree that has no leaf kinds yet (the constructor is then called without `leaf`): the figure to compare the
TRIANGLE set with.

    python tools/instances_leaf_bench.py [--kinds triangle,box,sphere] [--rays 1000000] [--cubes 10000] [--grid 4] [--warmup 3] [--repeats 10]
                                         [--inner 20] [--out FILE.json]
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

from instances_bench import rotations, timed  # noqa: E402


def inscribed_spheres(aabbs):
    """(n, 4) {centre of the box, its smallest half extent}; a degenerate box gets a quarter of its largest extent"""
    half = (aabbs[:, 3:] - aabbs[:, :3]) / 2
    r = half.min(axis=1)
    r = np.where(r > 0, r, half.max(axis=1) / 2)
    return np.ascontiguousarray(np.concatenate([(aabbs[:, :3] + aabbs[:, 3:]) / 2, r[:, None]], axis=1).astype(aabbs.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="triangle,box,sphere")
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kinds = [k for k in a.kinds.split(",") if k]

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, RayBatch, testbase as tb
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_leaf_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
    ctx = Context(0)
    half = np.float32(100000.0)
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
    if "sphere" in kinds:
        member.set_spheres(inscribed_spheres(aabbs))
    of = np.zeros(n, dtype=np.uint32)
    sets = {k: (Instances([member], of, x32, ctx) if k == "triangle" else Instances([member], of, x32, ctx, leaf=k)) for k in kinds}

    wb = next(iter(sets.values())).world_boxes
    bounds = np.concatenate([wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)]).astype(np.float32)
    buf = torch.empty(a.rays * 36, dtype=torch.uint8, device="cuda")
    rays = RayBatch.generate(0, a.rays, bounds, buf, np.float32, ctx)
    rng = np.random.default_rng(2)
    o = np.frombuffer(buf[: a.rays * 36].cpu().numpy().tobytes(), dtype=bvh_amd._lib.RAY_F32)["o"].copy()
    pick_i, pick_t = rng.integers(0, n, size=a.rays), rng.integers(0, len(tris), size=a.rays)
    target = np.einsum("rij,rj->ri", x32[pick_i, :, :3], tris[pick_t].mean(axis=1)) + x32[pick_i, :, 3]
    aimed_host = RayBatch.new(o, (target - o).astype(np.float32), np.float32, ctx).host
    buf2 = torch.from_numpy(aimed_host.view(np.uint8).copy()).cuda()
    aimed = RayBatch.from_device(buf2, a.rays, np.float32)

    res = dict(instances=n, member_shapes=int(len(tris)), rays=a.rays, warmup=a.warmup, repeats=a.repeats, inner=a.inner, kinds=kinds)
    for name, batch in (("stream", rays), ("aimed", aimed)):
        r = res[name] = {}
        for k in kinds:
            s = sets[k]
            r[k] = timed(lambda: s.closest_hits(batch), ctx.synchronize, a.warmup, a.repeats, a.inner)
            r[k]["rays_hit"] = int((s.closest_hits(batch)[1] != -1).sum())
        if "triangle" in r:
            for k in kinds:
                r[k]["vs_triangle"] = r[k]["median_ms"] / r["triangle"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
