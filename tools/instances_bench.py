"""Instanced scene against the flattened scene users had to build before: 64 instances of the 120 k-triangle cube tree on a 4 x 4 x 4 grid at
twice the tree's extent, random rotations, 1 M rays of the bench stream scaled to the grid.

Times Instances.closest_hits against closest_hits on ONE tree over the same 7.7 M world-space triangles, and the two build costs: a re-pose
(Instances.update: inverses, world boxes, top-level rebuild) against a full rebuild + flatten of the flattened tree.  Host clock around calls
that end in a device synchronise; warm-up, then the median and the minimum of the repeats.  Also reports the share of rays on which the two
scenes name the same (instance, shape) — they differ by rounding near edges; a sanity figure, not a test.

Two ray batches: the bench stream over the grid's bounds (what a random ray costs: it crosses world boxes and hits next to nothing), and
the same origins aimed at random triangles (what a ray that hits costs).

    python tools/instances_bench.py [--rays 1000000] [--cubes 10000] [--grid 4] [--warmup 3] [--repeats 10] [--inner 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def rotations(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def timed(fn, sync, warmup, repeats, inner):
    """per-call milliseconds: every sample is `inner` calls and a synchronise, so that a sample is tens of milliseconds of work"""
    for _ in range(warmup):
        fn()
    sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), repeats=repeats, inner=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0, help="the unit cubes are drawn in [-h, h]^3 (default: the bench's bounds; a smaller "
                    "scene keeps the flattened scene's f32 world coordinates fine against a cube's edge)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, RayBatch, testbase as tb
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
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
    world_aabbs = tb.triangles_aabbs(world)
    flat_bvh = Bvh.from_aabbs(world_aabbs, ctx)
    flat = flat_bvh.flatten()
    flat.set_triangles(world)

    wb = inst.world_boxes
    bounds = np.concatenate([wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)]).astype(np.float32)
    buf = torch.empty(a.rays * 36, dtype=torch.uint8, device="cuda")
    rays = RayBatch.generate(0, a.rays, bounds, buf, np.float32, ctx)

    # the bench stream over the grid's bounds crosses many world boxes and hits next to nothing (unit cubes in a 10^6-wide scene); a second
    # batch is aimed at triangles: origins of the same stream, each towards the centroid of a random world-space triangle
    rng = np.random.default_rng(2)
    o = np.frombuffer(buf[: a.rays * 36].cpu().numpy().tobytes(), dtype=bvh_amd._lib.RAY_F32)["o"].copy()
    target = world[rng.integers(0, len(world), size=a.rays)].mean(axis=1)
    aimed_host = RayBatch.new(o, target - o, np.float32, ctx).host
    buf2 = torch.from_numpy(aimed_host.view(np.uint8).copy()).cuda()
    aimed = RayBatch.from_device(buf2, a.rays, np.float32)

    res = dict(instances=n, member_triangles=int(len(tris)), flattened_triangles=int(len(world)), rays=a.rays, warmup=a.warmup, repeats=a.repeats)
    dev_aabbs = torch.from_numpy(world_aabbs).cuda()
    for name, batch in (("stream", rays), ("aimed", aimed)):
        r = res[name] = {}
        r["instances_closest"] = timed(lambda: inst.closest_hits(batch), ctx.synchronize, a.warmup, a.repeats, a.inner)
        r["flattened_closest"] = timed(lambda: flat.closest_hits(batch, fetch=False), ctx.synchronize, a.warmup, a.repeats, a.inner)
        vals, ii, ss = inst.closest_hits(batch)
        ii, ss = ii.cpu().numpy().view(np.uint32).astype(np.int64), ss.cpu().numpy().view(np.uint32).astype(np.int64)
        fvals, fshape, _ = flat.closest_hits(batch)
        fshape = fshape.astype(np.int64)
        hit_i, hit_f = ii != 0xFFFFFFFF, fshape != 0xFFFFFFFF
        same = (hit_i == hit_f) & (~hit_i | (ii * len(tris) + ss == fshape))
        r["rays_hit_instances"], r["rays_hit_flattened"] = int(hit_i.sum()), int(hit_f.sum())
        r["same_answer_share"] = float(same.mean())
        r["same_answer_share_of_hits"] = float(same[hit_i | hit_f].mean()) if (hit_i | hit_f).any() else None
    res["instances_update"] = timed(lambda: inst.update(x32), ctx.synchronize, a.warmup, a.repeats, a.inner)
    res["flattened_rebuild"] = timed(lambda: flat_bvh.rebuild(dev_aabbs, flatten=True), ctx.synchronize, a.warmup, a.repeats, max(1, a.inner // 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
