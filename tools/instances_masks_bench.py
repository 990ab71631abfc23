"""What per-instance visibility masks cost and save (bvhgpu_instances_*_masked_*), on tools/instances_bench.py's scene and clock: 64 rotated
instances of the 120 k-triangle cube tree on a 4 x 4 x 4 grid, 1 M rays in HBM aimed at random triangles, f32; host clock around calls that
end in a device synchronise, every sample `inner` calls.

Closest hit through four paths, timed in alternating rounds so that every path sees the same drift of the session:
    unmasked        Instances.closest_hits — the entry that reads no mask
    all_ones        closest_hits_masked, every instance mask 0xFFFFFFFF, no ray mask: the masked kernel with nothing to skip — what the test costs
    half_hidden     closest_hits_masked, every odd instance's mask 0, no ray mask: half of the scene hidden from every ray
    per_ray_half    closest_hits_masked, M[i] = 1 << (i % 32), per ray a random mask of 16 bits: half of the instances hidden from each ray,
                    another half for every ray (the lanes of a wave skip different instances)
and all-hits (sorted) through the first three.  Reports per path the median and the range over all samples, the rays that hit, and for
all-hits the rows' total — the work left.

    python tools/instances_masks_bench.py [--rays 1000000] [--cubes 10000] [--grid 4] [--rounds 3] [--warmup 2] [--repeats 5] [--inner 10] [--out FILE.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, RayBatch, testbase as tb
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_masks_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
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
    x[:, :, 3] = cells + centre - np.einsum("nij,j->ni", R, centre)
    x32 = np.ascontiguousarray(x.astype(np.float32))
    member = Bvh.from_aabbs(aabbs, ctx).flatten()
    member.set_triangles(tris)
    inst = Instances([member], np.zeros(n, dtype=np.uint32), x32, ctx)

    wb = inst.world_boxes
    bounds = np.concatenate([wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)]).astype(np.float32)
    buf = torch.empty(a.rays * 36, dtype=torch.uint8, device="cuda")
    RayBatch.generate(0, a.rays, bounds, buf, np.float32, ctx)
    rng = np.random.default_rng(2)
    o = np.frombuffer(buf[: a.rays * 36].cpu().numpy().tobytes(), dtype=bvh_amd._lib.RAY_F32)["o"].copy()
    pick = rng.integers(0, n * len(tris), size=a.rays)                    # a triangle of the flattened scene: (instance, triangle)
    pi, pt = pick // len(tris), pick % len(tris)
    centroid = tris.reshape(-1, 3, 3)[pt].mean(axis=1).astype(np.float64)
    target = (np.einsum("nij,nj->ni", x[pi, :, :3], centroid) + x[pi, :, 3]).astype(np.float32)
    aimed_host = RayBatch.new(o, target - o, np.float32, ctx).host
    buf2 = torch.from_numpy(aimed_host.view(np.uint8).copy()).cuda()
    aimed = RayBatch.from_device(buf2, a.rays, np.float32)

    ones = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    odd_hidden = np.where(np.arange(n) % 2 == 1, 0, 0xFFFFFFFF).astype(np.uint32)
    by_bit = (np.uint32(1) << (np.arange(n, dtype=np.uint32) % 32)).astype(np.uint32)
    bits = np.argsort(rng.random((a.rays, 32)), axis=1)[:, :16].astype(np.uint32)          # 16 of 32 bits per ray
    rmask = np.bitwise_or.reduce(np.uint32(1) << bits, axis=1).astype(np.uint32)
    rmask_dev = torch.from_numpy(rmask.view(np.int32).copy()).cuda()

    def setter(m):
        return lambda: inst.set_masks(m)
    closest = {
        "unmasked": (setter(ones), lambda: inst.closest_hits(aimed)),
        "all_ones": (setter(ones), lambda: inst.closest_hits_masked(aimed, None)),
        "half_hidden": (setter(odd_hidden), lambda: inst.closest_hits_masked(aimed, None)),
        "per_ray_half": (setter(by_bit), lambda: inst.closest_hits_masked(aimed, rmask_dev)),
    }
    allhits = {
        "unmasked": (setter(ones), lambda: inst.allhits_batch(aimed)),
        "all_ones": (setter(ones), lambda: inst.allhits_masked_batch(aimed, None)),
        "half_hidden": (setter(odd_hidden), lambda: inst.allhits_masked_batch(aimed, None)),
    }
    res = dict(instances=n, member_triangles=int(len(tris)), rays=a.rays, rounds=a.rounds, warmup=a.warmup, repeats=a.repeats, inner=a.inner)
    for family, paths in (("closest", closest), ("allhits_sorted", allhits)):
        samples = {k: [] for k in paths}
        fam = res[family] = {}
        for _ in range(a.rounds):
            for name, (prepare, fn) in paths.items():
                prepare()
                t = timed(fn, ctx.synchronize, a.warmup, a.repeats, a.inner)
                samples[name] += [t["min_ms"], t["median_ms"], t["max_ms"]]                # (the extremes and the middle of each round)
        for name, (prepare, fn) in paths.items():
            prepare()
            got = fn()
            s = samples[name]
            fam[name] = dict(median_ms=float(np.median(s)), min_ms=float(np.min(s)), max_ms=float(np.max(s)))
            if family == "closest":
                fam[name]["rays_hit"] = int((got[1] != -1).sum().item())
            else:
                fam[name]["hits"] = int(got["offsets"][-1].item())
        base = fam["unmasked"]["median_ms"]
        for name in paths:
            fam[name]["vs_unmasked"] = fam[name]["median_ms"] / base
    inst.set_masks(None)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
