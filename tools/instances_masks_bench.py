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

--families points times the point and region families instead, on the same scene and clock, each through
    unmasked        the entry that reads no mask (within_batch, knearest_batch, knearest_tree_batch, region_batch)
    all_ones        its *_masked_* form, every instance mask 0xFFFFFFFF, no row mask
    half_hidden     its *_masked_* form, every odd instance's mask 0, no row mask
with --points points in HBM drawn in the world boxes (k = 8; the radius of within is 1.5 x the point's nearest distance, so rows are short
and not empty) and --regions boxes of 30 % of the scene's extent as 6 planes each.  Reports per path the median and the range over all
samples, the ratio to the unmasked median and whether the two ranges overlap.  A family whose unmasked call takes longer than --slow-ms (the
k-nearest forms on this scene take seconds) is timed one call per path and round.

    python tools/instances_masks_bench.py [--families rays|points] [--unmasked-only] [--points 262144] [--regions 256] [--k 8] [--rays 1000000] [--cubes 10000] [--grid 4] [--rounds 3] [--warmup 2] [--repeats 5] [--inner 10] [--out FILE.json]
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


def point_families(a, ctx, inst, wb, bounds, setter, ones, odd_hidden, n, n_tris):
    import torch

    from bvh_amd import aabb_planes
    rng = np.random.default_rng(3)
    box = wb[rng.integers(0, n, a.points)]                               # a point in the world box of a random instance
    pts_host = (box[:, :3] + rng.random((a.points, 3)) * (box[:, 3:] - box[:, :3])).astype(np.float32)
    pts = torch.from_numpy(pts_host).cuda()
    _, _, nearest = inst.nearest_tree_batch(pts)                         # (the tree form: the flat form takes seconds here, §4q)
    radius = (nearest * 1.5).contiguous()
    ext = (bounds[3:] - bounds[:3]).astype(np.float64)
    lo = bounds[:3] + rng.random((a.regions, 3)) * ext * 0.7
    planes = torch.from_numpy(np.stack([aabb_planes(c, c + 0.3 * ext) for c in lo]).astype(np.float32)).cuda()
    k = a.k

    def three(plain, masked):
        if a.unmasked_only:
            return {"unmasked": (setter(ones), plain)}
        return {"unmasked": (setter(ones), plain), "all_ones": (setter(ones), lambda: masked(None)), "half_hidden": (setter(odd_hidden), lambda: masked(None))}
    families = (
        ("within_sorted", three(lambda: inst.within_batch(pts, radius), lambda m: inst.within_masked_batch(pts, radius, m))),
        ("knearest", three(lambda: inst.knearest_batch(pts, k), lambda m: inst.knearest_masked_batch(pts, k, m))),
        ("knearest_tree", three(lambda: inst.knearest_tree_batch(pts, k), lambda m: inst.knearest_tree_masked_batch(pts, k, m))),
        ("region", three(lambda: inst.region_batch(planes), lambda m: inst.region_masked_batch(planes, m))),
        ("region_instances_only", three(lambda: inst.region_batch(planes, instances_only=True),
                                        lambda m: inst.region_masked_batch(planes, m, instances_only=True))),
    )
    res = dict(instances=n, member_triangles=int(n_tris), points=a.points, regions=a.regions, k=k, rounds=a.rounds, warmup=a.warmup, repeats=a.repeats,
               inner=a.inner)
    import time
    for family, paths in families:
        samples = {name: [] for name in paths}
        last = {}
        fam = res[family] = {}
        # a probe call of the unmasked entry (the family's warm-up as well): a family whose call takes longer than --slow-ms (the k-nearest
        # forms on this scene take seconds, §4o / §4q) is timed one call per path and round, with no further warm-up
        paths["unmasked"][0]()
        t0 = time.perf_counter()
        paths["unmasked"][1]()
        ctx.synchronize()
        slow = (time.perf_counter() - t0) * 1e3 > a.slow_ms
        fam["samples_per_round"] = "1 call" if slow else f"min, median, max of {a.repeats} samples of {a.inner} calls"
        for _ in range(a.rounds):                                        # alternating rounds: every path sees the same drift of the session
            for name, (prepare, fn) in paths.items():
                prepare()
                if slow:
                    t0 = time.perf_counter()
                    last[name] = fn()
                    ctx.synchronize()
                    samples[name].append((time.perf_counter() - t0) * 1e3)
                else:
                    t = timed(fn, ctx.synchronize, a.warmup, a.repeats, a.inner)
                    samples[name] += [t["min_ms"], t["median_ms"], t["max_ms"]]
            print(family, {name: round(v[-1], 3) for name, v in samples.items()}, file=sys.stderr, flush=True)
        for name, (prepare, fn) in paths.items():
            if name in last:
                got = last[name]
            else:
                prepare()
                got = fn()
            s = samples[name]
            fam[name] = dict(median_ms=float(np.median(s)), min_ms=float(np.min(s)), max_ms=float(np.max(s)))
            if family.startswith("knearest"):
                fam[name]["slots_filled"] = int((got[0] != -1).sum().item())
            else:
                fam[name]["pairs"] = int(got["offsets"][-1].item())
        base = fam["unmasked"]
        for name in paths:
            fam[name]["vs_unmasked"] = fam[name]["median_ms"] / base["median_ms"]
            fam[name]["ranges_overlap"] = bool(fam[name]["min_ms"] <= base["max_ms"] and base["min_ms"] <= fam[name]["max_ms"])
    inst.set_masks(None)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


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
    ap.add_argument("--families", choices=("rays", "points"), default="rays")
    ap.add_argument("--points", type=int, default=262_144)
    ap.add_argument("--regions", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--slow-ms", type=float, default=500.0, help="--families points: a family whose unmasked call takes longer is timed one call "
                    "per path and round")
    ap.add_argument("--unmasked-only", action="store_true", help="--families points: time the unmasked entries alone (a tree from before the "
                    "masked point entries can run this file: the parent's side of an A/B)")
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
    ones = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    odd_hidden = np.where(np.arange(n) % 2 == 1, 0, 0xFFFFFFFF).astype(np.uint32)

    def setter(m):
        return lambda: inst.set_masks(m)

    if a.families == "points":
        point_families(a, ctx, inst, wb, bounds, setter, ones, odd_hidden, n, len(tris))
        return
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

    by_bit = (np.uint32(1) << (np.arange(n, dtype=np.uint32) % 32)).astype(np.uint32)
    bits = np.argsort(rng.random((a.rays, 32)), axis=1)[:, :16].astype(np.uint32)          # 16 of 32 bits per ray
    rmask = np.bitwise_or.reduce(np.uint32(1) << bits, axis=1).astype(np.uint32)
    rmask_dev = torch.from_numpy(rmask.view(np.int32).copy()).cuda()

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
