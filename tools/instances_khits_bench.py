"""k-hits over an instanced scene against the two ways to get the same rows without it: tools/instances_bench.py's scene (64 instances of
the 120 k-triangle cube tree on a 4 x 4 x 4 grid, random rotations), its two ray batches in HBM (the bench stream over the grid's bounds,
and the same origins aimed at random triangles) and its protocol (the host clock around `inner` calls ending in a device synchronise,
warm-ups, the median of the repeats with its range), in f32 and in f64.

Rows, for every dtype, batch and k: Instances.khits_batch; (a) Instances.allhits_batch(sort=True) of the same batch plus the caller's cut
of every row to k (torch, on the device the rows live on) — the only way to these rows without this entry; (b)
FlatBvh.khits_batch(leaf="triangle") on ONE tree over the same 7.7 M world-space triangles.  Before anything is timed the rows of (a) must
equal khits_batch's byte for byte; against (b) the share of slots with bit-equal distances is reported (the flattened scene rounds its
triangles into world space, so it is a sanity figure, not a test).  Every row is printed as soon as it is measured.

    python tools/instances_khits_bench.py [--rays 131072] [--k 1 8 64] [--dtypes f32 f64] [--cubes 10000] [--grid 4] [--warmup 2] [--repeats 7] [--inner 5] [--out FILE.json]
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


def block_lds(k, itemsize):
    """instances_khits_block: the largest of 256 / 128 / 64 lanes whose lists (k x (sizeof(T) + 8) bytes a lane) fit 32 KB, else 64 lanes"""
    per_lane = k * (itemsize + 8)
    lanes = 256 if 256 * per_lane <= 32 * 1024 else 128 if 128 * per_lane <= 32 * 1024 else 64
    return lanes, lanes * per_lane


def cut_rows(got, k):
    """the sorted CSR of allhits_batch (torch, on the device) cut to k and padded → (instance[n,k], shape[n,k], vals[n,k,3])"""
    import torch
    off, inst, shape, vals = got["offsets"], got["instance"], got["shape"], got["vals"]
    n = off.numel() - 1
    slot = torch.arange(k, device=off.device)[None, :]
    valid = slot < (off[1:] - off[:-1])[:, None]
    if inst.numel() == 0:
        pad = torch.zeros((n, k, 3), dtype=vals.dtype, device=off.device)
        pad[:, :, 0] = float("inf")
        return torch.full((n, k), -1, dtype=torch.int32, device=off.device), torch.full((n, k), -1, dtype=torch.int32, device=off.device), pad
    idx = (off[:-1, None] + slot).clamp(max=inst.numel() - 1)
    oi = torch.where(valid, inst[idx], torch.full_like(idx, -1, dtype=torch.int32))
    os_ = torch.where(valid, shape[idx], torch.full_like(idx, -1, dtype=torch.int32))
    pad = torch.zeros(3, dtype=vals.dtype, device=off.device)
    pad[0] = float("inf")
    ov = torch.where(valid[:, :, None], vals[idx], pad[None, None, :])
    return oi, os_, ov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=131_072)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--cubes", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed sample")
    ap.add_argument("--half-extent", type=float, default=100000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bvh_amd
    from bvh_amd import Bvh, Context, Instances, RayBatch, testbase as tb
    from instances_bench import rotations, timed
    if bvh_amd.device_count() <= 0:
        raise SystemExit("instances_khits_bench needs an MI355X: no HIP device visible and there is no CPU fallback")
    ctx = Context(0)
    half = np.float32(a.half_extent)
    tris32, aabbs32 = tb.create_n_cubes(a.cubes, np.array([-half] * 3 + [half] * 3, dtype=np.float32))
    lo, hi = aabbs32[:, :3].min(axis=0).astype(np.float64), aabbs32[:, 3:].max(axis=0).astype(np.float64)
    centre, extent = (lo + hi) / 2, float((hi - lo).max())
    g = a.grid
    n = g ** 3
    R = rotations(n, 1)
    cells = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(n, 3) * (2 * extent)
    x = np.zeros((n, 3, 4))
    x[:, :, :3] = R
    x[:, :, 3] = cells + centre - np.einsum("nij,j->ni", R, centre)      # rotate about the tree's centre, then onto the grid cell

    res = dict(instances=n, member_triangles=int(len(tris32)), flattened_triangles=int(n * len(tris32)), rays=a.rays, warmup=a.warmup,
               repeats=a.repeats, inner=a.inner, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    run = lambda fn: timed(fn, ctx.synchronize, a.warmup, a.repeats, a.inner)   # noqa: E731
    for name in a.dtypes:
        ft = np.float32 if name == "f32" else np.float64
        tris, aabbs = np.ascontiguousarray(tris32.astype(ft)), np.ascontiguousarray(aabbs32.astype(ft))
        xt = np.ascontiguousarray(x.astype(ft))
        member = Bvh.from_aabbs(aabbs, ctx).flatten()
        member.set_triangles(tris)
        inst = Instances([member], np.zeros(n, dtype=np.uint32), xt, ctx)
        world = np.einsum("nij,tvj->ntvi", xt[:, :, :3], tris) + xt[:, None, None, :, 3]
        world = np.ascontiguousarray(world.reshape(-1, 3, 3).astype(ft))
        waabbs = np.ascontiguousarray(np.concatenate([world.min(axis=1), world.max(axis=1)], axis=1))
        flat = Bvh.from_aabbs(waabbs, ctx).flatten()
        flat.set_triangles(world)

        # the bench stream over the grid's bounds (drawn in f32, as bench.py draws it), and its origins aimed at random triangles
        wb = inst.world_boxes
        bounds = np.concatenate([wb[:, :3].min(axis=0), wb[:, 3:].max(axis=0)]).astype(np.float32)
        buf = torch.empty(a.rays * 36, dtype=torch.uint8, device="cuda")
        RayBatch.generate(0, a.rays, bounds, buf, np.float32, ctx)
        stream = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=bvh_amd._lib.RAY_F32)
        o, d = stream["o"].astype(ft), stream["d"].astype(ft)
        target = world[np.random.default_rng(2).integers(0, len(world), size=a.rays)].mean(axis=1)
        batches = {}
        for bname, dirs in (("stream", d), ("aimed", target - o)):
            host = RayBatch.new(o, dirs.astype(ft), ft, ctx).host
            dev = torch.from_numpy(host.view(np.uint8).copy()).cuda()
            batches[bname] = RayBatch.from_device(dev, a.rays, ft)

        for bname, rays in batches.items():
            full = inst.allhits_batch(rays)
            lens = (full["offsets"][1:] - full["offsets"][:-1]).cpu().numpy()
            rows = dict(total=int(lens.sum()), mean=float(lens.mean()), max=int(lens.max()), empty=int((lens == 0).sum()))
            for k in a.k:
                lanes, lds = block_lds(k, np.dtype(ft).itemsize)
                row = dict(dtype=name, batch=bname, k=k, block=lanes, lds_bytes=lds, allhits_rows=rows, rows_longer_than_k=int((lens > k).sum()))
                gi, gs, gv = inst.khits_batch(rays, k)
                wi, ws, wv = cut_rows(inst.allhits_batch(rays), k)
                if not (torch.equal(gi, wi) and torch.equal(gs, ws) and torch.equal(gv.view(torch.uint8), wv.view(torch.uint8))):
                    raise SystemExit(f"khits_batch differs from the cut all-hits rows ({name}, {bname}, k = {k})")
                fv, _ = flat.khits_batch(rays, k, "triangle")
                row["flattened_same_distance_share"] = float((fv[:, :, 0] == gv[:, :, 0]).float().mean().item())
                row["instances_khits"] = run(lambda: inst.khits_batch(rays, k))
                row["allhits_sorted_then_cut"] = run(lambda: cut_rows(inst.allhits_batch(rays), k))
                row["flattened_khits"] = run(lambda: flat.khits_batch(rays, k, "triangle"))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
        inst.close()
        del flat, member, world, waabbs
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
