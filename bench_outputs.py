"""bench_outputs.py — `bench.py --dump-outputs DIR`: what the timed step computed in its last step, as a caller of that step receives it,
written as DIR/<name>.npy (float32 / float64) so that two builds of the project can be compared output for output on identical inputs.

The step is FlatBvh::build + FlatBvh::traverse of one ray batch, so its outputs are the FlatNode array of the tree it built and the batch's
result: the CSR hit lists (offsets, indices), for `--harness closest` the nearest Intersection and shape per ray, for `--harness
triangles` the CSR plus the Intersection of every candidate.  Integer fields are written as float64 (exact for u32).

Every value in the files is finite.  The reference's FlatNode array gives each shape entry Aabb::empty() = (+inf, -inf), and a ray
without a hit has an infinite distance: such elements are written as 0 in `<name>.npy`, and `<name>_nonfinite.npy` (same shape and
dtype, only when there are any) holds +1 / -1 / 2 for +inf / -inf / NaN and 0 elsewhere, so nothing is lost.  The files hold at most
DUMP_BUDGET bytes: outputs that fit are written whole, and one above its share of what is left is replaced by a fixed, seeded sample of its rows (the same rows in its `_nonfinite`
companion), and `<name>_rows.npy` names them."""
from __future__ import annotations

import os

import numpy as np

DUMP_BUDGET = 64_000_000        # bytes over all files of one dump


def step_outputs(wl, hits, tree):
    """the arrays of the batch `hits` just completed and of the FlatNode array of `tree`, copied to the host (after the timed region)"""
    from bvh_amd import FlatBvh
    flat = FlatBvh.nodes.fget(tree)        # (the reference-layout array of the tree the step built; a Bvh and a FlatBvh share the read)
    out = {"flat_bounds": np.concatenate([flat["min"], flat["max"]], axis=1).astype(wl.np_dtype),
           "flat_links": np.stack([flat["entry"], flat["exit"], flat["shape"]], axis=1).astype(np.float64)}
    if wl.harness == "closest":
        isect, shape = hits.fetch_closest(wl.R, wl.np_dtype)
        out.update(closest_isect=isect, closest_shape=shape.astype(np.float64))
        return out
    off, idx = hits.fetch(wl.R)
    out.update(hit_offsets=off.astype(np.float64), hit_indices=idx.astype(np.float64))
    if wl.harness == "triangles":
        out["triangle_isect"] = hits.fetch_triangles(wl.np_dtype)
    return out


def split_nonfinite(a):
    """(a with every non-finite element set to 0, codes +1 / -1 / 2 for +inf / -inf / NaN in a's dtype) — codes None when all are finite"""
    bad = ~np.isfinite(a)
    if not bad.any():
        return a, None
    codes = np.zeros_like(a)
    codes[np.isposinf(a)], codes[np.isneginf(a)], codes[np.isnan(a)] = 1, -1, 2
    return np.where(bad, np.zeros_like(a), a), codes


def write_outputs(outputs, dirname):
    """DIR/<name>.npy per output (+ <name>_nonfinite.npy); an output above its share keeps a seeded sample of its rows (sorted), named in
    <name>_rows.npy"""
    os.makedirs(dirname, exist_ok=True)
    groups = {}
    for name, a in outputs.items():
        a, codes = split_nonfinite(np.ascontiguousarray(a))
        groups[name] = {name: a} if codes is None else {name: a, name + "_nonfinite": codes}
    cost = {name: sum(v.nbytes for v in files.values()) for name, files in groups.items()}
    share, left = {}, DUMP_BUDGET - 4096 * sum(len(f) + 1 for f in groups.values())      # (npy headers)
    for i, name in enumerate(sorted(cost, key=cost.get)):     # the smaller outputs whole, the larger ones share what is left
        share[name] = min(cost[name], left // (len(cost) - i))
        left -= share[name]
    written = {}
    for name, files in groups.items():
        a = files[name]
        row = max(a.nbytes // max(len(a), 1), 1) * len(files)
        if cost[name] > share[name]:
            k = share[name] // (row + 8)
            rows = np.sort(np.random.default_rng(0).choice(len(a), size=k, replace=False))
            files = {n: v[rows] for n, v in files.items()}
            files[name + "_rows"] = rows.astype(np.float64)
        for n, v in files.items():
            np.save(os.path.join(dirname, n + ".npy"), v)
            written[n] = list(v.shape)
    return written
