"""CPU checker for AABB / point / ball query batches (a helper module, not collected by pytest).

Restates <FlatBvh as BoundingHierarchy>::traverse (src/flat_bvh.rs:396-431) with the crate's other three IntersectsAabb queries,
in numpy, in the tree's dtype:
  AABB   Aabb::intersects_aabb (src/aabb/aabb_impl.rs:240-248): miss iff on some axis q.max < lo or hi < q.min
  POINT  Aabb::contains (src/aabb/aabb_impl.rs:175-177): p >= lo and p <= hi on every axis
  BALL   Ball::intersects_aabb (src/ball.rs:85-99): s = ((0 + d0*d0) + d1*d1) + d2*d2 with d = clamp(c, lo, hi) - c
         (num_traits' clamp: c < lo ? lo : (c > hi ? hi : c)), hit iff s <= r*r
It WALKS the oracle's FlatNode array (oracle.orc.flatten): all queries move in lockstep, every iteration advances each unfinished
query by one entry (inner entry: test the node box, hit → entry_index, miss → exit_index; leaf entry: test the shape's own AABB,
report on a hit, go to exit_index).  A brute-force "every shape whose box passes" set would differ from the crate's answer on trees
with empty child bounds (a split without SAH winner) and for NaN box queries.
"""
from __future__ import annotations

import numpy as np

AABB, POINT, BALL = 1, 2, 3
WIDTH = {AABB: 6, POINT: 3, BALL: 4}
NONE = 0xFFFFFFFF


def predicate(kind: int, q: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """the kind's test of queries q (m, width) against boxes [lo, hi] (m, 3) → bool (m,), every operation in q's dtype"""
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == AABB:
            miss = np.zeros(len(q), dtype=bool)
            for k in range(3):
                miss |= (q[:, 3 + k] < lo[:, k]) | (hi[:, k] < q[:, k])
            return ~miss
        if kind == POINT:
            ok = np.ones(len(q), dtype=bool)
            for k in range(3):
                ok &= (q[:, k] >= lo[:, k]) & (q[:, k] <= hi[:, k])
            return ok
        s = np.zeros(len(q), dtype=q.dtype)
        for k in range(3):
            c = q[:, k]
            cl = np.where(c < lo[:, k], lo[:, k], np.where(c > hi[:, k], hi[:, k], c))
            d = cl - c
            s = s + d * d
        r = q[:, 3]
        return s <= r * r


def walk(flat: np.ndarray, shape_aabbs: np.ndarray, kind: int, queries) -> tuple:
    """the lockstep walk → (offsets[n+1] u32, indices u32), query i's shapes in the crate's order"""
    ft = flat["min"].dtype
    q = np.ascontiguousarray(queries, dtype=ft).reshape(-1, WIDTH[kind])
    n = len(q)
    boxes = np.ascontiguousarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    mn, mx = flat["min"], flat["max"]
    entry, exit_, shape = flat["entry"].astype(np.int64), flat["exit"].astype(np.int64), flat["shape"].astype(np.int64)
    m = len(flat)
    idx = np.zeros(n, dtype=np.int64)
    hits = [[] for _ in range(n)]
    while True:
        live = np.nonzero(idx < m)[0]
        if len(live) == 0:
            break
        i = idx[live]
        leaf = entry[i] == NONE
        lo, hi = mn[i].copy(), mx[i].copy()
        if leaf.any():   # leaf entries test the shape's own AABB (flat_bvh.rs:411-418)
            sb = boxes[shape[i[leaf]]]
            lo[leaf], hi[leaf] = sb[:, :3], sb[:, 3:]
        ok = predicate(kind, q[live], lo, hi)
        for j in np.nonzero(leaf & ok)[0]:
            hits[live[j]].append(int(shape[i[j]]))
        idx[live] = np.where(leaf, exit_[i], np.where(ok, entry[i], exit_[i]))
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(h) for h in hits], dtype=np.uint64).astype(np.uint32)
    indices = np.array([s for h in hits for s in h], dtype=np.uint32)
    return offsets, indices


def walk_one(flat: np.ndarray, shape_aabbs: np.ndarray, kind: int, query) -> list:
    """the same loop for ONE query, entry by entry in plain Python (flat_bvh.rs:404-430) — the cross-check of `walk`"""
    ft = flat["min"].dtype
    q = np.asarray(query, dtype=ft).reshape(1, -1)
    boxes = np.asarray(shape_aabbs, dtype=ft).reshape(-1, 6)
    out, i = [], 0
    while i < len(flat):
        node = flat[i]
        if int(node["entry"]) == NONE:
            b = boxes[int(node["shape"])]
            if predicate(kind, q, b[None, :3], b[None, 3:])[0]:
                out.append(int(node["shape"]))
            i = int(node["exit"])
        elif predicate(kind, q, node["min"][None, :], node["max"][None, :])[0]:
            i = int(node["entry"])
        else:
            i = int(node["exit"])
    return out


def reference_lists(shape_aabbs: np.ndarray, kind: int, queries) -> tuple:
    """build + flatten with the oracle, then walk: (offsets, indices, flat)"""
    from oracle import orc
    a = np.ascontiguousarray(shape_aabbs).reshape(-1, 6)
    tree = orc.build(a)
    flat = orc.flatten(tree.nodes)
    off, idx = walk(flat, a, kind, queries)
    return off, idx, flat
