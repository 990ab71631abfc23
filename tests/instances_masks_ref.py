"""Reference for the masked ray queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_*_masked_*): the candidate table of
tests/instances_ref.py's Scene.trace with the rows of the instances invisible to their ray dropped — instance i is visible to ray j iff
(M[i] & R[j]) != 0 — and then exactly what the existing references do on the full table: closest / first selection (instances_ref),
all-hits rows (instances_allhits_ref) and k-hits rows (instances_khits_ref).  Nothing else."""
import numpy as np

import instances_allhits_ref as iar
import instances_khits_ref as ikh

NONE = 0xFFFFFFFF
ALL = 0xFFFFFFFF


def ray_masks(ray_mask, n):
    """None / a scalar / n values → uint32[n]"""
    if ray_mask is None:
        return np.full(n, ALL, dtype=np.uint32)
    r = np.asarray(ray_mask)
    return np.full(n, int(r), dtype=np.uint32) if r.ndim == 0 else np.ascontiguousarray(r, dtype=np.uint32).reshape(n)


def filter_table(table, inst_mask, ray_mask):
    """the table of Scene.trace(rays)["table"] without the rows of invisible instances, in the same (double) order"""
    n = len(table["cand_off"]) - 1
    M = np.asarray(inst_mask, dtype=np.uint32)
    R = ray_masks(ray_mask, n)
    ray = table["ray"].astype(np.int64)
    keep = (M[table["instance"].astype(np.int64)] & R[ray]) != 0 if len(ray) else np.zeros(0, dtype=bool)
    cand_off = np.concatenate([[0], np.cumsum(np.bincount(ray[keep], minlength=n))]).astype(np.int64)
    return dict(ray=table["ray"][keep], instance=table["instance"][keep], shape=table["shape"][keep], vals=table["vals"][keep], cand_off=cand_off)


def select(table, n, tmax, dtype, first):
    """instances_ref.Scene.trace's selection over a table: (vals[n,3], instance[n], shape[n]); strict <, the earlier candidate keeps a tie"""
    ft = np.dtype(dtype).type
    tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
    vals = np.zeros((n, 3), dtype=ft)
    vals[:, 0] = np.inf
    inst = np.full(n, NONE, dtype=np.uint32)
    shape = np.full(n, NONE, dtype=np.uint32)
    off = table["cand_off"]
    for j in range(n):
        for c in range(int(off[j]), int(off[j + 1])):
            d = table["vals"][c, 0]
            if d < tm[j] and (first or d < vals[j, 0]):
                vals[j] = table["vals"][c]
                inst[j] = table["instance"][c]
                shape[j] = table["shape"][c]
                if first:
                    break
    return vals, inst, shape


def closest(table, inst_mask, ray_mask, n, tmax, dtype):
    return select(filter_table(table, inst_mask, ray_mask), n, tmax, dtype, False)


def first(table, inst_mask, ray_mask, n, tmax, dtype):
    return select(filter_table(table, inst_mask, ray_mask), n, tmax, dtype, True)


def allhits(table, inst_mask, ray_mask, n, tmax, dtype, sort=True):
    """(offsets[n+1] u32, instance, shape, vals[total,3]): instances_allhits_ref.rows over the filtered table"""
    return iar.rows(filter_table(table, inst_mask, ray_mask), n, tmax, dtype, sort)


def khits(table, inst_mask, ray_mask, n, tmax, k, dtype):
    """(instance[n,k], shape[n,k], vals[n,k,3]): instances_khits_ref.definition over the filtered table"""
    return ikh.definition(filter_table(table, inst_mask, ray_mask), n, tmax, k, dtype)


def brute_force(scene, rays, inst_mask, ray_mask, tmax, dtype):
    """no table: per ray, the visible instances of its top-level list in that list's order, each walked alone → per ray the list of
    (instance, shape, vals[3]) with distance < tmax in the double order"""
    import instances_ref as ir
    from oracle import orc
    n = len(rays)
    ft = np.dtype(dtype).type
    tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
    M = np.asarray(inst_mask, dtype=np.uint32)
    R = ray_masks(ray_mask, n)
    rays = np.ascontiguousarray(rays)
    toff, tidx, _, _ = orc.traverse_flat(scene.top, scene.w, rays)
    out = []
    for j in range(n):
        row = []
        for i in tidx[int(toff[j]):int(toff[j + 1])]:
            i = int(i)
            if (int(M[i]) & int(R[j])) == 0:
                continue
            orays = scene.object_rays(rays[j:j + 1], i)
            aabbs, tris = scene.trees[int(scene.tree_of[i])]
            off, idx, _, _ = orc.traverse_flat(scene.flats[int(scene.tree_of[i])], aabbs, orays)
            isect, _, _ = orc.triangle_stage(tris, orays, off, idx)
            for s, v in zip(idx.tolist(), isect):
                if v[0] < tm[j]:
                    row.append((i, int(s), v.copy()))
        out.append(row)
    assert ir.NONE == NONE
    return out
