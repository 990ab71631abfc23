"""Reference for the radius-search queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_within_*): the definition
restated in Python over tests/instances_ref.py's Scene (its x, y, w, top, flats) and tests/knn_ref.py's distances, in the set's dtype T
with one rounded operation per step; not a test file.

Point p comes with m = max_dist; r2 = m * m; a negative or NaN m gives an empty row without a walk.
  top level (the FlatNode array over the world boxes, with p and r2):
    non-leaf entry: md = aabb.min_distance_squared(p); entry_index iff md <= r2, else exit_index
    leaf entry (instance i): walk instance i, then exit_index
  instance i (member t = tree_of[i]):
    q = forward(Y_i, p);  F = (f[0] + f[1]) + f[2] with f[k] = (Y_i[k][0]^2 + Y_i[k][1]^2) + Y_i[k][2]^2;  r2o = r2 * F
    member t's FlatNode array with q and r2o: a non-leaf entry is entered iff md <= r2o; a leaf entry (shape s) gives
    d = triangle_dist2(forward(X_i, tri_s), p) — the WORLD triangle and the WORLD point — and (i, s) is a candidate iff d <= r2
`brute` is the same candidate predicate over all (instance, triangle) pairs with no tree and no object frame."""
import os
import re

import numpy as np

import instances_ref as ir
import knn_ref as kr
import knn_tree_ref as ktr
import within_ref as wr

NONE = kr.NONE


def stretch(y):
    """F: the squared Frobenius norm of the 3x3 part of y (3, 4), row by row in row3's order"""
    f = [(y[k, 0] * y[k, 0] + y[k, 1] * y[k, 1]) + y[k, 2] * y[k, 2] for k in range(3)]
    return (f[0] + f[1]) + f[2]


def world_triangles(sc):
    """per instance its member's triangles under X_i, (n_tris, 3, 3) in T: w[v][k] = forward(X_i, tri[v])[k]"""
    out = []
    with np.errstate(all="ignore"):
        for i in range(len(sc.x)):
            _, tris = sc.trees[int(sc.tree_of[i])]
            out.append(np.ascontiguousarray(ir.forward(sc.x[i], tris.reshape(-1, 3)).reshape(-1, 3, 3).astype(sc.ft)))
    return out


def _top_instances(top_lists, md, r2):
    """the instances the top-level loop enters, in list order"""
    entry, exit_, shape = top_lists
    out, i, n = [], 0, len(entry)
    while i < n:
        if entry[i] == NONE:
            out.append(shape[i]); i = exit_[i]
        else:
            i = entry[i] if md[i] <= r2 else exit_[i]
    return out


def rows(sc, points, max_dist, stats=None):
    """the definition for every point → per point the candidates [(d, instance, shape)] in the double order.  stats (a dict, optional)
    receives `instances` (instances entered) and `entries` (member entries visited) summed over the batch"""
    ft = sc.ft
    pts = np.ascontiguousarray(points, dtype=ft).reshape(-1, 3)
    lim = ktr.limits(max_dist, len(pts), ft)
    out = [[] for _ in pts]
    n_inst = n_entries = 0
    if len(sc.x) == 0:
        return out
    top_lists = kr.flat_lists(sc.top)
    member_lists = [kr.flat_lists(f) for f in sc.flats]
    wtris = world_triangles(sc)
    with np.errstate(all="ignore"):
        big_f = [ft(stretch(y)) for y in sc.y]
        for j, p in enumerate(pts):
            if lim[j] is False:
                continue
            r2 = ft(lim[j])
            mdt = kr.aabb_min_dist2_v(np.ascontiguousarray(sc.top["min"]), np.ascontiguousarray(sc.top["max"]), p).astype(ft).tolist()
            row = out[j]
            for i in _top_instances(top_lists, mdt, r2.item()):
                n_inst += 1
                t = int(sc.tree_of[i])
                flat = sc.flats[t]
                q = ir.forward(sc.y[i], p).astype(ft)
                r2o = ft(r2 * big_f[i]).item()
                md = kr.aabb_min_dist2_v(np.ascontiguousarray(flat["min"]), np.ascontiguousarray(flat["max"]), q).astype(ft).tolist()
                d = kr.triangle_dist2_v(wtris[i], p).astype(ft).tolist()
                entry, exit_, shape = member_lists[t]
                k, n = 0, len(entry)
                while k < n:
                    n_entries += 1
                    if entry[k] == NONE:
                        s = shape[k]
                        if d[s] <= r2.item():
                            row.append((d[s], i, s))
                        k = exit_[k]
                    else:
                        k = entry[k] if md[k] <= r2o else exit_[k]
    if stats is not None:
        stats["instances"] = n_inst
        stats["entries"] = n_entries
    return out


def brute(sc, points, max_dist):
    """per point the set {(instance, shape) : d <= r2} over all pairs, no tree"""
    ft = sc.ft
    pts = np.ascontiguousarray(points, dtype=ft).reshape(-1, 3)
    lim = ktr.limits(max_dist, len(pts), ft)
    wtris = world_triangles(sc)
    out = []
    with np.errstate(all="ignore"):
        for j, p in enumerate(pts):
            got = set()
            if lim[j] is not False:
                r2 = ft(lim[j])
                for i, wt in enumerate(wtris):
                    d = kr.triangle_dist2_v(wt, p).astype(ft)
                    got.update((i, int(s)) for s in np.nonzero(d <= r2)[0])
            out.append(got)
    return out


def csr(list_rows, dtype, sort=True):
    """rows in the double order → (offsets[n + 1] u32, instance[total] u32, shape[total] u32, dist[total]) as
    bvhgpu_hits_fetch_instances_within gives them"""
    offsets = np.zeros(len(list_rows) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in list_rows], dtype=np.uint64).astype(np.uint32)
    dd, ii, ss = [], [], []
    for r in list_rows:
        if sort:
            r = sorted(r, key=lambda e: e[0])                 # sorted() is stable; no NaN among candidates
        dd += [e[0] for e in r]; ii += [e[1] for e in r]; ss += [e[2] for e in r]
    return offsets, np.asarray(ii, dtype=np.uint32), np.asarray(ss, dtype=np.uint32), np.sqrt(np.asarray(dd, dtype=dtype))


def within(sc, points, max_dist, sort=True):
    return csr(rows(sc, points, max_dist), sc.ft, sort)


def engine_thresholds(root):
    """(INST_WITHIN_LANE_ROW_MAX, INST_WITHIN_LDS_ROW_MAX) as bvh_amd/csrc/instances_within.hip names them"""
    src = open(os.path.join(root, "bvh_amd", "csrc", "instances_within.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))
                 for name in ("INST_WITHIN_LANE_ROW_MAX", "INST_WITHIN_LDS_ROW_MAX"))


# ---------------------------------------------------------------- the scenes the CPU and the GPU tests share
LINE_POS, LINE_INSTANCES = 64, 64


def line_instances(dtype):
    """One member: within_ref.line_scene(copies=1, n_pos=64), point triangles at x = 1 .. 64.  64 instances: even k the identity plus
    64 k along x (x = 64 k + 1 .. 64 k + 64), odd k the half turn diag(-1, -1, 1) plus 64 k + 65 (the same positions, the member running
    backwards); every operation is exact in f32.  Together: one point triangle at every integer x = 1 .. 4096.  Instances 64 and 65 are
    coincident copies of 0 and 41: every distance there appears twice.  → (trees, tree_of, x[66, 3, 4])"""
    aabbs, tris = wr.line_scene(dtype, copies=1, n_pos=LINE_POS)
    n = LINE_INSTANCES
    x = np.zeros((n + 2, 3, 4), dtype=dtype)
    for k in range(n):
        if k % 2 == 0:
            x[k, :, :3] = np.eye(3); x[k, 0, 3] = LINE_POS * k
        else:
            x[k, :, :3] = np.diag([-1.0, -1.0, 1.0]); x[k, 0, 3] = LINE_POS * k + LINE_POS + 1
    x[n], x[n + 1] = x[0], x[41]
    return [(aabbs, tris)], np.zeros(n + 2, dtype=np.uint32), x


def cluster_points(n_instances, dtype, n=600):
    """the issue's draw for test_instances_cpu.case(orc, dtype, n_instances): points U(-11, 11)^3, limits U(0.1, 4), seed 500 + n_instances"""
    rng = np.random.default_rng(500 + n_instances)
    pts = rng.uniform(-11.0, 11.0, size=(n, 3)).astype(dtype)
    m = rng.uniform(0.1, 4.0, size=n).astype(dtype)
    return pts, m
