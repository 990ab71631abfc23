"""Reference for the instanced ray queries (include/bvh_mi355x.h, bvhgpu_instances_*): the definition restated with numpy in the set's
dtype T, one rounded operation per step, over the oracle's build / flatten / traverse / triangle stage.

A member tree is (aabbs[n,6], tris[n,3,3]); instance i is (tree_of[i], X_i row-major 3x4, object -> world).
"""
import numpy as np

from oracle import orc

NONE = 0xFFFFFFFF


def _join_min(a, axis=0):
    """min with -0 below +0 (exact, order-free on NaN-free data)"""
    m = a.min(axis=axis)
    neg = ((a == 0) & np.signbit(a)).any(axis=axis)
    return np.where(m == 0, np.where(neg, a.dtype.type(-0.0), a.dtype.type(0.0)), m)


def _join_max(a, axis=0):
    m = a.max(axis=axis)
    pos = ((a == 0) & ~np.signbit(a)).any(axis=axis)
    return np.where(m == 0, np.where(pos, a.dtype.type(0.0), a.dtype.type(-0.0)), m)


def tree_bounds(aabbs):
    """B_t = {min of the mins, max of the maxes} over the tree's shape AABBs"""
    a = np.asarray(aabbs).reshape(-1, 6)
    return np.concatenate([_join_min(a[:, :3]), _join_max(a[:, 3:])]).astype(a.dtype)


def forward(m, p):
    """w[k] = ((m[k][0]*p[0] + m[k][1]*p[1]) + m[k][2]*p[2]) + m[k][3]; m: (..., 3, 4), p: (..., 3)"""
    return ((m[..., 0] * p[..., None, 0] + m[..., 1] * p[..., None, 1]) + m[..., 2] * p[..., None, 2]) + m[..., 3]


def linear(m, p):
    """(m[k][0]*p[0] + m[k][1]*p[1]) + m[k][2]*p[2]"""
    return (m[..., 0] * p[..., None, 0] + m[..., 1] * p[..., None, 1]) + m[..., 2] * p[..., None, 2]


def inverse(x):
    """Y_i of X_i (n, 3, 4): cofactors a*b - c*d, det = (m00*C00 + m01*C01) + m02*C02, r = 1/det, y[k][j] = C[j][k]*r,
    y[k][3] = -(((y[k][0]*m03) + (y[k][1]*m13)) + y[k][2]*m23)"""
    m = x
    ft = m.dtype.type

    def cof(a, b, c, d):
        return m[:, a[0], a[1]] * m[:, b[0], b[1]] - m[:, c[0], c[1]] * m[:, d[0], d[1]]

    Cf = np.empty((len(m), 3, 3), dtype=m.dtype)
    Cf[:, 0, 0] = cof((1, 1), (2, 2), (1, 2), (2, 1))
    Cf[:, 0, 1] = cof((1, 2), (2, 0), (1, 0), (2, 2))
    Cf[:, 0, 2] = cof((1, 0), (2, 1), (1, 1), (2, 0))
    Cf[:, 1, 0] = cof((0, 2), (2, 1), (0, 1), (2, 2))
    Cf[:, 1, 1] = cof((0, 0), (2, 2), (0, 2), (2, 0))
    Cf[:, 1, 2] = cof((0, 1), (2, 0), (0, 0), (2, 1))
    Cf[:, 2, 0] = cof((0, 1), (1, 2), (0, 2), (1, 1))
    Cf[:, 2, 1] = cof((0, 2), (1, 0), (0, 0), (1, 2))
    Cf[:, 2, 2] = cof((0, 0), (1, 1), (0, 1), (1, 0))
    with np.errstate(all="ignore"):
        det = (m[:, 0, 0] * Cf[:, 0, 0] + m[:, 0, 1] * Cf[:, 0, 1]) + m[:, 0, 2] * Cf[:, 0, 2]
        r = ft(1) / det
        y = np.empty_like(m)
        for k in range(3):
            for j in range(3):
                y[:, k, j] = Cf[:, j, k] * r
            y[:, k, 3] = -(((y[:, k, 0] * m[:, 0, 3]) + (y[:, k, 1] * m[:, 1, 3])) + y[:, k, 2] * m[:, 2, 3])
    return y


def world_boxes(bounds, tree_of, x):
    """W_i: min / max over the 8 corners of B_tree_of[i]; bit k of the corner number picks the max on axis k"""
    n = len(x)
    corners = np.empty((8, n, 3), dtype=x.dtype)
    with np.errstate(all="ignore"):
        for c in range(8):
            p = np.stack([bounds[tree_of, 3 + k] if (c >> k) & 1 else bounds[tree_of, k] for k in range(3)], axis=1)
            corners[c] = forward(x, p)
    return np.concatenate([_join_min(corners), _join_max(corners)], axis=1).astype(x.dtype) if n else np.zeros((0, 6), dtype=x.dtype)


class Scene:
    """trees: [(aabbs[n,6], tris[n,3,3])] in T; tree_of: n ints; xforms: n x 12 or n x 3 x 4 in T"""

    def __init__(self, trees, tree_of, xforms, ft):
        self.ft = np.dtype(ft).type
        self.trees = [(np.ascontiguousarray(a, dtype=ft).reshape(-1, 6), np.ascontiguousarray(t, dtype=ft).reshape(-1, 3, 3)) for a, t in trees]
        self.flats = [orc.flatten(orc.build(a).nodes) for a, _ in self.trees]
        self.tree_of = np.asarray(tree_of, dtype=np.int64).reshape(-1)
        self.bounds = np.stack([tree_bounds(a) for a, _ in self.trees]) if self.trees else np.zeros((0, 6), dtype=ft)
        self.pose(xforms)

    def pose(self, xforms):
        self.x = np.ascontiguousarray(xforms, dtype=self.ft).reshape(-1, 3, 4)
        assert len(self.x) == len(self.tree_of)
        self.y = inverse(self.x)
        self.w = world_boxes(self.bounds, self.tree_of, self.x)
        self.top = orc.flatten(orc.build(self.w).nodes)
        return self

    def object_rays(self, rays, i):
        """{o', d', 1/d'} of `rays` in instance i's frame, assembled by hand"""
        out = np.zeros(len(rays), dtype=rays.dtype)
        y = self.y[i]
        with np.errstate(all="ignore"):
            out["o"] = forward(y, rays["o"])
            out["d"] = linear(y, rays["d"])
            out["inv"] = self.ft(1) / out["d"]
        return out

    def trace(self, rays, tmax=None):
        """returns dict: top (offsets, indices) = I_j as a CSR; table = the candidate table in the double order, as arrays ray / instance /
        shape / vals[.,3] with CSR offsets `cand_off`; closest and first = (vals[n,3], instance[n], shape[n])"""
        ft = self.ft
        n = len(rays)
        rays = np.ascontiguousarray(rays)
        toff, tidx, _, _ = orc.traverse_flat(self.top, self.w, rays)
        ray_of = np.repeat(np.arange(n), np.diff(toff.astype(np.int64)))          # ray of every (ray, instance) visit
        pos_of = np.arange(len(tidx)) - toff.astype(np.int64)[ray_of]             # ... and its position in I_j
        c_ray, c_pos, c_k, c_inst, c_shape, c_vals = [], [], [], [], [], []
        for i in np.unique(tidx):
            sel = np.nonzero(tidx == i)[0]
            rid = ray_of[sel]
            orays = self.object_rays(rays[rid], int(i))
            aabbs, tris = self.trees[int(self.tree_of[i])]
            off, idx, _, _ = orc.traverse_flat(self.flats[int(self.tree_of[i])], aabbs, orays)
            isect, _, _ = orc.triangle_stage(tris, orays, off, idx)
            cnt = np.diff(off.astype(np.int64))
            c_ray.append(np.repeat(rid, cnt)); c_pos.append(np.repeat(pos_of[sel], cnt))
            c_k.append(np.arange(len(idx)) - np.repeat(off.astype(np.int64)[:-1], cnt))
            c_inst.append(np.full(len(idx), i, dtype=np.uint32)); c_shape.append(idx.astype(np.uint32)); c_vals.append(isect)
        if c_ray:
            c_ray, c_pos, c_k = np.concatenate(c_ray), np.concatenate(c_pos), np.concatenate(c_k)
            c_inst, c_shape, c_vals = np.concatenate(c_inst), np.concatenate(c_shape), np.concatenate(c_vals)
            order = np.lexsort((c_k, c_pos, c_ray))
            c_ray, c_inst, c_shape, c_vals = c_ray[order], c_inst[order], c_shape[order], c_vals[order]
        else:
            c_ray = np.zeros(0, dtype=np.int64); c_inst = np.zeros(0, dtype=np.uint32); c_shape = np.zeros(0, dtype=np.uint32)
            c_vals = np.zeros((0, 3), dtype=ft)
        cand_off = np.concatenate([[0], np.cumsum(np.bincount(c_ray, minlength=n))]).astype(np.int64)
        tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
        res = {}
        for name in ("closest", "first"):
            vals = np.zeros((n, 3), dtype=ft); vals[:, 0] = np.inf
            inst = np.full(n, NONE, dtype=np.uint32); shape = np.full(n, NONE, dtype=np.uint32)
            for j in range(n):
                for c in range(cand_off[j], cand_off[j + 1]):
                    d = c_vals[c, 0]
                    if d < tm[j] and (name == "first" or d < vals[j, 0]):   # strict, in T: the earlier candidate keeps a tie
                        vals[j] = c_vals[c]; inst[j] = c_inst[c]; shape[j] = c_shape[c]
                        if name == "first":
                            break
            res[name] = (vals, inst, shape)
        res["top"] = (toff, tidx)
        res["table"] = dict(ray=c_ray, instance=c_inst, shape=c_shape, vals=c_vals, cand_off=cand_off)
        return res
