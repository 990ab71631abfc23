"""Reference for the k-hit queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_khits_*), in two forms over
tests/instances_ref.py's candidate table: (a) the definition — the sorted rows of tests/instances_allhits_ref.py cut to k and padded — and
(b) the incremental list the kernel runs, restated in plain Python over the table in the double order.  Nothing else."""
import numpy as np

import instances_allhits_ref as iar

NONE = 0xFFFFFFFF


def padding(n, k, dtype):
    """n rows of k empty slots → (instance[n,k], shape[n,k], vals[n,k,3]): NONE, NONE and {+inf, 0, 0}"""
    vals = np.zeros((n, k, 3), dtype=dtype)
    vals[:, :, 0] = np.inf
    return np.full((n, k), NONE, dtype=np.uint32), np.full((n, k), NONE, dtype=np.uint32), vals


def cut_rows(rows_, n, k, dtype):
    """a sorted CSR (offsets, instance, shape, vals[total,3]) → its rows cut to the first k entries and padded"""
    off, inst, shape, vals = rows_
    oi, os_, ov = padding(n, k, dtype)
    for j in range(n):
        lo = int(off[j])
        m = min(k, int(off[j + 1]) - lo)
        oi[j, :m], os_[j, :m], ov[j, :m] = inst[lo:lo + m], shape[lo:lo + m], vals[lo:lo + m]
    return oi, os_, ov


def definition(table, n, tmax, k, dtype):
    """(a): table = Scene.trace(rays)["table"] of the UNCUT batch; tmax: None or n values"""
    return cut_rows(iar.rows(table, n, tmax, dtype, sort=True), n, k, dtype)


def incremental(table, n, tmax, k, dtype):
    """(b): per ray a list of at most k entries, ascending by distance.  While the list is not full every candidate enters; a full list
    accepts d iff d < L[k-1] and drops L[k-1]; an accepted d goes in front of the first element e with d < e, else to the end.  Every
    comparison is the strict < of T (the distances are T values; a Python float holds them exactly)."""
    ft = np.dtype(dtype).type
    tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
    off = table["cand_off"]
    oi, os_, ov = padding(n, k, dtype)
    for j in range(n):
        lo, hi = int(off[j]), int(off[j + 1])
        dist = table["vals"][lo:hi, 0]
        cand = np.nonzero(dist < tm[j])[0]                       # strict, in T: a miss (+inf) and a NaN never pass
        ld, lp = [], []                                         # the list: distances, positions in the table
        for c, d in zip(cand.tolist(), dist[cand].tolist()):
            if len(ld) == k:
                if not d < ld[-1]:
                    continue
                ld.pop(); lp.pop()
            hole = len(ld)
            while hole > 0 and d < ld[hole - 1]:                # the search from the back
                hole -= 1
            ld.insert(hole, d); lp.insert(hole, lo + c)
        m = len(lp)
        if m:
            oi[j, :m], os_[j, :m], ov[j, :m] = table["instance"][lp], table["shape"][lp], table["vals"][lp]
    return oi, os_, ov


def same(a, b):
    """two padded results, byte for byte"""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
