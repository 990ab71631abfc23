"""Reference for the all-hits queries over instanced scenes (include/bvh_mi355x.h, bvhgpu_instances_allhits_*): the candidate table of
tests/instances_ref.py's Scene.trace, cut by tmax and sorted stably.  Nothing else."""
import numpy as np


def rows(table, n, tmax, dtype, sort=True):
    """table: Scene.trace(rays)["table"] of the UNCUT batch; tmax: None or n values → (offsets[n+1] u32, instance, shape, vals[total,3])"""
    ft = np.dtype(dtype).type
    tm = np.full(n, np.inf, dtype=ft) if tmax is None else np.asarray(tmax, dtype=ft)
    off = table["cand_off"]
    keep_all = []
    counts = np.zeros(n, dtype=np.int64)
    for j in range(n):
        lo, hi = int(off[j]), int(off[j + 1])
        d = table["vals"][lo:hi, 0]
        keep = np.nonzero(d < tm[j])[0]                      # strict, in T: a miss (+inf) and a NaN never pass
        if sort:
            keep = keep[np.argsort(d[keep], kind="stable")]
        keep_all.append(lo + keep)
        counts[j] = len(keep)
    sel = np.concatenate(keep_all) if keep_all else np.zeros(0, dtype=np.int64)
    sel = sel.astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return (offsets, np.ascontiguousarray(table["instance"][sel], dtype=np.uint32), np.ascontiguousarray(table["shape"][sel], dtype=np.uint32),
            np.ascontiguousarray(table["vals"][sel], dtype=ft).reshape(-1, 3))


def engine_thresholds(root):
    """(INST_ALLHITS_LANE_ROW_MAX, INST_ALLHITS_LDS_ROW_MAX) as bvh_amd/csrc/instances_allhits.hip names them"""
    import os
    import re
    src = open(os.path.join(root, "bvh_amd", "csrc", "instances_allhits.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))
                 for name in ("INST_ALLHITS_LANE_ROW_MAX", "INST_ALLHITS_LDS_ROW_MAX"))
