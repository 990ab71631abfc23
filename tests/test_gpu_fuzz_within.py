"""Fuzz over within_batch (bvhgpu_within_*) on the random scenes of tests/fuzz_scenes.py, with tests/test_gpu_fuzz_queries.py's
conventions: the same seeds (16 combinations of dtype, scene character and scale band by default, all 32 with BVH_FUZZ_SEEDS=32), the same
scenes, points and drawn limits as the k-nearest families there — the k-th neighbour distance x U(0.3, 1.7), a fifth of the points pinned
to 0, -1, NaN and +inf — one build per seed, and every leg against tests/within_ref.py byte for byte: both shape distances, sorted rows,
list order and counts, points in host memory and (one shape distance per seed) in HBM."""
import os
import time

import numpy as np
import pytest

import fuzz_scenes as fs
import within_ref as wr
from test_gpu_within import _call, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


@pytest.mark.parametrize("seed", range(int(os.environ.get("BVH_FUZZ_SEEDS", fs.DEFAULT_SEEDS))))
def test_fuzz_within(eng, seed):
    t0 = time.perf_counter()
    c = fs.case(seed)
    scene, ex = c["scene"], c["extras"]
    dtype, tri, aabbs, kpts = scene["dtype"], scene["tri"], scene["aabbs"], ex["kpts"]
    name = fs.label(seed)
    rows = {kind: wr.rows(c["oflat"], aabbs, kpts, ex["max_dist"][kind], tri if kind else None) for kind in (0, 1)}
    t1 = time.perf_counter()

    ctx = eng.Context(0)
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    flat = bvh.flatten()
    assert flat.nodes.tobytes() == c["oflat"].tobytes(), name   # a wrong tree must not show up as query failures
    flat.set_triangles(tri)
    on_device = seed % 2
    for kind in (0, 1):
        m = ex["max_dist"][kind]
        for device in ((False, True) if kind == on_device else (False,)):
            for sort in (True, False):
                _same(_call(flat, kpts, m, kind, sort, False, device), wr.csr(rows[kind], dtype, sort), (name, kind, sort, device))
            o, s, d = _call(flat, kpts, m, kind, True, True, device)
            assert o.tobytes() == wr.csr(rows[kind], dtype, False)[0].tobytes() and len(s) == 0 and len(d) == 0, (name, kind, "count only")
    n = np.asarray([len(r[0]) for r in rows[0]])
    print(f"{name}: n = {scene['n']}, {len(kpts)} points, rows mean {n.mean():.1f} max {n.max()}, reference {t1 - t0:.2f} s, GPU side {time.perf_counter() - t1:.2f} s")
