"""bench.py is load-bearing evidence (the driver's record is its one JSON line), so its N = 1 sections run here at a small size on every GPU
test round: the headline with its roofline lookup by the kernel name the LIBRARY reports, `step_excludes` (ray generation / eager FlatNode
array / host I/O beside `value`), the reference's whole harness loop as extra configs with parity and the CPU loop beside it, the fair CPU
baseline, and `--harness` as the headline of a run (what the profile rounds use)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_args, env_extra=None):
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cubes", "2500", "--rays", "200000", "--steps", "5", "--warmup", "2",
           "--settle-steps", "10", "--extra-steps", "3", "--cpu-sample-rays", "100000", "--full"] + extra_args
    detail_file = os.path.join(tempfile.mkdtemp(prefix="bvh_bench_"), "detail.json")
    p = subprocess.run(cmd + ["--detail-out", detail_file], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and p.stdout.strip().splitlines()[-1] == lines[0], p.stdout[-2000:]     # ONE line, and it is the last one
    assert len(lines[0]) < 8192, len(lines[0])                                                     # the driver must be able to read it (BENCH_r05)
    return json.loads(lines[0]), json.loads(open(detail_file).read())


def test_default_line_sections_at_a_small_size():
    out, det = _run([], {"BVH_BENCH_EXTRAS": "0,1,8"})      # extras: the harness loop on the cube scene — closest, triangles, closest in f64
    assert out["value"] > 0 and out["n_gpus"] == 1 and out["steps"] == 5 and out["warmup"] == 2 and out["settle_steps"] == 10
    assert out["value"] == det["value"] and out["config"]["flat_array"] == "eager"    # the FlatNode array is written inside the timed step
    assert out["parity"]["equal"] is True and out["parity"]["checked_rays"] == 200000
    roof = out["roofline"]
    assert roof["kernel"].startswith("bvhgpu::k_traverse_wide<float, 0, ") and roof["kernel"].endswith(">")      # as the library spells it
    assert roof["algorithmic_frac"] > 0 and set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(roof)
    ex, exd = out["step_excludes"], det["step_excludes"]
    for k in ("with_ray_gen", "lazy_flat_array", "all_arrays_eager", "beside_flat_array", "host_io"):
        assert ex[k] > 0 and exd[k]["value"] == ex[k] and exd[k]["ms_per_step"] > 0, ex
    pg, pn = exd["host_io"]["paths"]["pageable"], exd["host_io"]["paths"]["pinned"]
    assert pg["bytes_per_step"]["aabbs_up"] == 2500 * 12 * 24 and pg["bytes_per_step"]["rays_up"] == 200000 * 36
    assert pn["bytes_per_step"]["rays_up"] == 200000 * 24 and pn["csr_equal_to_pageable_path"] is True      # origins + directions only
    p1 = exd["host_io"]["paths"]["pinned_one_call"]
    assert p1["csr_equal_to_pageable_path"] is True and p1["value"] > 0
    assert ex["host_io"] == max(pg["value"], pn["value"], p1["value"]) < out["value"]          # PCIe-inclusive: never the faster one
    assert out["pipelined"]["hits_every_step_equal"] is True
    modes = []
    for e, ed in zip(out["extra_configs"], det["extra_configs"]):
        assert "error" not in e, ed
        modes.append((e["harness"], e["dtype"]))
        assert e["workload"] == "cubes120k+" + e["harness"] and e["parity"]["equal"] is True and e["parity"]["checked_rays"] == e["rays_this_rank"]
        # (the f64 closest-hit walk runs over the tree's f32 guide boxes: k_traverse_wide<float, 3, 2, 1024, 8, 1>)
        assert e["ray_gen_ms"] > 0 and ed["roofline"]["kernel"].startswith("bvhgpu::k_traverse_wide<float, %d, " % (3 if e["harness"] == "closest" else 2))
        assert ed["roofline"]["kernel"].endswith(", 1>" if e["dtype"] == "f64" else ", 0>")
        if e["dtype"] == "f32":
            assert e["cpu_harness"] > 0 and e["speedup_vs_cpu_harness"] > 0 and ed["cpu_harness"]["oracle_library"].startswith("liboracle")
    assert modes == [("closest", "f32"), ("triangles", "f32"), ("closest", "f64")]
    cb, cbd = out["cpu_baseline"], det["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] >= cb["value_median"] > 0 and len(cb["host_load_1m"]) == 2 and len(cb["sample"]) < 220
    assert cbd["build_threads"] >= 1 and cbd["build_ms"] <= cbd["build_ms_serial"] * 1.05 and set(cbd["legs"]) == {"free", "pinned"} and cb["threads"] in cbd["legs"]


@pytest.mark.parametrize("mode", ["closest", "triangles"])
def test_harness_as_the_headline(mode):
    """`bench.py --harness M`: the step is ray generation + build + flatten + walk + triangle stage (intersect_bh, testbase.rs:819-837); the line is
    tagged so that its profile is looked up under its own workload name"""
    out, det = _run(["--harness", mode, "--no-extra", "--no-cpu-baseline", "--pipeline-streams", "0"])
    assert out["workload_name"] == "cubes120k+" + mode and out["harness"] == mode and out["value"] > 0
    assert out["parity"]["equal"] is True and out["cpu_harness"]["value"] > 0
    assert "intersect_bh" in out["config"]["workload"] and out["phases_ms"]["ray_gen_ms"] > 0
    assert "step_excludes" not in out        # (those compare against the index step of `value`: not measured beside a harness headline)


def test_plain_run_times_the_headline_and_dumps_what_it_computed(tmp_path):
    """Without --full a run is the headline alone: exactly K timed steps (the regions add up to them), the line's contract keys, no section
    beside it, no detail file.  --dump-outputs writes the last step's FlatNode array and CSR, and those are the oracle's for the same inputs."""
    import bvh_amd
    import numpy as np
    from bvh_amd import testbase as tb
    from oracle import orc
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cubes", "2500", "--rays", "200000", "--steps", "7", "--warmup", "2",
           "--settle-steps", "10", "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "Mrays/s (build+traverse)" and out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 7 and out["value"] > 0 and out["ms_per_step"] > 0 and len(out["regions_ms_per_step"]) == 5
    assert abs(out["value"] - 200000 / (out["ms_per_step"] * 1e-3) / 1e6) <= 2e-3 * out["value"]     # (both rounded on the line)
    for k in ("parity", "roofline", "phases_ms", "pipelined", "step_excludes", "extra_configs", "cpu_baseline", "detail"):
        assert k not in out, k
    names = sorted(f.name for f in dump.iterdir())
    assert names == ["flat_bounds.npy", "flat_bounds_nonfinite.npy", "flat_links.npy", "hit_indices.npy", "hit_offsets.npy"], names
    assert sum(f.stat().st_size for f in dump.iterdir()) <= 64_000_000
    _, aabbs = tb.create_n_cubes(2500)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    ooff, oidx, _, _ = orc.traverse_flat(oflat, aabbs, orc.create_rays(0, 200000), threads=orc.max_threads())
    got = {n[:-4]: np.load(dump / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["hit_offsets"], ooff.astype(np.float64)) and np.array_equal(got["hit_indices"], oidx.astype(np.float64))
    # the shape entries' Aabb::empty() (+inf, -inf): 0 in flat_bounds, +1 / -1 in flat_bounds_nonfinite
    v, c = got["flat_bounds"], got["flat_bounds_nonfinite"]
    assert set(np.unique(c)) == {-1.0, 0.0, 1.0} and not v[c != 0].any()
    assert np.array_equal(np.where(c == 1, np.inf, np.where(c == -1, -np.inf, v)), np.concatenate([oflat["min"], oflat["max"]], axis=1))
    assert np.array_equal(got["flat_links"], np.stack([oflat["entry"], oflat["exit"], oflat["shape"]], axis=1).astype(np.float64))


@pytest.mark.parametrize("mode", ["closest", "triangles"])
def test_plain_harness_run_dumps_its_results(mode, tmp_path):
    """--dump-outputs under --harness: the nearest hit per ray (closest) or the CSR with every candidate's Intersection (triangles)"""
    import bvh_amd
    import numpy as np
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cubes", "2500", "--rays", "200000", "--steps", "5", "--warmup", "2",
           "--settle-steps", "10", "--harness", mode, "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["workload_name"] == "cubes120k+" + mode and out["steps"] == 5 and "parity" not in out
    got = {f.name[:-4]: np.load(f) for f in tmp_path.iterdir()}
    assert all(np.isfinite(a).all() for a in got.values())     # (misses' infinite distances are coded in <name>_nonfinite)
    base = {k for k in got if not k.endswith("_nonfinite")}
    assert all(k[:-len("_nonfinite")] in base and got[k].shape == got[k[:-len("_nonfinite")]].shape for k in set(got) - base)
    assert got["flat_links"].shape[1] == 3 and got["flat_bounds"].dtype == np.float32 and "flat_bounds_nonfinite" in got
    if mode == "closest":
        assert base == {"flat_bounds", "flat_links", "closest_isect", "closest_shape"}
        assert got["closest_isect"].shape == (200000, 3) and got["closest_shape"].shape == (200000,)
    else:
        assert base == {"flat_bounds", "flat_links", "hit_offsets", "hit_indices", "triangle_isect"}
        assert got["hit_offsets"][-1] == len(got["hit_indices"]) == len(got["triangle_isect"]) > 0
