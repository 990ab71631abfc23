"""The walk dispatch table as a whole: which kernel a batch is handed to (bvhgpu_hits_walk_kernel) and how its hits are handed over
(bvhgpu_hits_walk_info), for every output x dtype x tuning combination below, pinned against tests/golden/walk_dispatch.json; and, for
the unordered batches, results byte-equal to the same batch walked one ray per lane (BVHGPU_TUNE_TRAVERSE_VARIANT = 0).

The golden file is written by this module's own recorder (`python tests/test_gpu_walk_dispatch.py [out.json]`, format: unpack_golden)
and committed as recorded: a change of the dispatch is a change of that file, made on purpose.

Scene: create_n_cubes(100) (1 200 triangles: deep enough for the cut into 16 items), the first 2 048 rays of the bench stream, and
BVHGPU_TUNE_TRAVERSE_LDS_MIN_RAYS = 0 so that the size thresholds need no large batch."""
import itertools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_dispatch.json")
N_RAYS = 2048
DTYPES = {"f32": np.float32, "f64": np.float64}
OUTPUTS = ["indices", "indices_stats", "t_slice", "triangles", "closest", "any"]
VARIANTS = [None, 0, 2, 3]          # BVHGPU_TUNE_TRAVERSE_VARIANT (None: a context whose knob was never set)
ITEMS = [-1, 0, 1, 2]               # BVHGPU_TUNE_WIDE_ITEMS_LOG4
GUIDE = [0, 1]                      # BVHGPU_TUNE_WIDE_F64_GUIDE
REC8 = [0, 1]                       # BVHGPU_TUNE_WIDE_REC8
COHERENT = [False, True]
ORDERS = ["nearest", "farthest", "nearest_heap", "farthest_heap"]
ORDERED_OUTPUTS = ["indices", "triangles", "closest"]
QUERY_KINDS = ["aabb", "point", "ball"]
QUERY_VARIANTS = [0, 1]             # BVHGPU_TUNE_QUERY_VARIANT

_scene_cache = {}
_reference_cache = {}


def _engine():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


def _scene(dname):
    """(tris, aabbs, rays) in the dtype, made once"""
    if dname not in _scene_cache:
        from bvh_amd import testbase as tb
        from oracle import orc
        dt = DTYPES[dname]
        tris, aabbs = tb.create_n_cubes(100)
        _scene_cache[dname] = (tris.astype(dt), aabbs.astype(dt), orc.create_rays(0, N_RAYS, dtype=dt))
    return _scene_cache[dname]


def _tree(eng, dname, tune):
    """a fresh context, tree and result object: what bvhgpu_hits_walk_info reports depends on this object's batches only"""
    from bvh_amd import _lib
    tris, aabbs, rays = _scene(dname)
    ctx = eng.Context(0)
    ctx.set_tuning(_lib.TUNE_TRAVERSE_LDS_MIN_RAYS, 0)
    for k, v in tune.items():
        ctx.set_tuning(k, v)
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_triangles(tris)
    return ctx, flat, eng.RayBatch(len(rays), DTYPES[dname], host=np.ascontiguousarray(rays))


def _walk(flat, rb, output, coherent=False, order=None):
    """run one batch; returns its results as a tuple of byte strings"""
    if output == "indices":
        off, idx, _, _ = flat.traverse_batch(rb, coherent=coherent, order=order)
        res = (off, idx)
    elif output == "indices_stats":
        off, idx, _, _ = flat.traverse_batch(rb, stats=True, coherent=coherent, order=order)
        res = (off, idx)
    elif output == "t_slice":
        off, idx, ts, _ = flat.traverse_batch(rb, want_t=True, coherent=coherent, order=order)
        res = (off, idx, ts)
    elif output == "triangles":
        off, idx, isect, _ = flat.intersect_triangles(rb, coherent=coherent, order=order)
        res = (off, idx, isect)
    elif output == "closest":
        isect, shape, _ = flat.closest_hits(rb, coherent=coherent, order=order)
        res = (isect, shape)
    else:
        isect, shape = flat.any_hits(rb, None, coherent=coherent)
        res = (isect, shape)
    return tuple(a.tobytes() for a in res)


def _entry(flat):
    return [flat._hits.walk_kernel(), flat._hits.walk_flags()]


def _reference(eng, dname, output):
    """the batch walked one ray per lane per launch, every other knob at its default: computed once, shared by all cases"""
    key = (dname, output)
    if key not in _reference_cache:
        from bvh_amd import _lib
        _, flat, rb = _tree(eng, dname, {_lib.TUNE_TRAVERSE_VARIANT: 0})
        _reference_cache[key] = _walk(flat, rb, output)
        assert flat._hits.walk_kernel().startswith("bvhgpu::k_traverse<"), flat._hits.walk_kernel()
    return _reference_cache[key]


def ray_cases(eng, dname, output):
    """yields (key, [kernel, flags], results) for every tuning combination of one dtype and output"""
    from bvh_amd import _lib
    for variant in VARIANTS:
        ctx, flat, rb = _tree(eng, dname, {} if variant is None else {_lib.TUNE_TRAVERSE_VARIANT: variant})
        for items, guide, rec8, coherent in itertools.product(ITEMS, GUIDE, REC8, COHERENT):
            ctx.set_tuning(_lib.TUNE_WIDE_ITEMS_LOG4, items)
            ctx.set_tuning(_lib.TUNE_WIDE_F64_GUIDE, guide)
            ctx.set_tuning(_lib.TUNE_WIDE_REC8, rec8)
            res = _walk(flat, rb, output, coherent=coherent)
            vname = "default" if variant is None else str(variant)
            yield f"{dname}|{output}|variant={vname}|items={items}|guide={guide}|rec8={rec8}|coherent={int(coherent)}", _entry(flat), res


def ordered_cases(eng, dname):
    for output, order in itertools.product(ORDERED_OUTPUTS, ORDERS):
        _, flat, rb = _tree(eng, dname, {})
        _walk(flat, rb, output, order=order)
        yield f"{dname}|{output}|order={order}", _entry(flat)


def _queries(dname, kind):
    _, aabbs, _ = _scene(dname)
    centre = (aabbs[:, :3] + aabbs[:, 3:]) / 2
    if kind == "aabb":
        return aabbs
    if kind == "point":
        return np.ascontiguousarray(centre)
    return np.ascontiguousarray(np.concatenate([centre, np.full((len(centre), 1), 1.5, dtype=aabbs.dtype)], axis=1))


def query_cases(eng, dname):
    from bvh_amd import _lib
    for kind in QUERY_KINDS:
        for knob in QUERY_VARIANTS:
            _, flat, _ = _tree(eng, dname, {_lib.TUNE_QUERY_VARIANT: knob})
            off, idx = flat.query_batch(kind, _queries(dname, kind))
            yield f"{dname}|query={kind}|query_variant={knob}", _entry(flat), (off.tobytes(), idx.tobytes())


# The golden file names every distinct [kernel, flags] pair once ("entries") and gives each case the index of its pair: ray cases in
# groups "dtype|output|variant=v" of one index per tuning combination in _knob_suffixes() order, every other case under its own key.
def _knob_suffixes():
    return [f"|items={items}|guide={guide}|rec8={rec8}|coherent={int(coherent)}"
            for items, guide, rec8, coherent in itertools.product(ITEMS, GUIDE, REC8, COHERENT)]


def _group_keys(group):
    return [group + sfx for sfx in _knob_suffixes()] if "|variant=" in group else [group]


def unpack_golden(packed):
    table = {}
    for group, indices in packed["cases"].items():
        keys = _group_keys(group)
        assert len(keys) == len(indices), group
        for key, i in zip(keys, indices):
            table[key] = packed["entries"][i]
    return table


def pack_golden(table):
    entries = sorted({(k, f) for k, f in table.values()})
    cases = {}
    for key in table:
        cases.setdefault(key.split("|items=")[0], [])
    for group, indices in cases.items():
        indices.extend(entries.index(tuple(table[key])) for key in _group_keys(group))
    return {"entries": [list(e) for e in entries], "cases": cases}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return unpack_golden(json.load(f))


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("dname", list(DTYPES))
def test_walk_dispatch_rays(golden, dname, output):
    eng = _engine()
    want = _reference(eng, dname, output)
    seen = 0
    for key, entry, res in ray_cases(eng, dname, output):
        assert entry == golden[key], (key, entry, golden[key])
        assert res == want, key
        seen += 1
    assert seen == len(VARIANTS) * len(ITEMS) * len(GUIDE) * len(REC8) * len(COHERENT)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_walk_dispatch_ordered(golden, dname):
    eng = _engine()
    seen = 0
    for key, entry in ordered_cases(eng, dname):
        assert entry == golden[key], (key, entry, golden[key])
        seen += 1
    assert seen == len(ORDERED_OUTPUTS) * len(ORDERS)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_walk_dispatch_queries(golden, dname):
    eng = _engine()
    binary = {}
    seen = 0
    for key, entry, res in query_cases(eng, dname):
        assert entry == golden[key], (key, entry, golden[key])
        kind = key.split("|")[1]
        assert res == binary.setdefault(kind, res), key    # (QUERY_VARIANT = 0 comes first: the binary walk's lists)
        seen += 1
    assert seen == len(QUERY_KINDS) * len(QUERY_VARIANTS)


def test_walk_dispatch_golden_is_complete(golden):
    """the golden file holds exactly the cases above: none left out, none stale"""
    keys = set()
    for dname in DTYPES:
        for output, variant, items, guide, rec8, coherent in itertools.product(OUTPUTS, VARIANTS, ITEMS, GUIDE, REC8, COHERENT):
            vname = "default" if variant is None else str(variant)
            keys.add(f"{dname}|{output}|variant={vname}|items={items}|guide={guide}|rec8={rec8}|coherent={int(coherent)}")
        keys.update(f"{dname}|{output}|order={order}" for output, order in itertools.product(ORDERED_OUTPUTS, ORDERS))
        keys.update(f"{dname}|query={kind}|query_variant={knob}" for kind, knob in itertools.product(QUERY_KINDS, QUERY_VARIANTS))
    assert keys == set(golden)


if __name__ == "__main__":   # the recorder: run on the commit whose dispatch is to be pinned
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bvh_amd
    table = {}
    for dn in DTYPES:
        for out in OUTPUTS:
            for k, e, _ in ray_cases(bvh_amd, dn, out):
                table[k] = e
        for k, e in ordered_cases(bvh_amd, dn):
            table[k] = e
        for k, e, _ in query_cases(bvh_amd, dn):
            table[k] = e
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    packed = pack_golden(table)
    assert unpack_golden(packed) == table
    with open(path, "w") as f:   # one line per entry and per group
        f.write('{"entries": [\n' + ",\n".join(json.dumps(e) for e in packed["entries"]) + '\n],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(g)}: {json.dumps(i)}" for g, i in sorted(packed["cases"].items())) + "\n}}\n")
    print(f"{len(table)} cases -> {path}; kernels: {len({e[0] for e in table.values()})}")
