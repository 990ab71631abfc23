"""Every module-level batch entry of the Python API (tests/test_module_entries_cpu.py MODULE_READERS: bvh_amd.region_batch, classified,
plain on a Bvh, count-only, planes in HBM) as the FIRST reader of a new tree generation — tests/test_gpu_tree_generations.py's test, with
its scenes, transitions, positions and flatten modes, over the rows that file's class enumeration cannot see:

  after each transition away from scene A      a  rebuild(B, flatten=True)        b  rebuild(B), flatten()
                                               c  rebuild_async(B in HBM), no wait: the reader is the call that settles the build
                                               d  refit(A')                       e  rebuild(C, flatten=True), rebuild(D, flatten=True)
  in each position                             primed, first / unprimed, first / primed, after wide
  under each flatten mode                      (FLATTEN_LAZY, FLATTEN_INLINE) = (1,1) (0,1) (2,1) (3,1) (1,0); with LAZY = 2 the entry's
                                               ensure_flat_arrays is the join with the side stream

and must give region_ref.walk over the ORACLE's tree of the new generation byte for byte (for the refit: the oracle's refit of A's tree).
region.hip reads the folded array (ensure_flat_arrays) and builds its ancestor table per batch, so nothing of A may survive.  Also: a failed
asynchronous rebuild reaches region_batch when it is the first call."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_refit import _device
from test_gpu_tree_generations import MODES, POSITIONS, TARGET, WIDE, _context, _inputs, _prime, _refused, _transition, _tree_on_a
from test_module_entries_cpu import MODULE_READERS, planes, want
from test_tree_generations_cpu import DTYPES, gen, same_all
from test_tree_generations_cpu import want as tree_want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


def _with_planes(eng, dtype):
    import torch
    I = _inputs(eng, dtype)
    p = np.ascontiguousarray(planes(dtype))
    return SimpleNamespace(**vars(I), planes=p, planes_dev=torch.from_numpy(p.copy()).cuda())


@pytest.mark.parametrize("lazy,inline", MODES, ids=[f"lazy{m[0]}-inline{m[1]}" for m in MODES])
@pytest.mark.parametrize("transition", list("abcde"))
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_every_module_reader_first_on_a_new_generation(eng, dtype, transition, lazy, inline):
    ctx = _context(lazy, inline)
    I = _with_planes(eng, dtype)
    a, g = gen("A", dtype), gen(TARGET[transition], dtype)
    dev = _device(g.aabbs) if transition == "c" else None
    for reader in MODULE_READERS:
        expected = want(reader, g.name, dtype)
        for position in POSITIONS:
            label = (reader.name, position)
            T = _tree_on_a(eng, ctx, a)
            if not position.startswith("unprimed"):
                _prime(T, I, a)
            _transition(T, transition, g, dev)
            if position.endswith("after wide"):
                assert same_all(WIDE.call(T, I), tree_want(WIDE, g.name, dtype)), label
            assert same_all(reader.call(T, I), expected), label
            assert T.flat.nodes.tobytes() == g.flat.tobytes(), label
            T.bvh.close()
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_failed_async_rebuild_reaches_a_module_reader_that_comes_first(eng, dtype):
    """rebuild_async of boxes with one NaN, input in HBM, no wait: region_batch as the first call on the tree returns the settle's refusal
    instead of rows; after the next rebuild the same reader gives the reference"""
    ctx = _context()
    I = _with_planes(eng, dtype)
    a, b = gen("A", dtype), gen("B", dtype)
    bad = b.aabbs.copy()
    bad[77, 3] = np.nan
    dev = _device(bad)
    for reader in MODULE_READERS:
        T = _tree_on_a(eng, ctx, a)
        T.bvh.rebuild_async(dev)
        _refused(reader, T, I)
        T.bvh.rebuild(b.aabbs, flatten=True)
        assert same_all(reader.call(T, I), want(reader, "B", dtype)), reader.name
        assert T.flat.nodes.tobytes() == b.flat.tobytes(), reader.name
        T.bvh.close()
    ctx.close()
