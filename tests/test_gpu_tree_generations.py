"""Every batch entry of the Python API as the FIRST reader of a new tree generation.

Since the lazy flatten (BVHGPU_TUNE_FLATTEN_LAZY, default 1) a build, rebuild, refit or flatten writes what the wide walk reads; the FlatNode
array, the folded binary array and the binary LDS slot table are owed until something reads them, and each host function that reads one
has to call ensure_flat_arrays first (with mode 2 that call also joins the side stream).  A reader that forgot would answer from the
generation before — so here the generation before is ANOTHER scene (tests/test_tree_generations_cpu.py proves on the CPU that every
expectation tells them apart), and every row of its reader table runs on a fresh tree

  after each transition away from scene A      a  rebuild(B, flatten=True)        b  rebuild(B), flatten()
                                               c  rebuild_async(B in HBM), no wait: the reader is the call that settles the build
                                               d  refit(A')                       e  rebuild(C, flatten=True), rebuild(D, flatten=True)
  in each position                             primed, first:      A had materialised everything, the reader is the first call on the new tree
                                               unprimed, first:    A was never read, its lazy parts are still owed when the transition comes
                                               primed, after wide: a wide CSR batch, which materialises nothing, ran on the new tree first
  under each flatten mode                      (FLATTEN_LAZY, FLATTEN_INLINE) = (1,1) (0,1) (2,1) (3,1) (1,0)

and must give the reference of the NEW generation byte for byte; afterwards flat.nodes is the oracle's flatten of the new tree.  Triangles
and spheres are the caller's to refresh.  Also: a rebuild to another shape count drops the sphere array as it drops the triangles, and a
failed asynchronous rebuild reaches whichever entry is called first."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_refit import _device, _rb
from test_tree_generations_cpu import DTYPES, READER_IDS, READERS, gen, inputs, same_all, want

pytestmark = pytest.mark.gpu

MODES = [(1, 1), (0, 1), (2, 1), (3, 1), (1, 0)]               # (BVHGPU_TUNE_FLATTEN_LAZY, BVHGPU_TUNE_FLATTEN_INLINE)
TARGET = dict(a="B", b="B", c="B", d="A1", e="D")              # the generation each transition leaves on the tree
POSITIONS = ("primed, first", "unprimed, first", "primed, after wide")
WIDE = READERS[READER_IDS.index("csr_wide")]
CSR_T = READERS[READER_IDS.index("csr_t")]


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


def _inputs(eng, dtype):
    I = inputs(dtype)
    return SimpleNamespace(**vars(I), rb=_rb(eng, I.rays))


def _context(lazy=None, inline=None):
    from bvh_amd import Context
    from bvh_amd._lib import TUNE_FLATTEN_INLINE, TUNE_FLATTEN_LAZY
    ctx = Context(0)
    if lazy is not None:
        ctx.set_tuning(TUNE_FLATTEN_LAZY, lazy)
        ctx.set_tuning(TUNE_FLATTEN_INLINE, inline)
    return ctx


def _hand_over(T, G):
    """the caller's per-shape arrays of generation G"""
    T.flat.set_triangles(G.tris)
    T.flat.set_spheres(G.spheres)


def _tree_on_a(eng, ctx, a):
    """a fresh tree holding generation A, flattened (lazily) and never read"""
    bvh = eng.Bvh.from_aabbs(a.aabbs, ctx)
    T = SimpleNamespace(bvh=bvh, flat=bvh.flatten(), ctx=ctx)
    _hand_over(T, a)
    return T


def _prime(T, I, a):
    """generation A materialises everything: the FlatNode array, and the binary array with its slot table through a t-slice walk"""
    assert T.flat.nodes.tobytes() == a.flat.tobytes()
    assert same_all(CSR_T.call(T, I), want(CSR_T, "A", a.dtype))


def _transition(T, kind, G, dev):
    if kind == "a":
        T.bvh.rebuild(G.aabbs, flatten=True)
    elif kind == "b":
        T.bvh.rebuild(G.aabbs)
        T.flat = T.bvh.flatten()
    elif kind == "c":
        _hand_over(T, G)                       # (same shape count: handed over before the build is enqueued, so that nothing but the reader looks at the tree)
        T.bvh.rebuild_async(dev)
        return
    elif kind == "d":
        T.bvh.refit(G.aabbs)
    else:
        c = gen("C", G.dtype)
        T.bvh.rebuild(c.aabbs, flatten=True)
        T.bvh.rebuild(G.aabbs, flatten=True)
    _hand_over(T, G)


@pytest.mark.parametrize("lazy,inline", MODES, ids=[f"lazy{m[0]}-inline{m[1]}" for m in MODES])
@pytest.mark.parametrize("transition", list("abcde"))
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_every_reader_first_on_a_new_generation(eng, dtype, transition, lazy, inline):
    ctx = _context(lazy, inline)
    I = _inputs(eng, dtype)
    a, g = gen("A", dtype), gen(TARGET[transition], dtype)
    dev = _device(g.aabbs) if transition == "c" else None
    for reader in READERS:
        expected = want(reader, g.name, dtype)
        for position in POSITIONS:
            label = (reader.name, position)
            T = _tree_on_a(eng, ctx, a)
            if not position.startswith("unprimed"):
                _prime(T, I, a)
            _transition(T, transition, g, dev)
            if position.endswith("after wide"):
                assert same_all(WIDE.call(T, I), want(WIDE, g.name, dtype)), label
            assert same_all(reader.call(T, I), expected), label
            assert T.flat.nodes.tobytes() == g.flat.tobytes(), label
            T.bvh.close()
    ctx.close()


def _refused(reader, T, I):
    from bvh_amd._lib import INVALID_ARG, BvhGpuError
    with pytest.raises(BvhGpuError) as e:
        reader.call(T, I)
    assert e.value.status == INVALID_ARG, (reader.name, str(e.value))
    return str(e.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_rebuild_to_another_shape_count_drops_spheres_and_triangles(eng, dtype):
    """one triangle and one sphere per shape: after a rebuild from 1500 to 2300 shapes both arrays are too short.  Every entry that reads one
    is refused until the caller hands the new one over; entries that read the boxes alone answer for the new tree throughout."""
    ctx = _context()
    I = _inputs(eng, dtype)
    a, d = gen("A", dtype), gen("D", dtype)
    T = _tree_on_a(eng, ctx, a)
    for r in READERS:                                       # both arrays are in use before the rebuild
        if r.needs:
            assert same_all(r.call(T, I), want(r, "A", dtype)), r.name
    T.bvh.rebuild(d.aabbs, flatten=True)
    have = set()
    for step in (None, "spheres", "triangles"):
        if step == "spheres":
            T.flat.set_spheres(d.spheres)
        elif step == "triangles":
            T.flat.set_triangles(d.tris)
        have.add(step)
        for r in READERS:
            if r.needs in have:
                assert same_all(r.call(T, I), want(r, "D", dtype)), (r.name, step)
            else:
                assert ("sphere" if r.needs == "spheres" else "triangle") in _refused(r, T, I), (r.name, step)
    assert {r.needs for r in READERS} == {None, "spheres", "triangles"}
    T.bvh.close()
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_failed_async_rebuild_reaches_whichever_entry_comes_first(eng, dtype):
    """rebuild_async of boxes with one NaN, input in HBM, no wait: the first call on the tree — each reader in turn, on a tree of its own —
    returns the settle's refusal instead of a result; after the next rebuild the same reader gives the reference."""
    ctx = _context()
    I = _inputs(eng, dtype)
    a, b = gen("A", dtype), gen("B", dtype)
    bad = b.aabbs.copy()
    bad[77, 3] = np.nan
    dev = _device(bad)
    for reader in READERS:
        T = _tree_on_a(eng, ctx, a)
        _hand_over(T, b)
        T.bvh.rebuild_async(dev)
        _refused(reader, T, I)
        T.bvh.rebuild(b.aabbs, flatten=True)
        assert same_all(reader.call(T, I), want(reader, "B", dtype)), reader.name
        assert T.flat.nodes.tobytes() == b.flat.tobytes(), reader.name
        T.bvh.close()
    ctx.close()
