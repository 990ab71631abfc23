"""Closest-hit and any-hit ray queries against the shapes' own boxes (bvhgpu_traverse_box_*), pinned on the oracle alone.

Definition: L_i is FlatBvh::traverse's list for ray i, (enter_s, exit_s) is Ray::intersection_slice_for_aabb on shape s's AABB; s is a
candidate iff enter_s < tmax[i] (strict, in T; tmax None = +inf).  closest: the candidate with the smallest enter, the first of L_i on equal
entries.  first: the first candidate of L_i.  No candidate: {+inf, 0} and NONE.  box_match below is that definition on a CSR with t-slices;
tests/test_gpu_box_hit.py compares the GPU against it byte for byte."""
import numpy as np
import pytest

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


def box_match(off, idx, ts, tmax, first):
    """the definition on a CSR (offsets, indices, tslice[total,2]) → (slice[n,2], shape[n])"""
    n = len(off) - 1
    counts = np.diff(off.astype(np.int64))
    t = np.full(n, np.inf, dtype=ts.dtype) if tmax is None else np.asarray(tmax, dtype=ts.dtype)
    total = len(ts)
    starts = off[:-1].astype(np.int64)
    rows = counts > 0
    with np.errstate(invalid="ignore"):
        ok = ts[:, 0] < np.repeat(t, counts)                              # strict, in T: NaN admits nothing
    if not first and total:                                               # closest: of the candidates, those with the row's smallest entry
        masked = np.where(ok, ts[:, 0], np.inf).astype(ts.dtype)
        rowmin = np.full(n, np.inf, dtype=ts.dtype)
        rowmin[rows] = np.minimum.reduceat(masked, starts[rows])
        ok = ok & (ts[:, 0] == np.repeat(rowmin, counts))
    pos = np.where(ok, np.arange(total), total)                           # ... and of those, the first of the list
    win = np.full(n, total, dtype=np.int64)
    if total:
        win[rows] = np.minimum.reduceat(pos, starts[rows])
    found = win < total
    out = np.zeros((n, 2), dtype=ts.dtype)
    out[:, 0] = np.inf
    out[found] = ts[win[found]]
    shape = np.full(n, NONE, dtype=np.uint32)
    shape[found] = idx[win[found]]
    return out, shape


# two proper boxes and an inverted one (min > max on x), a ray from the origin along +x: the inner node over shapes {0, 2} has x in [3.5, 3.6]
# and is entered at 3.5, the inverted box below it at 3 — a node's entry is no lower bound for the shapes below it
THREE_BOXES = np.array([[3.5, -1, -1, 3.6, 1, 1], [4, -1, -1, 6, 1, 1], [5, -1, -1, 3, 1, 1]], dtype=np.float64)


def three_box_scene(orc, dtype, shift=(0.0, 0.0, 0.0)):
    """(aabbs, one ray) of the scene above, moved by `shift`"""
    s = np.asarray(shift, dtype=np.float64)
    aabbs = (THREE_BOXES + np.concatenate([s, s])).astype(dtype)
    rays = orc.make_rays(s[None, :].astype(dtype), np.array([[1.0, 0.0, 0.0]], dtype=dtype), dtype)
    return aabbs, rays


def _csr(orc, aabbs, rays):
    oflat = orc.flatten(orc.build(aabbs).nodes)
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True)
    return off, idx, ts


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_boxes_with_an_inverted_one(orc, dtype):
    aabbs, rays = three_box_scene(orc, dtype)
    off, idx, ts = _csr(orc, aabbs, rays)
    assert idx.tolist() == [0, 2, 1] and ts[:, 0].tolist() == [3.5, 3.0, 4.0]
    for first, tmax, shape, sl in ((False, None, 2, (3.0, 5.0)), (True, None, 0, (3.5, dtype(3.6))),
                                   (False, 3.25, 2, (3.0, 5.0)), (True, 3.25, 2, (3.0, 5.0)),
                                   (False, 3.0, NONE, (np.inf, 0.0)), (True, 3.0, NONE, (np.inf, 0.0))):
        got = box_match(off, idx, ts, None if tmax is None else np.array([tmax], dtype), first)
        assert got[1].tolist() == [shape], (first, tmax, got)
        assert got[0].tobytes() == np.array([sl], dtype).tobytes(), (first, tmax, got)
    # the inner node over {0, 2} is entered later than the inverted box below it
    oflat = orc.flatten(orc.build(aabbs).nodes)
    leaf = int(np.nonzero((oflat["entry"] == NONE) & (oflat["shape"] == 2))[0][0])
    above = [i for i in range(leaf) if oflat["entry"][i] != NONE and oflat["exit"][i] > leaf]
    enters = [orc.ray_slice(rays[0], np.concatenate([oflat["min"][i], oflat["max"][i]]))[0] for i in above]
    assert max(enters) == 3.5 > ts[1, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_equal_entries_the_first_of_the_list_wins(orc, dtype):
    aabbs = np.array([[1, -1, -1, 2, 1, 1], [1, -2, -2, 3, 2, 2], [5, -1, -1, 6, 1, 1]], dtype=dtype)
    rays = orc.make_rays(np.zeros((1, 3), dtype), np.array([[1.0, 0.0, 0.0]], dtype), dtype)
    off, idx, ts = _csr(orc, aabbs, rays)
    assert sorted(idx.tolist()) == [0, 1, 2]
    tied = np.nonzero(ts[:, 0] == 1.0)[0]
    assert len(tied) == 2
    for first in (False, True):
        sl, shape = box_match(off, idx, ts, None, first)
        if first:
            assert shape[0] == idx[0]
        else:
            assert shape[0] == idx[tied[0]] and sl.tobytes() == ts[tied[0]][None, :].tobytes()
    # a tmax between the tie and the far box changes nothing; at the tie it admits neither of the two
    assert box_match(off, idx, ts, np.array([2.0], dtype), False)[1][0] == idx[tied[0]]
    assert box_match(off, idx, ts, np.array([1.0], dtype), False)[1][0] == NONE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_origin_inside_a_box_enters_at_plus_zero(orc, dtype):
    aabbs = np.array([[-1, -1, -1, 1, 1, 1], [4, -1, -1, 6, 1, 1]], dtype=dtype)
    rays = orc.make_rays(np.zeros((1, 3), dtype), np.array([[1.0, 0.25, -0.5]], dtype), dtype)
    off, idx, ts = _csr(orc, aabbs, rays)
    for first in (False, True):
        sl, shape = box_match(off, idx, ts, None, first)
        assert shape[0] == 0 and sl[0, 0] == 0 and not np.signbit(sl[0, 0])
        assert sl[:, 0].tobytes() == np.zeros(1, dtype).tobytes()        # +0: the sign bit is clear
        sl, shape = box_match(off, idx, ts, np.zeros(1, dtype), first)   # tmax = 0 admits nothing, not even an entry of 0
        assert shape[0] == NONE and sl.tobytes() == np.array([[np.inf, 0]], dtype).tobytes()


def test_the_python_surface_exists():
    from bvh_amd import api
    for name in ("closest_box_hits", "first_box_hits", "box_occluded"):
        assert callable(getattr(api._TreeBase, name, None)), name
    assert callable(getattr(api._Hits, "fetch_box", None))
    from bvh_amd import _lib
    assert _lib.TRAVERSE_FIRST == 1024
    assert {"bvhgpu_traverse_box_f32", "bvhgpu_traverse_box_f64", "bvhgpu_hits_fetch_box"} <= {name for name, _, _ in _lib.SYMBOLS}
