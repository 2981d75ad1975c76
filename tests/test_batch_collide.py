"""col_collide_batch / BatchCollider (csrc/batch.hip): B independent scenes, concatenated, in one call.  Every scene must get
exactly what the oracle gives for that scene alone -- sorted codes, sorted local ids, pair count and the oriented pair set.
All scenes sit in the same unit cube, so a leak between scenes shows up as extra pairs.

Scenes as in tests/test_nodes_optional.py: coords U[0,1)^3, radii U(0.2, 0.6) * n^(-1/3): about 2 pairs per sphere, so a
list capacity of 64 x total never truncates (the degenerate scenes get the capacity they need)."""
import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call, cdll
from collision_amd.collision import BatchCollider, Collider
from tests.util import assert_same_pair_set, download, pad4, packed_pairs, run_collider, upload

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
SKIPPED = 0xFFFFFFFF
PREFILL = 0xA5A5A5A5
GUARD = 0x5EED5EED
MIXED = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1024]


def _limit(dt):
    return int(call.col_collide_batch_max_scene(np.dtype(dt).itemsize))


def _scene(rs, n, dt):
    coords = rs.random_sample((n, 3)).astype(dt)
    radii = (rs.uniform(0.2, 0.6, size=n) * max(n, 1) ** (-1.0 / 3.0)).astype(dt)
    return coords, radii


def _concat(scenes, dt):
    sizes = [len(c) for c, _ in scenes]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    coords = np.concatenate([c for c, _ in scenes] + [np.empty((0, 3), dt)]).astype(dt)
    radii = np.concatenate([r for _, r in scenes] + [np.empty(0, dt)]).astype(dt)
    return coords, radii, offsets


def _random_batch(sizes, dt, seed):
    rs = np.random.RandomState(seed)
    return _concat([_scene(rs, n, dt) for n in sizes], dt)


def _reference(oracle, coords, radii, offsets, capacity_per_scene=None):
    """The checker, scene by scene: oracle.collide(pad4(scene), radii)."""
    out = []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        n = b - a
        if n <= 0:                       # an empty scene: nothing to ask the oracle
            out.append(dict(count=0, pairs=np.empty((0, 2), np.uint32), codes=np.empty(0, np.uint32), ids=np.empty(0, np.uint32)))
            continue
        cap = 64 * n if capacity_per_scene is None else capacity_per_scene
        ref = oracle.collide(oracle.pad4(coords[a:b]), radii[a:b], capacity=cap)
        assert ref["count"] <= cap
        out.append(ref)
    return out


def _run(ctx, cq, coords, radii, offsets, max_scene, capacity, total=None, bufs=None, sorted_out=True):
    """col_collide_batch on prefilled outputs.  `capacity` None: count-only mode (pairs = NULL)."""
    dt = coords.dtype
    total = len(coords) if total is None else total
    nsc = len(offsets) - 1
    if bufs is None:
        bufs = dict(coords=upload(ctx, pad4(coords)) if len(coords) else hip.Buffer(ctx, 64), radii=upload(ctx, radii) if len(radii) else hip.Buffer(ctx, 64),
                    offsets=upload(ctx, offsets))
    cap = 0 if capacity is None else capacity
    words = max(len(coords), 1)
    out = dict(codes=upload(ctx, np.full(words, PREFILL, np.uint32)), ids=upload(ctx, np.full(words, PREFILL, np.uint32)),
               counter=upload(ctx, np.full(1, PREFILL, np.uint32)), counts=upload(ctx, np.full(max(nsc, 1), PREFILL, np.uint32)),
               pairs=upload(ctx, np.full(2 * cap + 2, GUARD, np.uint32)))
    scratch_bytes = call.col_collide_batch_scratch_bytes(nsc, total, max_scene, dt.itemsize)
    scratch = hip.Buffer(ctx, scratch_bytes) if scratch_bytes else None
    args = lambda: (cq.stream, bufs["coords"].ptr, bufs["radii"].ptr, bufs["offsets"].ptr, nsc, total, max_scene, dt.itemsize,
                    out["codes"].ptr if sorted_out else None, out["ids"].ptr if sorted_out else None,
                    scratch.ptr if scratch else None, out["counter"].ptr, out["counts"].ptr,
                    None if capacity is None else out["pairs"].ptr, cap)
    call.col_collide_batch(*args())
    cq.finish()

    def read():
        counter = int(download(cq, out["counter"], np.uint32, 1)[0])
        raw = download(cq, out["pairs"], np.uint32, 2 * cap + 2)
        return dict(counter=counter, counts=download(cq, out["counts"], np.uint32, max(nsc, 1))[:nsc],
                    codes=download(cq, out["codes"], np.uint32, words), ids=download(cq, out["ids"], np.uint32, words),
                    pairs=raw[:2 * min(counter, cap)].reshape(-1, 2), rest=raw[2 * min(counter, cap):])
    res = read()
    res.update(bufs=bufs, out=out, again=lambda: (call.col_collide_batch(*args()), cq.finish(), read())[2])
    return res


def _check(res, ref, offsets, skipped=(), sorted_out=True):
    """Every scene against its reference; pairs only if the list was not truncated."""
    offsets = offsets.astype(np.int64)
    nsc = len(offsets) - 1
    want_counts = np.array([SKIPPED if s in skipped else ref[s]["count"] for s in range(nsc)], np.uint32)
    np.testing.assert_array_equal(res["counts"], want_counts)
    total = int(sum(ref[s]["count"] for s in range(nsc) if s not in skipped))
    assert res["counter"] == total
    pairs = res["pairs"].astype(np.int64)
    assert len(pairs) == total                                   # (callers pass a capacity that holds everything)
    owner = np.searchsorted(offsets[1:], pairs[:, 0], side="right") if nsc and not skipped else None
    for s in range(nsc):
        a, b = offsets[s], offsets[s + 1]
        if s in skipped:
            if sorted_out and b > a:
                assert (res["codes"][a:b] == PREFILL).all() and (res["ids"][a:b] == PREFILL).all()
            continue
        if sorted_out:
            np.testing.assert_array_equal(res["codes"][a:b], ref[s]["codes"])
            np.testing.assert_array_equal(res["ids"][a:b], ref[s]["ids"])
        mine = pairs[owner == s] if owner is not None else pairs[(pairs[:, 0] >= a) & (pairs[:, 0] < b)]
        assert ((mine[:, 1] >= a) & (mine[:, 1] < b)).all()      # both indices of a row lie in one scene
        assert_same_pair_set(mine - a, ref[s]["pairs"])
    assert (res["rest"] == GUARD).all()


_cache = {}


def _mixed(oracle, dt):
    """The mixed batch and its reference, computed once per dtype and never changed."""
    if dt not in _cache:
        sizes = [n for n in MIXED if n <= _limit(dt)]
        np.random.RandomState(7).shuffle(sizes)
        coords, radii, offsets = _random_batch(sizes, np.dtype(dt), 11)
        for a in (coords, radii, offsets):
            a.setflags(write=False)
        _cache[dt] = (coords, radii, offsets, _reference(oracle, coords, radii, offsets))
    return _cache[dt]


@pytest.mark.parametrize("dt", DTYPES)
def test_mixed_batch(hip_env, oracle, dt):
    ctx, cq = hip_env
    coords, radii, offsets, ref = _mixed(oracle, dt)
    res = _run(ctx, cq, coords, radii, offsets, _limit(dt), 64 * len(coords))
    _check(res, ref, offsets)
    assert res["counter"] > len(coords)                          # the scenes are what they are here for


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("top", [64, 256])
def test_instance_choice_changes_nothing(hip_env, oracle, dt, top):
    ctx, cq = hip_env
    sizes = {64: [64, 1, 40, 63, 0, 17, 64, 2, 33, 5, 64, 50], 256: [256, 65, 3, 200, 0, 255, 64, 129, 256]}[top]
    coords, radii, offsets = _random_batch(sizes, np.dtype(dt), top)
    ref = _reference(oracle, coords, radii, offsets)
    first = None
    for max_scene in (top, top + 1, 256, _limit(dt)) if top == 64 else (top, top + 1, _limit(dt)):
        res = _run(ctx, cq, coords, radii, offsets, max_scene, 64 * len(coords))
        _check(res, ref, offsets)
        if first is None:
            first = res
        np.testing.assert_array_equal(res["codes"], first["codes"])
        np.testing.assert_array_equal(res["ids"], first["ids"])
        np.testing.assert_array_equal(res["counts"], first["counts"])
        np.testing.assert_array_equal(packed_pairs(res["pairs"]), packed_pairs(first["pairs"]))


@pytest.mark.parametrize("dt", DTYPES)
def test_many_scenes(hip_env, oracle, dt):
    """More workgroups than CUs, several scenes per workgroup in the small class, a last workgroup that is not full."""
    ctx, cq = hip_env
    sizes = np.random.RandomState(3).randint(1, 41, size=3000).tolist()
    coords, radii, offsets = _random_batch(sizes, np.dtype(dt), 5)
    ref = _reference(oracle, coords, radii, offsets)
    res = _run(ctx, cq, coords, radii, offsets, 40, 64 * len(coords), sorted_out=False)
    _check(res, ref, offsets, sorted_out=False)
    assert (res["codes"] == PREFILL).all() and (res["ids"] == PREFILL).all()      # NULL codes_out / ids_out: nothing written


@pytest.mark.parametrize("dt", DTYPES)
def test_degenerate_scenes(hip_env, oracle, dt):
    ctx, cq = hip_env
    dt = np.dtype(dt)
    rs = np.random.RandomState(21)
    same = (np.full((70, 3), 0.25, dt), np.full(70, 0.01, dt))                # one point 70 times
    flat = _scene(rs, 200, dt)
    flat[0][:, 2] = 0.5                                                       # z constant: a degenerate axis
    dup = _scene(rs, 300, dt)
    dup[0][17] = dup[0][170]                                                  # two exact duplicates
    dup[1][17] = dup[1][170]
    line = _scene(rs, 64, dt)
    line[0][:, 0] = 0.125                                                     # two degenerate axes, in the small class's size
    line[0][:, 1] = 0.75
    coords, radii, offsets = _concat([same, flat, _scene(rs, 100, dt), dup, line], dt)
    ref = _reference(oracle, coords, radii, offsets, capacity_per_scene=300 * 299 // 2)
    assert ref[0]["count"] == 2415 and (ref[0]["codes"] == 0).all()
    np.testing.assert_array_equal(ref[0]["ids"], np.arange(70))
    res = _run(ctx, cq, coords, radii, offsets, 300, 64 * len(coords))
    _check(res, ref, offsets)
    assert res["counts"][0] == 2415
    # two of them alone, in the smallest class that holds each (70 spheres: 256; 64 spheres: the one-wave class)
    for s in (0, 4):
        a, b = int(offsets[s]), int(offsets[s + 1])
        one = np.array([0, b - a], np.uint32)
        res = _run(ctx, cq, coords[a:b], radii[a:b], one, b - a, 4096)
        _check(res, [ref[s]], one)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,scenes", [(64, 9), (200, 5), (400, 3), (700, 2)])
def test_dense_scenes(hip_env, oracle, dt, n, scenes):
    """Far more pairs per sphere than a workgroup stages (every size class): the pairs come from the second walk, with the
    list space of every thread taken from the scan of the hit counts.  Also with a list that ends inside a thread's rows."""
    ctx, cq = hip_env
    dt = np.dtype(dt)
    rs = np.random.RandomState(n)
    coords, radii, offsets = _concat([(rs.random_sample((n, 3)).astype(dt), np.full(n, 0.25, dt)) for _ in range(scenes)], dt)
    ref = _reference(oracle, coords, radii, offsets, capacity_per_scene=n * (n - 1) // 2)
    total = sum(r["count"] for r in ref)
    assert min(r["count"] for r in ref) > 8 * n
    res = _run(ctx, cq, coords, radii, offsets, n, total + 5)
    _check(res, ref, offsets)
    cut = _run(ctx, cq, coords, radii, offsets, n, total // 3)
    assert cut["counter"] == total and len(cut["pairs"]) == total // 3
    np.testing.assert_array_equal(cut["counts"], res["counts"])
    got = packed_pairs(cut["pairs"])
    assert (np.diff(got) != 0).all() and np.isin(got, packed_pairs(res["pairs"])).all() and (cut["rest"] == GUARD).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_capacity(hip_env, oracle, dt):
    ctx, cq = hip_env
    coords, radii, offsets, ref = _mixed(oracle, dt)
    full = _run(ctx, cq, coords, radii, offsets, _limit(dt), 64 * len(coords))
    total = full["counter"]
    cap = total // 2
    res = _run(ctx, cq, coords, radii, offsets, _limit(dt), cap)
    assert res["counter"] == total
    np.testing.assert_array_equal(res["counts"], full["counts"])
    assert len(res["pairs"]) == cap
    got, everything = packed_pairs(res["pairs"]), packed_pairs(full["pairs"])
    assert (np.diff(got) != 0).all() and np.isin(got, everything).all()       # distinct members of the full set
    assert (res["rest"] == GUARD).all()                                       # the guard words behind the list
    count_only = _run(ctx, cq, coords, radii, offsets, _limit(dt), None)
    assert count_only["counter"] == total
    np.testing.assert_array_equal(count_only["counts"], full["counts"])
    assert (count_only["rest"] == GUARD).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_skipped_scene(hip_env, oracle, dt):
    ctx, cq = hip_env
    sizes = [100, 257, 256, 0, 31]
    coords, radii, offsets = _random_batch(sizes, np.dtype(dt), 9)
    ref = _reference(oracle, coords, radii, offsets)
    res = _run(ctx, cq, coords, radii, offsets, 256, 64 * len(coords))
    _check(res, ref, offsets, skipped={1})
    assert res["counts"][1] == SKIPPED and res["counter"] == sum(r["count"] for i, r in enumerate(ref) if i != 1)
    # a non-monotone pair of offsets: scene 1 runs backwards (skipped), scene 2 is what lies between the swapped ends
    bad = offsets.copy()
    bad[1], bad[2] = offsets[2], offsets[1]
    ref_bad = _reference(oracle, coords, radii, bad)
    assert int(bad[1]) - int(bad[0]) == 357 and int(bad[3]) - int(bad[2]) == 513
    res = _run(ctx, cq, coords, radii, bad, 1024, 64 * len(coords), sorted_out=False)
    want = np.array([ref_bad[0]["count"], SKIPPED, ref_bad[2]["count"], 0, ref_bad[4]["count"]], np.uint32)
    np.testing.assert_array_equal(res["counts"], want)
    assert res["counter"] == int(want[[0, 2, 4]].sum())
    # (scenes 0 and 2 now share rows 100..356, so the list is compared as a whole: every scene's pairs, nothing else)
    expect = np.concatenate([ref_bad[s]["pairs"].astype(np.int64) + int(bad[s]) for s in (0, 2, 4)])
    np.testing.assert_array_equal(packed_pairs(res["pairs"]), packed_pairs(expect))
    assert (res["rest"] == GUARD).all()
    # ... and a scene whose end lies beyond `total` (the last one, with total cut short)
    res = _run(ctx, cq, coords, radii, offsets, 1024, 64 * len(coords), total=len(coords) - 1)
    _check(res, ref, offsets, skipped={4})


@pytest.mark.parametrize("dt", DTYPES)
def test_reuse_and_isolation(hip_env, oracle, dt):
    ctx, cq = hip_env
    coords, radii, offsets, ref = _mixed(oracle, dt)
    guard = upload(ctx, np.full(4096, PREFILL, np.uint32))                    # passed nowhere
    res = _run(ctx, cq, coords, radii, offsets, _limit(dt), 64 * len(coords))
    _check(res, ref, offsets)
    again = res["again"]()                                                    # same buffers: counter and counts are re-zeroed by the call
    _check(again, ref, offsets)
    bufs = res["bufs"]
    assert download(cq, bufs["coords"], coords.dtype, (len(coords), 4)).tobytes() == pad4(coords).tobytes()
    assert download(cq, bufs["radii"], radii.dtype, len(radii)).tobytes() == radii.tobytes()
    assert download(cq, bufs["offsets"], np.uint32, len(offsets)).tobytes() == offsets.tobytes()
    assert (download(cq, guard, np.uint32, 4096) == PREFILL).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_against_the_single_scene_path(hip_env, dt):
    ctx, cq = hip_env
    sizes = [65, 300, 1000]
    if _limit(dt) < 1000:
        sizes[2] = _limit(dt)
    coords, radii, offsets = _random_batch(sizes, np.dtype(dt), 13)
    res = _run(ctx, cq, coords, radii, offsets, max(sizes), 64 * len(coords))
    for s, n in enumerate(sizes):
        a, b = int(offsets[s]), int(offsets[s + 1])
        count, pairs = run_collider(ctx, cq, Collider(ctx, n, 8, 64, dt), coords[a:b], radii[a:b], 64 * n)
        assert res["counts"][s] == count and count <= 64 * n
        mine = res["pairs"].astype(np.int64)
        mine = mine[(mine[:, 0] >= a) & (mine[:, 0] < b)] - a
        assert_same_pair_set(mine, pairs)


@pytest.mark.parametrize("dt", DTYPES)
def test_batch_collider_end_to_end(hip_env, oracle, dt):
    ctx, cq = hip_env
    coords, radii, offsets, ref = _mixed(oracle, dt)
    total, nsc = len(coords), len(offsets) - 1

    def run(col, coords, radii, offsets, wait=False):
        cap = 64 * len(coords)
        cbuf, rbuf, obuf = upload(ctx, pad4(coords)), upload(ctx, radii), upload(ctx, offsets)
        n_buf, counts_buf = hip.Buffer(ctx, 4), hip.Buffer(ctx, 4 * (len(offsets) - 1))
        pairs_buf = upload(ctx, np.full(2 * cap + 2, GUARD, np.uint32))
        other = hip.CommandQueue(ctx)                                         # an event of another queue to wait for
        e0 = hip.enqueue_fill_buffer(other, n_buf, np.uint32(PREFILL), 0, 4) if wait else None
        e = col.get_collisions(cq, cbuf, rbuf, obuf, n_buf, counts_buf, pairs_buf, cap, wait_for=[e0] if wait else None)
        counter = int(download(cq, n_buf, np.uint32, 1, wait_for=[e])[0])
        raw = download(cq, pairs_buf, np.uint32, 2 * cap + 2)
        words = len(coords)
        return dict(counter=counter, counts=download(cq, counts_buf, np.uint32, len(offsets) - 1),
                    pairs=raw[:2 * counter].reshape(-1, 2), rest=raw[2 * counter:],
                    codes=download(cq, col._codes_buf, np.uint32, words) if col._codes_buf else None,
                    ids=download(cq, col._ids_buf, np.uint32, words) if col._ids_buf else None)

    col = BatchCollider(ctx, total, nsc, _limit(dt), dt)
    assert col._codes_buf is None and col._ids_buf is None
    _check(run(col, coords, radii, offsets, wait=True), ref, offsets, sorted_out=False)
    count_only = hip.Buffer(ctx, 4), hip.Buffer(ctx, 4 * nsc)
    e = col.get_collisions(cq, upload(ctx, pad4(coords)), upload(ctx, radii), upload(ctx, offsets), count_only[0], count_only[1], None, 0)
    assert int(download(cq, count_only[0], np.uint32, 1, wait_for=[e])[0]) == sum(r["count"] for r in ref)
    # a larger batch after resize: the mixed batch twice
    coords2, radii2 = np.concatenate([coords, coords]), np.concatenate([radii, radii])
    offsets2 = np.concatenate([offsets, offsets[1:] + offsets[-1]]).astype(np.uint32)
    col.resize(total_size=2 * total, n_scenes=2 * nsc)
    _check(run(col, coords2, radii2, offsets2), ref + ref, offsets2, sorted_out=False)
    # keep_sorted: the sorted codes and local ids of every scene
    kept = BatchCollider(ctx, total, nsc, _limit(dt), dt, keep_sorted=True)
    assert kept._codes_buf.size == 4 * total and kept._ids_buf.size == 4 * total
    _check(run(kept, coords, radii, offsets), ref, offsets)
    kept.resize(total_size=2 * total, n_scenes=2 * nsc)
    assert kept._codes_buf.size == 8 * total
    _check(run(kept, coords2, radii2, offsets2), ref + ref, offsets2)
