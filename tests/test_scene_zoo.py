"""The scene zoo (tests/zoo.py) through every variant of the path, bit for bit against the CPU oracle, which
tests/test_oracle_zoo.py pins on the same scenes.  Every operation on the path is a min, a max, a compare, an integer
operation or one correctly rounded IEEE operation, so there is no tolerance: a kernel that flushes a subnormal in one of its
union forms, contracts c - r into something else, divides in the wrong precision or screens with a rounded box differs in
a code, a box or a pair on one of these scenes.

Sizes: 300 = 2 chunks, 5 packets (the last ragged), one sort tile; 4099 = 17 chunks with crossing nodes, 5 tiles (the gather
finish with a 3-code last tile), 65 packets (the last with 3 leaves); 132 000 = 516 chunks (k_cross's long-range unions; the
root takes the whole-workgroup union)."""
import ctypes

import numpy as np
import pytest

from collision_amd._lib import cdll
from tests.test_batch_collide import _check, _concat, _limit, _reference, _run
from tests.test_pipeline_parity import check_against_oracle
from tests.util import assert_same_pair_set, packed_pairs
from tests.zoo import DTYPES, FAMILIES, cached_scene

pytestmark = pytest.mark.gpu

MARK = 0x80000000                       # COL_LINK_MARK (csrc/col_common.h)
CHUNKED_ROOM = 512 * 8192 + 1000        # room for the chunked allocation's holes: the list comes from the chunked walk itself
# name: (sort_plan, traverse_plan, col_debug_traverse, col_debug_lbvh, col_debug_leaf_blocks)
VARIANTS = {
    "lsd_exact": ("lsd", "exact", 0, 0, 3.0),
    "lsd_chunked": ("lsd", "chunked", 0, 0, 3.0),
    "msd_exact": ("msd", "exact", 0, 0, 3.0),
    "msd_chunked": ("msd", "chunked", 0, 0, 3.0),
    "dynamic_order": ("msd", "exact", 32768, 4096, 3.0),      # dynamic packet order, longest walks first
    "chunk_wide": ("msd", "exact", 0, 1024, 3.0),             # k_chunk_wide
    "group_tables": ("msd", "exact", 0, 32768, 3.0),          # k_group's tables instead of the direct unions
    "no_marks": ("msd", "exact", 0, 0, 0.0),                  # no leaf blocks
    "all_marks": ("msd", "exact", 0, 0, 1e30),                # every node of <= 16 leaves a leaf block
}


def _run_variant(oracle, hip_env, coords, radii, variant, **kw):
    sort_plan, traverse_plan, traverse, lbvh, k = VARIANTS[variant]
    lib = cdll()
    lib.col_debug_leaf_blocks.argtypes = [ctypes.c_float]
    assert lib.col_debug_traverse(traverse) == 0 and lib.col_debug_lbvh(lbvh) == 0
    lib.col_debug_leaf_blocks(ctypes.c_float(k))
    try:
        return check_against_oracle(oracle, hip_env, coords, radii, sort_plan=sort_plan, traverse_plan=traverse_plan,
                                    extra_capacity=CHUNKED_ROOM if traverse_plan == "chunked" else 0, **kw)
    finally:
        lib.col_debug_traverse(0)
        lib.col_debug_lbvh(0)
        lib.col_debug_leaf_blocks(ctypes.c_float(3.0))


# ---------------------------------------------------------------- a. the path's variants on every family
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_variant_matches_the_oracle(oracle, hip_env, family, dtype, n, variant):
    coords, radii = cached_scene(family, n, dtype)
    _, _, count, _ = _run_variant(oracle, hip_env, coords, radii, variant)
    assert n / 2 <= count <= 16 * n


# ---------------------------------------------------------------- b. the instance of k_chunk that writes the Node array
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_the_nodes_writing_instance(oracle, hip_env, family, dtype):
    """check_against_oracle reads Collider._nodes_buf AFTER the call: the path ran with nodes = NULL and the Node words it
    compares are col_bvh_build's.  With the array asked for BEFORE the call, k_chunk's Node-writing instance produces
    what is compared -- and the same `bounds`, links and marks included, as the instance without."""
    coords, radii = cached_scene(family, 4099, dtype)
    _, with_nodes, count, pairs = check_against_oracle(oracle, hip_env, coords, radii, prepare=lambda c: c._nodes_buf)
    _, without, count2, pairs2 = check_against_oracle(oracle, hip_env, coords, radii)
    assert with_nodes["bounds"].tobytes() == without["bounds"].tobytes()
    assert count == count2
    assert_same_pair_set(pairs, pairs2)


# ---------------------------------------------------------------- c. k_cross's long-range unions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["tiny", "huge", "log_radii", "offset"])
def test_516_chunks(oracle, hip_env, family, dtype):
    coords, radii = cached_scene(family, 132000, dtype)
    _, _, count, _ = check_against_oracle(oracle, hip_env, coords, radii, group_size=256, ngroups=16)
    assert count > 132000


# ---------------------------------------------------------------- d. exact scaling on the device
def _leaf_spans(nodes, n):
    """(first leaf, last leaf) of every internal node."""
    hi = nodes["right_edge"][:n - 1].astype(np.int64)
    cur = nodes["data"][:n - 1, 0].astype(np.int64)
    while (cur < n - 1).any():
        inner = cur < n - 1
        cur[inner] = nodes["data"][cur[inner], 0]
    return cur - (n - 1), hi


_unscaled = {}


def _log_radii_run(oracle, hip_env, dtype):
    """The unscaled run of log_radii at 4099, once per dtype, read-only."""
    if dtype not in _unscaled:
        coords, radii = cached_scene("log_radii", 4099, dtype)
        _, st, count, pairs = check_against_oracle(oracle, hip_env, coords, radii)
        for a in list(st.values()) + [pairs]:
            a.setflags(write=False)
        _unscaled[dtype] = (st, count, pairs)
    return _unscaled[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_log_radii_has_marked_and_unmarked_small_nodes(oracle, hip_env, dtype):
    n = 4099
    st, _, _ = _log_radii_run(oracle, hip_env, dtype)
    bits = np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64
    down = st["bounds"].view(bits)[:n - 1, 1, 3].astype(np.uint64)
    marked = (down & np.uint64(MARK)) != 0
    lo, hi = _leaf_spans(st["nodes"], n)
    small = hi - lo < 16
    assert (marked & small).any() and (~marked & small).any() and not (marked & ~small).any()
    np.testing.assert_array_equal(down[marked], (np.uint64(MARK) | (lo[marked].astype(np.uint64) << np.uint64(4))
                                                 | (hi[marked] - lo[marked]).astype(np.uint64)))


@pytest.mark.parametrize("k", [-60, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_power_of_two_scaling_on_the_device(oracle, hip_env, dtype, k):
    """The leaf-block criterion compares a node's width with k x its first leaf's: invariant under exact scaling.  So the
    scaled run's links and marks (lane w) are the unscaled run's bits, its boxes exactly 2^k x, everything else the same:
    the marks of a heavy-tailed scene are pinned without a reference for them."""
    n = 4099
    st, count, pairs = _log_radii_run(oracle, hip_env, dtype)
    coords, radii = cached_scene("log_radii", n, dtype)
    f = np.asarray(2.0 ** k, dtype)
    sc, sr = coords * f, radii * f
    assert (sc / f == coords).all() and (sr / f == radii).all()             # exact
    _, st2, count2, pairs2 = check_against_oracle(oracle, hip_env, sc, sr)
    bits = np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64
    np.testing.assert_array_equal(st2["bounds"].view(bits)[:, :, 3], st["bounds"].view(bits)[:, :, 3])
    np.testing.assert_array_equal(st2["bounds"][:, :, :3].view(bits), (st["bounds"][:, :, :3] * f).view(bits))
    np.testing.assert_array_equal(st2["codes"], st["codes"])
    np.testing.assert_array_equal(st2["ids"], st["ids"])
    assert count2 == count
    assert_same_pair_set(pairs2, pairs)


# ---------------------------------------------------------------- e. col_collide_batch
_batches = {}


def _zoo_batch(oracle, dt, sizes):
    """Every family at every size of `sizes`, shuffled, an empty scene in between; with its reference; read-only."""
    key = (dt, tuple(sizes))
    if key not in _batches:
        scenes = [cached_scene(family, n, dt) for family in FAMILIES for n in sizes]
        np.random.RandomState(7).shuffle(scenes)
        scenes.insert(len(scenes) // 2, (np.empty((0, 3), dt), np.empty(0, dt)))
        coords, radii, offsets = _concat(scenes, np.dtype(dt))
        for a in (coords, radii, offsets):
            a.setflags(write=False)
        top = max(sizes)
        _batches[key] = (coords, radii, offsets, _reference(oracle, coords, radii, offsets, capacity_per_scene=top * (top - 1) // 2))
    return _batches[key]


def _same_results(a, b):
    np.testing.assert_array_equal(a["codes"], b["codes"])
    np.testing.assert_array_equal(a["ids"], b["ids"])
    np.testing.assert_array_equal(a["counts"], b["counts"])
    np.testing.assert_array_equal(packed_pairs(a["pairs"]), packed_pairs(b["pairs"]))


@pytest.mark.parametrize("dt", DTYPES)
def test_batch_of_every_family(hip_env, oracle, dt):
    """64, 300 and the limit: with max_scene at the limit every scene runs in the 1024-thread instance, one scene per
    workgroup, which stages 4096 hits: aniso at the limit has more (the second walk), every other scene fewer."""
    ctx, cq = hip_env
    limit = _limit(dt)
    sizes = [64, 300, min(1024, limit)]
    coords, radii, offsets, ref = _zoo_batch(oracle, dt, sizes)
    n = np.diff(offsets.astype(np.int64))
    counts = np.array([r["count"] for r in ref])
    assert (counts > 4 * n).any() and (counts[n > 0] < 4 * n[n > 0]).any()
    assert (counts[n == sizes[2]] > 4 * limit).any() and (counts[n == sizes[2]] < 4 * limit).any()
    capacity = int(counts.sum()) + 5
    first = None
    for max_scene in (int(n.max()), limit):
        res = _run(ctx, cq, coords, radii, offsets, max_scene, capacity)
        _check(res, ref, offsets)
        first = first or res
        _same_results(res, first)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", [[64], [64, 300]])
def test_batch_in_the_smaller_instances(hip_env, oracle, dt, sizes):
    """The same scenes where the batch's largest scene lets the smaller instances run: eight scenes per workgroup in the
    one-wave class (64), two in the 512 class (300); and what they give is what the 1024-thread instance gives."""
    ctx, cq = hip_env
    coords, radii, offsets, ref = _zoo_batch(oracle, dt, sizes)
    capacity = sum(r["count"] for r in ref) + 5
    own = _run(ctx, cq, coords, radii, offsets, max(sizes), capacity)
    _check(own, ref, offsets)
    top = _run(ctx, cq, coords, radii, offsets, _limit(dt), capacity)
    _check(top, ref, offsets)
    _same_results(own, top)
