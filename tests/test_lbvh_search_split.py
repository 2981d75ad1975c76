"""The production k_chunk (csrc/lbvh.hip) runs Karras' search for the nodes that cross a chunk boundary in search workgroups
of its own launch -- a wave per chunk -- while the chunk workgroups end behind the climb; every word of `nodes`, `bounds` and
other_end[] has exactly one writer.  col_lbvh on constructed sorted codes: the production kernel against k_chunk_wide
(col_debug_lbvh bit 1024: the search inside the chunk's workgroup, for every node) byte for byte -- links and marks
included, on buffers prefilled with 0xFF bytes so that a word nobody wrote cannot pass as a link -- and against the oracle;
without `nodes` the same `bounds`; and with the count on the device (col_collide_plan_dev under a bound) the arrays and the
pair set of the exact-n call."""
import ctypes as C
import functools

import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call, cdll
from collision_amd.collision import Collider, Node
from tests.test_cross_direct_unions import _codes
from tests.test_nodes_optional import _crossing_per_chunk, _two_chains
from tests.util import assert_same_pair_set, download, pad4, upload

pytestmark = pytest.mark.gpu

WIDE = 1024                 # col_debug_lbvh: k_chunk_wide at every size
# the root is the only crossing node; either side of two full chunks; ranges that end at the search window's +-256 edge and
# one leaf beyond it; a range longer than one thread of k_cross reads; far probes across groups of 256 chunks
SIZES = [257, 511, 512, 513, 769, 1025, 256 * 11 + 1, 256 * 257 + 3]
KINDS = ["uniform", "equal", "runs", "forty"]
F64_SIZES = SIZES[:3] + SIZES[-1:]
NULL_NODES = [("uniform", 513), ("equal", 513), ("runs", 513), ("forty", 513)] + [(k, 256 * 11 + 1) for k in KINDS] + [("two_chains", 700)]


@functools.lru_cache(maxsize=None)
def _inputs(kind, n):
    rs = np.random.RandomState(n % 100003 + len(kind))
    codes = _two_chains(n) if kind == "two_chains" else _codes(kind, n, rs)
    ids = rs.permutation(n).astype(np.uint32)
    coords = rs.uniform(-1, 1, size=(n, 3))
    radii = rs.uniform(0.001, 0.05, size=n)
    return codes, ids, coords, radii


@functools.lru_cache(maxsize=None)
def _reference(kind, n, dt):
    import oracle
    oracle.build()
    codes, ids, coords, radii = _inputs(kind, n)
    nodes = oracle.build_bvh(codes, ids)
    return nodes, oracle.node_bounds(pad4(coords.astype(dt)), radii.astype(dt), nodes)


def _lbvh(ctx, cq, bufs, n, dt, mode, with_nodes=True):
    """col_lbvh into buffers prefilled with 0xFF bytes (bounds, nodes, scratch)."""
    cb, nn = np.dtype(dt).itemsize, 2 * n - 1
    codes_buf, ids_buf, coords_buf, radii_buf = bufs
    nodes = upload(ctx, np.full(nn * Node.itemsize, 0xFF, np.uint8)) if with_nodes else None
    bounds = upload(ctx, np.full(nn * 8 * cb, 0xFF, np.uint8))
    scratch = upload(ctx, np.full(call.col_lbvh_scratch_bytes(n, cb), 0xFF, np.uint8))
    cdll().col_debug_lbvh(mode)
    try:
        call.col_lbvh(cq.stream, codes_buf.ptr, ids_buf.ptr, coords_buf.ptr, radii_buf.ptr, nodes.ptr if with_nodes else None,
                      bounds.ptr, scratch.ptr, n, cb)
        cq.finish()
    finally:
        cdll().col_debug_lbvh(0)
    return download(cq, nodes, Node, nn) if with_nodes else None, download(cq, bounds, dt, (nn, 2, 4))


def _upload_inputs(ctx, kind, n, dt):
    codes, ids, coords, radii = _inputs(kind, n)
    return tuple(upload(ctx, a) for a in (codes, ids, pad4(coords.astype(dt)), radii.astype(dt)))


def _check(hip_env, kind, n, dt):
    ctx, cq = hip_env
    bufs = _upload_inputs(ctx, kind, n, dt)
    nodes_p, bounds_p = _lbvh(ctx, cq, bufs, n, dt, 0)
    nodes_w, bounds_w = _lbvh(ctx, cq, bufs, n, dt, WIDE)
    ref_nodes, ref_bounds = _reference(kind, n, dt)
    bits = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    np.testing.assert_array_equal(bounds_p.view(bits)[:, :, :3], ref_bounds.view(bits)[:, :, :3])
    np.testing.assert_array_equal(nodes_p["right_edge"], ref_nodes["right_edge"])
    np.testing.assert_array_equal(nodes_p["parent"][1:], ref_nodes["parent"][1:])
    np.testing.assert_array_equal(nodes_p["data"][:n - 1], ref_nodes["data"][:n - 1])
    links_w, links_p = bounds_w.view(bits)[:, :, 3], bounds_p.view(bits)[:, :, 3]
    print("production vs wide-index, %s n = %d %s: skip links differ at %d nodes, down links / marks at %d, node words at %d"
          % (kind, n, dt, int((links_w[:, 0] != links_p[:, 0]).sum()), int((links_w[:, 1] != links_p[:, 1]).sum()),
             int((nodes_w.view(np.uint32) != nodes_p.view(np.uint32)).sum())))
    assert bounds_p.tobytes() == bounds_w.tobytes()             # links and marks included
    assert nodes_p.tobytes() == nodes_w.tobytes()
    return nodes_p, bounds_p


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_search_split_f32(hip_env, kind, n):
    _check(hip_env, kind, n, "float32")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", F64_SIZES)
def test_search_split_f64(hip_env, kind, n):
    _check(hip_env, kind, n, "float64")


FIRST_MAX_CHUNKS = 1500000 // 256        # SEARCH_FIRST_MAX_CHUNKS: up to here all search workgroups come first, above in groups of 40


@pytest.mark.parametrize("chunks", [FIRST_MAX_CHUNKS, FIRST_MAX_CHUNKS + 1])
def test_search_split_either_side_of_the_layout_threshold(hip_env, chunks):
    _check(hip_env, "uniform", 256 * chunks - 5, "float32")


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_search_split_full_crossing_list(hip_env, dt):
    """_two_chains(700): chunk 1 has ~60 crossing nodes, more than its list holds and more than one round of the searcher."""
    nodes_p, _ = _check(hip_env, "two_chains", 700, dt)
    assert _crossing_per_chunk(nodes_p, 700).max() >= 32


@pytest.mark.parametrize("kind,n", NULL_NODES)
def test_search_split_without_nodes(hip_env, kind, n):
    ctx, cq = hip_env
    bufs = _upload_inputs(ctx, kind, n, "float32")
    _, bounds_a = _lbvh(ctx, cq, bufs, n, "float32", 0, with_nodes=True)
    _, bounds_b = _lbvh(ctx, cq, bufs, n, "float32", 0, with_nodes=False)
    ref_nodes, ref_bounds = _reference(kind, n, "float32")
    np.testing.assert_array_equal(bounds_b.view(np.uint32)[:, :, :3], ref_bounds.view(np.uint32)[:, :, :3])
    assert bounds_a.tobytes() == bounds_b.tobytes()


def _plan_dev(ctx, cq, rows, rad, n, bound, plan, gs=256):
    """col_collide_plan_dev with n real spheres under `bound` (bound == n: the exact-n call)."""
    dt = rows.dtype
    cb = dt.itemsize
    col = Collider(ctx, bound, 16, gs, dt.name)
    col._allocate()
    rb, qb = upload(ctx, rows[:bound]), upload(ctx, rad[:bound])
    cap = 1 << 16
    nb, pb, word = hip.Buffer(ctx, 4), hip.Buffer(ctx, cap * 8), upload(ctx, np.array([n, n], np.uint32))
    partials, parts = hip.Buffer(ctx, 256 * 8 * cb), C.c_uint32(0)
    guard = upload(ctx, np.full(8 * bound + 1024, 0xA5A5A5A5, np.uint32))      # passed nowhere
    call.col_minmax4_stage1_dev(cq.stream, rb.ptr, word.ptr, bound, cb, partials.ptr, C.byref(parts))
    call.col_collide_plan_dev(cq.stream, rb.ptr, qb.ptr, bound, col.padded_size, cb, col._codes_bufs[0].ptr, col._codes_bufs[1].ptr,
                              col._ids_bufs[0].ptr, col._ids_bufs[1].ptr, col._nodes_buf.ptr, col._bounds_buf.ptr, None,
                              col._alloc["scratch"].ptr, nb.ptr, pb.ptr, cap, plan, None, partials.ptr, parts.value, word.ptr)
    cq.finish()
    count = int(download(cq, nb, np.uint32, 1)[0])
    assert count <= cap
    return dict(codes=download(cq, col._codes_bufs[1], np.uint32, col.padded_size)[:n],
                ids=download(cq, col._ids_bufs[1], np.uint32, col.padded_size)[:n],
                bounds=download(cq, col._bounds_buf, dt, (2 * bound - 1, 2, 4))[:2 * n - 1],
                pairs=download(cq, pb, np.uint32, (count, 2)), guard=download(cq, guard, np.uint32, 8 * bound + 1024))


@pytest.mark.parametrize("plan", [0, 1])
def test_device_side_count_under_a_bound(hip_env, plan):
    """1000 real spheres under a bound of 1600: the grid holds chunk and search workgroups for seven chunks, four are real."""
    ctx, cq = hip_env
    n, bound = 1000, 1600
    rs = np.random.RandomState(1000)
    rows = np.full((bound, 4), 7.0, np.float32)                 # rows beyond the count: never read as spheres
    rows[:n, :3] = rs.random_sample((n, 3))
    rad = np.full(bound, 3.0, np.float32)
    rad[:n] = 0.5 * n ** (-1.0 / 3.0)
    got = _plan_dev(ctx, cq, rows, rad, n, bound, plan)
    want = _plan_dev(ctx, cq, rows, rad, n, n, plan)
    np.testing.assert_array_equal(got["codes"], want["codes"])
    np.testing.assert_array_equal(got["ids"], want["ids"])
    assert got["bounds"].tobytes() == want["bounds"].tobytes()
    assert len(want["pairs"]) > 0
    assert_same_pair_set(got["pairs"], want["pairs"])
    assert (got["guard"] == 0xA5A5A5A5).all() and (want["guard"] == 0xA5A5A5A5).all()
