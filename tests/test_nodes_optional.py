"""`nodes` is optional on the collide path (csrc/lbvh.hip: the k_chunk instance without the Node stores): with a NULL
pointer the boxes, links and leaf-block marks in `bounds`, the sorted codes and ids, the pair count and the pair set are the
bits a call with the array gives; nothing is written behind the caller's back; and Collider._nodes_buf, filled on its first
access from the sorted codes and ids of the last call, is byte for byte the array the tree build writes itself."""
import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call, cdll
from collision_amd.collision import NO_NODE, Collider, Node
from collision_amd.misc import roundUp
from tests.util import assert_same_pair_set, download, pad4, run_collider, upload

pytestmark = pytest.mark.gpu

GS = 64
MARK = 0x80000000                        # COL_LINK_MARK (csrc/col_common.h): a leaf block in an internal node's down link
FF = np.uint32(0xFFFFFFFF)
# one chunk of 256 leaves and its edges, two chunks and a leaf, three chunks, a few
SIZES = [2, 3, 255, 256, 257, 513, 1000]
SCENES = [("uniform", n) for n in SIZES] + [("equal", 600), ("dense", 1000)]


def _scene(kind, n, dt):
    rs = np.random.RandomState(n + len(kind))
    if kind == "equal":                  # one point 600 times: all codes equal, the tree is balanced by position
        return np.full((n, 3), 0.25, dt), np.full(n, 0.01, dt)
    coords = rs.random_sample((n, 3)).astype(dt)
    if kind == "dense":                  # leaf boxes wider than the spacing: small nodes are marked as leaf blocks
        return coords, np.full(n, 0.06, dt)
    return coords, (rs.uniform(0.2, 0.6, size=n) * n ** (-1.0 / 3.0)).astype(dt)


def _collide(ctx, cq, coords, radii, with_nodes, capacity):
    """col_collide_plan (LSD plan) on fresh buffers; nodes prefilled with 0xFFFFFFFF or not passed at all."""
    dt = coords.dtype
    n, cb = len(coords), coords.dtype.itemsize
    padded = roundUp(n, 2 * GS)
    nn = 2 * n - 1
    cbuf, rbuf = upload(ctx, pad4(coords)), upload(ctx, radii)
    codes = [upload(ctx, np.zeros(padded, np.uint32)) for _ in range(2)]
    ids = [upload(ctx, np.zeros(padded, np.uint32)) for _ in range(2)]
    nodes = upload(ctx, np.full(4 * nn, FF, np.uint32)) if with_nodes else None
    bounds = upload(ctx, np.zeros((nn, 2, 4), dt))
    scratch = hip.Buffer(ctx, call.col_collide_scratch_bytes(n, padded, cb))
    counter, pairs = upload(ctx, np.zeros(1, np.uint32)), hip.Buffer(ctx, capacity * 8)
    guard = upload(ctx, np.full(4 * nn + 1024, 0xA5A5A5A5, np.uint32))       # passed nowhere
    call.col_collide_plan(cq.stream, cbuf.ptr, rbuf.ptr, n, padded, cb, codes[0].ptr, codes[1].ptr, ids[0].ptr, ids[1].ptr,
                          nodes.ptr if with_nodes else None, bounds.ptr, None, scratch.ptr, counter.ptr, pairs.ptr, capacity,
                          0, None)
    cq.finish()
    count = int(download(cq, counter, np.uint32, 1)[0])
    assert count <= capacity
    return dict(codes=download(cq, codes[1], np.uint32, padded), ids=download(cq, ids[1], np.uint32, padded),
                bounds=download(cq, bounds, dt, (nn, 2, 4)), count=count, pairs=download(cq, pairs, np.uint32, (count, 2)),
                nodes=download(cq, nodes, Node, nn) if with_nodes else None,
                guard=download(cq, guard, np.uint32, 4 * nn + 1024))


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("kind,n", SCENES)
def test_null_nodes_changes_no_other_output(hip_env, kind, n, dt):
    ctx, cq = hip_env
    coords, radii = _scene(kind, n, np.dtype(dt))
    cap = n * (n - 1) // 2 if kind == "equal" else 64 * n
    a = _collide(ctx, cq, coords, radii, True, cap)
    b = _collide(ctx, cq, coords, radii, False, cap)
    assert a["bounds"].tobytes() == b["bounds"].tobytes()           # boxes, skip and down links, leaf-block marks
    np.testing.assert_array_equal(a["codes"], b["codes"])
    np.testing.assert_array_equal(a["ids"], b["ids"])
    assert a["count"] == b["count"]
    assert_same_pair_set(b["pairs"], a["pairs"])
    assert (b["guard"] == 0xA5A5A5A5).all() and (a["guard"] == 0xA5A5A5A5).all()
    # the scenes are what they are here for
    bits = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    down = a["bounds"].view(bits)[:n - 1, 1, 3].astype(np.uint64)
    if kind == "equal":
        assert (a["codes"][:n] == a["codes"][0]).all() and a["count"] == n * (n - 1) // 2
    if kind == "dense":
        assert (down & np.uint64(MARK)).any()
    if kind == "uniform" and n >= 255:
        assert a["count"] > 0
    # and the array, where asked for, leaves the root's parent and a leaf's second word alone
    assert a["nodes"]["parent"][0] == NO_NODE and (a["nodes"]["data"][n - 1:, 1] == NO_NODE).all()


def _two_chains(n):
    """Sorted codes whose tree has two chains that all end inside leaves 256..511: nodes 300..328 cover [0, k] and nodes
    329..357 cover [k, n - 1], so chunk 1 has ~60 nodes that cross a chunk boundary -- more than its list of CROSS_CAP - 1 = 31
    holds: k_cross then goes through ALL 256 nodes of the chunk and tells the crossing ones by their other_end[] words."""
    top = 0x3FFFFFFF
    up = [1 << j for j in range(29)]
    down = [top - (1 << j) for j in range(28, -1, -1)]
    codes = np.array([0] * 300 + up + down + [top] * (n - 300 - 58), np.uint32)
    assert (np.diff(codes.astype(np.int64)) >= 0).all()
    return codes


def _crossing_per_chunk(nodes, n):
    hi = nodes["right_edge"][:n - 1].astype(np.int64)
    cur = nodes["data"][:n - 1, 0].astype(np.int64)                # first leaf: follow the left children
    while (cur < n - 1).any():
        inner = cur < n - 1
        cur[inner] = nodes["data"][cur[inner], 0]
    lo = cur - (n - 1)
    cross = (lo // 256) != (hi // 256)
    return np.bincount(np.arange(n - 1)[cross] // 256, minlength=(n + 255) // 256)


WIDE = 1024                              # col_debug_lbvh: k_chunk_wide (n >= 2^30) at every size


@pytest.mark.parametrize("mode", [0, WIDE])
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("n", [700, 256 * 11 + 1])
def test_null_nodes_in_a_chunk_with_a_full_crossing_list(hip_env, oracle, n, dt, mode):
    """The instance without Node stores writes other_end[] for crossing nodes only -- except in a chunk whose crossing list
    is full, where k_cross asks for the word of every node.  Scratch prefilled with zeros: a word that was left out would
    read as "my other end is leaf 0", a range that crosses, and the node's finished box would be overwritten.  Also with
    k_chunk_wide, which drops the Node stores alone."""
    ctx, cq = hip_env
    rs = np.random.RandomState(n)
    codes, ids = _two_chains(n), rs.permutation(n).astype(np.uint32)
    coords = pad4(rs.uniform(-1, 1, size=(n, 3)).astype(dt))
    radii = rs.uniform(0.001, 0.05, size=n).astype(dt)
    cb, nn = np.dtype(dt).itemsize, 2 * n - 1
    bufs = [upload(ctx, a) for a in (codes, ids, coords, radii)]
    out = []
    for with_nodes in (True, False):
        nodes = upload(ctx, np.full(4 * nn, FF, np.uint32)) if with_nodes else None
        bounds = upload(ctx, np.zeros((nn, 2, 4), dt))
        scratch = upload(ctx, np.zeros(call.col_lbvh_scratch_bytes(n, cb), np.uint8))
        cdll().col_debug_lbvh(mode)
        try:
            call.col_lbvh(cq.stream, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, nodes.ptr if with_nodes else None,
                          bounds.ptr, scratch.ptr, n, cb)
            cq.finish()
        finally:
            cdll().col_debug_lbvh(0)
        out.append((download(cq, nodes, Node, nn) if with_nodes else None, download(cq, bounds, dt, (nn, 2, 4))))
    (nodes_a, bounds_a), (_, bounds_b) = out
    assert _crossing_per_chunk(nodes_a, n).max() >= 32               # the list of chunk 1 is full
    ref_nodes = oracle.build_bvh(codes, ids)
    ref_bounds = oracle.node_bounds(coords, radii, ref_nodes)
    bits = np.uint32 if cb == 4 else np.uint64
    np.testing.assert_array_equal(bounds_b.view(bits)[:, :, :3], ref_bounds.view(bits)[:, :, :3])
    assert bounds_a.tobytes() == bounds_b.tobytes()


def _fill_ff(cq, buf):
    hip.enqueue_fill_buffer(cq, buf, FF, 0, buf.size)
    cq.finish()


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("kind,n", [("uniform", 2), ("uniform", 257), ("uniform", 1000), ("equal", 600)])
def test_collider_nodes_on_first_access_then_kept(hip_env, oracle, kind, n, dt):
    ctx, cq = hip_env
    coords, radii = _scene(kind, n, np.dtype(dt))
    cap = n * (n - 1) // 2 if kind == "equal" else 64 * n
    col = Collider(ctx, n, 8, GS, dt)
    count, pairs = run_collider(ctx, cq, col, coords, radii, cap)
    assert "nodes" not in col._alloc and col._nodes_ptr is None     # no array, no pointer
    buf = col._nodes_buf                                             # allocates, fills for the call above, keeps from now on
    assert col._nodes_ptr == buf.ptr and buf.size == (2 * n - 1) * Node.itemsize
    first = download(cq, buf, Node, 2 * n - 1)
    _fill_ff(cq, buf)
    col._fill_nodes()                                                # the same fill on a known prefill
    lazy = download(cq, buf, Node, 2 * n - 1)
    _fill_ff(cq, buf)
    count2, pairs2 = run_collider(ctx, cq, col, coords, radii, cap)  # keep mode: the tree build writes the array
    assert col._nodes_buf is buf
    direct = download(cq, buf, Node, 2 * n - 1)
    assert lazy.tobytes() == direct.tobytes()                        # every byte, the unwritten ones included
    assert direct["parent"][0] == NO_NODE and (direct["data"][n - 1:, 1] == NO_NODE).all()
    written = direct.view(np.uint32) != FF
    np.testing.assert_array_equal(first.view(np.uint32)[written], direct.view(np.uint32)[written])
    assert count2 == count
    assert_same_pair_set(pairs2, pairs)
    # a larger size after the access: a new array, written by the call itself
    m = 2 * n + 301
    coords, radii = _scene("uniform", m, np.dtype(dt))
    col.resize(size=m)
    ref = oracle.collide(oracle.pad4(coords), radii, padded=col.padded_size, capacity=64 * m)
    count3, pairs3 = run_collider(ctx, cq, col, coords, radii, 64 * m)
    assert col._nodes_ptr == col._nodes_buf.ptr and col._nodes_buf.size == (2 * m - 1) * Node.itemsize
    nodes = download(cq, col._nodes_buf, Node, 2 * m - 1)
    np.testing.assert_array_equal(nodes["right_edge"], ref["nodes"]["right_edge"])
    np.testing.assert_array_equal(nodes["parent"][1:], ref["nodes"]["parent"][1:])
    np.testing.assert_array_equal(nodes["data"][:m - 1], ref["nodes"]["data"][:m - 1])
    np.testing.assert_array_equal(nodes["data"][m - 1:, 0], ref["nodes"]["data"][m - 1:, 0])
    assert count3 == ref["count"]
    assert_same_pair_set(pairs3, ref["pairs"])


def test_first_access_before_any_call_only_allocates(hip_env):
    ctx, cq = hip_env
    col = Collider(ctx, 300, 8, GS, "float32")
    assert col._nodes_buf.size == 599 * Node.itemsize and col._nodes_ptr == col._nodes_buf.ptr
