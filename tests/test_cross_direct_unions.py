"""k_cross's direct unions (csrc/lbvh.hip): up to COL_MSD_MAX_N / 256 chunks the boxes of the nodes that cross a chunk
boundary are unions over the chunk totals themselves, without k_group's tables.  col_lbvh on sorted codes must give the
oracle's boxes and node records bit for bit, and the same bytes as the table path (col_debug_lbvh bit 32768)."""
import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call, cdll
from collision_amd.collision import NO_NODE, Node
from tests.util import download, pad4, upload

pytestmark = pytest.mark.gpu

K = 8                       # CROSS_SHORT: ranges of up to K whole chunks are read by one thread, longer ones by a wave
TABLES = 32768              # col_debug_lbvh: the table path at every size
MAX_DIRECT_CHUNKS = 4050000 // 256       # COL_MSD_MAX_N / 256
SIZES = [257, 256 * (K + 2) + 1, 256 * (K + 3) + 1, 256 * 257 + 3, 256 * 600]
KINDS = ["uniform", "equal", "runs", "forty"]


def _codes(kind, n, rs):
    if kind == "uniform":
        return np.sort(rs.randint(0, 1 << 30, size=n).astype(np.uint32))
    if kind == "equal":                 # the tree is balanced by position
        return np.full(n, 12345, np.uint32)
    if kind == "runs":                  # 2^k - 1 in runs: a chain-like top
        vals = ((1 << np.arange(31, dtype=np.uint64)) - 1).astype(np.uint32)
        return np.sort(vals[rs.randint(0, 31, size=n)])
    return np.sort((rs.randint(0, 40, size=n) * 26843545).astype(np.uint32))        # 40 values: dense chunks


def _lbvh(ctx, cq, bufs, n, dt, mode):
    cb = np.dtype(dt).itemsize
    codes_buf, ids_buf, coords_buf, radii_buf = bufs
    nn = 2 * n - 1
    nodes = upload(ctx, np.full(nn, NO_NODE, np.uint32).repeat(4))
    bounds = upload(ctx, np.zeros((nn, 2, 4), dt))
    scratch = hip.Buffer(ctx, call.col_lbvh_scratch_bytes(n, cb))
    cdll().col_debug_lbvh(mode)
    try:
        call.col_lbvh(cq.stream, codes_buf.ptr, ids_buf.ptr, coords_buf.ptr, radii_buf.ptr, nodes.ptr, bounds.ptr,
                      scratch.ptr, n, cb)
        cq.finish()
    finally:
        cdll().col_debug_lbvh(0)
    return download(cq, nodes, Node, nn), download(cq, bounds, dt, (nn, 2, 4))


def _check(hip_env, oracle, kind, n, dt):
    ctx, cq = hip_env
    rs = np.random.RandomState(n % 100003 + len(kind))
    codes = _codes(kind, n, rs)
    ids = rs.permutation(n).astype(np.uint32)
    coords = pad4(rs.uniform(-1, 1, size=(n, 3)).astype(dt))
    radii = rs.uniform(0.001, 0.05, size=n).astype(dt)
    bufs = tuple(upload(ctx, a) for a in (codes, ids, coords, radii))
    nodes_d, bounds_d = _lbvh(ctx, cq, bufs, n, dt, 0)
    nodes_t, bounds_t = _lbvh(ctx, cq, bufs, n, dt, TABLES)
    ref_nodes = oracle.build_bvh(codes, ids)
    ref_bounds = oracle.node_bounds(coords, radii, ref_nodes)
    bits = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    np.testing.assert_array_equal(bounds_d.view(bits)[:, :, :3], ref_bounds.view(bits)[:, :, :3])
    np.testing.assert_array_equal(nodes_d["right_edge"], ref_nodes["right_edge"])
    np.testing.assert_array_equal(nodes_d["parent"][1:], ref_nodes["parent"][1:])
    np.testing.assert_array_equal(nodes_d["data"][:n - 1], ref_nodes["data"][:n - 1])
    assert bounds_d.tobytes() == bounds_t.tobytes()             # links included
    assert nodes_d.tobytes() == nodes_t.tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_direct_unions_f32(hip_env, oracle, kind, n):
    _check(hip_env, oracle, kind, n, "float32")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES[:3])
def test_direct_unions_f64(hip_env, oracle, kind, n):
    _check(hip_env, oracle, kind, n, "float64")


# all codes equal: the tree is balanced by position and the root's range is every chunk but the first and the last -- exactly 512
# chunks (the longest range one wave takes) and 513 (the shortest the whole workgroup takes)
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("chunks", [514, 515])
def test_wave_and_workgroup_boundary(hip_env, oracle, chunks, dt):
    _check(hip_env, oracle, "equal", 256 * chunks, dt)


@pytest.mark.parametrize("kind", ["uniform", "forty"])
def test_workgroup_unions_and_two_groups_f64(hip_env, oracle, kind):
    _check(hip_env, oracle, kind, 256 * 600, "float64")


@pytest.mark.parametrize("chunks", [MAX_DIRECT_CHUNKS, MAX_DIRECT_CHUNKS + 1])
def test_either_side_of_the_chunk_count_threshold(hip_env, oracle, chunks):
    """The largest size that takes the direct unions, and the smallest that keeps k_group (there the switch changes nothing)."""
    _check(hip_env, oracle, "uniform", 256 * chunks - 5, "float32")
