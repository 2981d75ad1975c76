"""k_chunk_wide, the 64-bit-index chunk kernel (csrc/lbvh.hip), is the only code that builds trees of n >= 2^30 leaves: shuffle
scans and Karras' searches for every node, where the production k_chunk has DPP scans, adjacent deltas and the climb.
col_debug_lbvh bit 1024 selects it at every size: col_lbvh on sorted codes must give the oracle's boxes and node records
bit for bit, and the same bytes -- traversal links and leaf-block marks included -- as the production kernel."""
import numpy as np
import pytest

from tests.test_cross_direct_unions import _codes, _lbvh
from tests.util import pad4, upload

pytestmark = pytest.mark.gpu

WIDE = 1024                 # col_debug_lbvh: k_chunk_wide at every size
# one chunk, two chunks, a range longer than one thread of k_cross reads (8 whole chunks), two groups of 256 chunks
SIZES = [2, 257, 256 * 11 + 1, 256 * 257 + 3]
KINDS = ["uniform", "equal"]


def _check(hip_env, oracle, kind, n, dt):
    ctx, cq = hip_env
    rs = np.random.RandomState(n % 100003 + len(kind))
    codes = _codes(kind, n, rs)
    ids = rs.permutation(n).astype(np.uint32)
    coords = pad4(rs.uniform(-1, 1, size=(n, 3)).astype(dt))
    radii = rs.uniform(0.001, 0.05, size=n).astype(dt)
    bufs = tuple(upload(ctx, a) for a in (codes, ids, coords, radii))
    nodes_p, bounds_p = _lbvh(ctx, cq, bufs, n, dt, 0)
    nodes_w, bounds_w = _lbvh(ctx, cq, bufs, n, dt, WIDE)
    ref_nodes = oracle.build_bvh(codes, ids)
    ref_bounds = oracle.node_bounds(coords, radii, ref_nodes)
    bits = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    np.testing.assert_array_equal(bounds_w.view(bits)[:, :, :3], ref_bounds.view(bits)[:, :, :3])
    np.testing.assert_array_equal(nodes_w["right_edge"], ref_nodes["right_edge"])
    np.testing.assert_array_equal(nodes_w["parent"][1:], ref_nodes["parent"][1:])
    np.testing.assert_array_equal(nodes_w["data"][:n - 1], ref_nodes["data"][:n - 1])
    links_w, links_p = bounds_w.view(bits)[:, :, 3], bounds_p.view(bits)[:, :, 3]
    print("wide-index vs production, %s n = %d %s: skip links differ at %d nodes, down links / marks at %d, node words at %d"
          % (kind, n, dt, int((links_w[:, 0] != links_p[:, 0]).sum()), int((links_w[:, 1] != links_p[:, 1]).sum()),
             int((nodes_w.view(np.uint32) != nodes_p.view(np.uint32)).sum())))
    assert bounds_w.tobytes() == bounds_p.tobytes()             # links and marks included
    assert nodes_w.tobytes() == nodes_p.tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_wide_index_f32(hip_env, oracle, kind, n):
    _check(hip_env, oracle, kind, n, "float32")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES[:3])
def test_wide_index_f64(hip_env, oracle, kind, n):
    _check(hip_env, oracle, kind, n, "float64")
