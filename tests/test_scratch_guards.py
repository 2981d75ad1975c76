"""Every call that carves a caller's scratch stays inside the size its query reports.

The size queries and the carves read the same layouts (csrc/collide.hip collide_layout, csrc/radix.hip radix_layout,
csrc/multi.hip ghost_layout).  Here each call gets a 256-byte aligned window of EXACTLY the reported size inside a larger
allocation filled with 0xA5: a carve that ran past the size would write into the guard behind the window (same allocation:
nothing faults), and the results must be right with nothing to spare.
"""
import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call
from collision_amd.collision import Collider
from tests.test_pipeline_parity import check_against_oracle, uniform_scene
from tests.util import download, pad4, upload

pytestmark = pytest.mark.gpu

GUARD = 4096


class Guarded:
    """`window`: nbytes at a 256-byte aligned address, at least GUARD bytes of 0xA5 in front of it and behind it."""

    def __init__(self, ctx, nbytes):
        self.nbytes = int(nbytes)
        self.whole = upload(ctx, np.full(self.nbytes + 2 * GUARD + 256, 0xA5, np.uint8))
        start = (self.whole.ptr + GUARD + 255) & ~255
        self.offset = start - self.whole.ptr
        self.window = hip.Buffer.from_ptr(ctx, start, self.nbytes, owner=self.whole)

    def check(self, cq):
        front = hip.read_buffer(cq, self.whole, np.uint8, self.offset)
        back_at = self.offset + self.nbytes
        back = hip.read_buffer(cq, self.whole, np.uint8, self.whole.size - back_at, offset=back_at)
        assert len(front) >= GUARD and len(back) >= GUARD
        assert (front == 0xA5).all(), "written in front of the scratch"
        assert (back == 0xA5).all(), "written %d bytes beyond the scratch" % (int(np.nonzero(back != 0xA5)[0].max()) + 1)


def guard_collider(ctx, made):
    """A check_against_oracle hook: the collider's scratch becomes a guarded window (same size: _allocate keeps it)."""
    def prepare(collider):
        collider._allocate()
        g = Guarded(ctx, collider._alloc["scratch"].size)
        collider._alloc["scratch"] = g.window
        made.append((collider, g))
    return prepare


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("traverse_plan", ["exact", "chunked"])
@pytest.mark.parametrize("sort_plan", ["lsd", "msd"])
@pytest.mark.parametrize("n,r", [(1000, 0.03), (5000, 0.01)])
def test_whole_path_stays_inside_its_scratch(oracle, hip_env, n, r, sort_plan, traverse_plan, dtype):
    """n = 1000: padded 1024 -- one sort tile, four tree chunks (k_cross runs); n = 5000: padded 5120 -- several tiles, a
    ragged last chunk.  Every array and the pair set against the oracle, as tests/test_pipeline_parity.py does."""
    ctx, cq = hip_env
    coords, radii = uniform_scene(n, r, dtype)
    made = []
    check_against_oracle(oracle, hip_env, coords, radii, group_size=64, sort_plan=sort_plan, traverse_plan=traverse_plan,
                         extra_capacity=512 * 8192 + 1000 if traverse_plan == "chunked" else 0, prepare=guard_collider(ctx, made))
    (collider, g), = made
    assert collider._alloc["scratch"] is g.window and collider.padded_size == (1024 if n == 1000 else 5120)
    g.check(cq)


@pytest.fixture(scope="module")
def big_scene(oracle):
    """2^20 uniform spheres and the oracle's count-only results for its first 786432 and for all of them (computed once)."""
    coords, radii = uniform_scene(1 << 20, 0.002, "float32")
    return coords, radii, {n: oracle.collide(oracle.pad4(coords[:n]), radii[:n], padded=n, capacity=0) for n in (786432, 1 << 20)}


@pytest.mark.parametrize("n", [786432, 1 << 20])
def test_msd_carves_of_the_large_tiles_stay_inside(hip_env, big_scene, n):
    """Count-only MSD calls at the smallest sizes of two carves: padded = 786432, where the gather finish carves for the
    Morton kernel's 4096-code tile, and padded = 2^20, where the fused scatter pass (4096-pair tile) first runs."""
    ctx, cq = hip_env
    coords, radii, refs = big_scene
    ref = refs[n]
    collider = Collider(ctx, n, 8, 64)
    collider.sort_plan, collider.traverse_plan = "msd", "exact"
    assert collider.padded_size == n
    collider._allocate()
    g = Guarded(ctx, collider._alloc["scratch"].size)
    collider._alloc["scratch"] = g.window
    nbuf = hip.Buffer(ctx, 4)
    e = collider.get_collisions(cq, upload(ctx, pad4(coords[:n])), upload(ctx, radii[:n]), nbuf, None, 0)
    count = int(download(cq, nbuf, np.uint32, 1, wait_for=[e])[0])
    assert collider._alloc["scratch"] is g.window
    assert count == ref["count"]
    np.testing.assert_array_equal(download(cq, collider._codes_bufs[1], np.uint32, n), ref["codes"])
    assert collider.oversize_bucket == 0
    g.check(cq)


@pytest.mark.parametrize("kb,vb", [(4, 4), (8, 8), (4, 32), (1, 4), (2, 64), (4, 128)])
def test_radix_sort_stays_inside_its_scratch(hip_env, kb, vb):
    """n = 3000: three 1024-pair tiles, the last one ragged; native, narrow-key and wide-value sorts (the last two carve
    their tails behind the u32 sort's scratch)."""
    ctx, cq = hip_env
    n = 3000
    rs = np.random.RandomState(kb * 131 + vb)
    key_dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[kb]
    keys = (rs.randint(0, 1 << 62, size=n, dtype=np.uint64) >> np.uint64(64 - 8 * kb if kb < 8 else 2)).astype(key_dtype)
    keys[::7] = keys[3]                                        # duplicates: stability matters
    vals = rs.randint(0, 256, size=(n, vb)).astype(np.uint8)
    g = Guarded(ctx, call.col_radix_scratch_bytes(n, kb, vb))
    kbuf, vbuf = upload(ctx, keys), upload(ctx, vals)
    ko, vo = hip.Buffer(ctx, keys.nbytes), hip.Buffer(ctx, vals.nbytes)
    call.col_radix_sort(cq.stream, kbuf.ptr, ko.ptr, vbuf.ptr, vo.ptr, n, kb, vb, g.window.ptr, 0)
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(download(cq, ko, key_dtype, n), keys[order])
    np.testing.assert_array_equal(download(cq, vo, np.uint8, (n, vb)), vals[order])
    g.check(cq)


def test_msd_sort_stays_inside_its_scratch(hip_env):
    """col_radix_sort_msd at n = 3000 with the bucket-digit histogram at the start of its scratch, fed as
    tests/test_radix_kernels.py feeds it."""
    ctx, cq = hip_env
    rs = np.random.RandomState(3000)
    keys = np.concatenate([rs.randint(0, 1 << 30, size=2900, dtype=np.uint64).astype(np.uint32), np.full(100, 0xFFFFFFFF, np.uint32)])
    keys[:2900:5] = keys[1]
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    tile = call.col_radix_tile(n, 4, 4)
    assert tile == 1024
    nb = -(-n // tile)
    d8 = ((keys >> np.uint32(22)) & np.uint32(255)).astype(np.int64)
    hist = np.zeros((256, nb), np.uint32)
    np.add.at(hist, (d8, np.arange(n) // tile), 1)
    g = Guarded(ctx, call.col_radix_scratch_bytes(n, 4, 4))
    kbuf, vbuf = upload(ctx, keys), upload(ctx, vals)
    ko, vo = hip.Buffer(ctx, keys.nbytes), hip.Buffer(ctx, vals.nbytes)
    flag = upload(ctx, np.zeros(1, np.uint32))
    hip.write_buffer(cq, g.window, hist)
    call.col_radix_sort_msd(cq.stream, kbuf.ptr, ko.ptr, vbuf.ptr, vo.ptr, n, g.window.ptr, flag.ptr)
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(download(cq, ko, np.uint32, n), keys[order])
    np.testing.assert_array_equal(download(cq, vo, np.uint32, n), order.astype(np.uint32))
    assert int(download(cq, flag, np.uint32, 1)[0]) == 0
    g.check(cq)


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_ghost_walk_stays_inside_its_scratch(hip_env, dt):
    """col_traverse_ghost_slots' packet walk (3 slots of 4096 records against a tree of 20000 spheres, the shape of
    tests/test_multi_kernels.py): every (ghost, local) AABB overlap against NumPy."""
    ctx, cq = hip_env
    cb = np.dtype(dt).itemsize
    rw = cb + 1                                              # words per record: an (x, y, z, r) row and a global id
    n_slots, slot, m = 3, 4096, 20000
    rng = np.random.RandomState(7)

    def rows_of(k, radius):
        rows = np.empty((k, 4), dt)
        rows[:, :3] = rng.random_sample((k, 3))
        rows[:, 3] = rng.uniform(0.2, 1.0, size=k) * radius
        return rows
    local = rows_of(m, 0.02)
    lg = np.arange(m, dtype=np.uint32) + 5000000
    col = Collider(ctx, m, 16, 64, dt)
    col.get_collisions(cq, upload(ctx, local), upload(ctx, np.ascontiguousarray(local[:, 3])), hip.Buffer(ctx, 4), None, 0)
    counts = [4096, 1, 2500]                                 # a full slot, a single ghost, a ragged one
    rec = np.full((n_slots, slot + 1, rw), 0xCDCDCDCD, np.uint32)
    ghosts, ggids = [], []
    for k, cnt in enumerate(counts):
        rows = rows_of(cnt, 0.01)
        gid = (rng.permutation(1 << 20)[:cnt] + (k << 20)).astype(np.uint32)
        rec[k, 0] = 0
        rec[k, 0, 0] = cnt
        rec[k, 1:1 + cnt, :rw - 1] = rows.view(np.uint32).reshape(cnt, rw - 1)
        rec[k, 1:1 + cnt, rw - 1] = gid
        ghosts.append(rows)
        ggids.append(gid)
    ghosts, ggids = np.concatenate(ghosts), np.concatenate(ggids)
    cap = 1 << 20
    pairs, counter, flags = hip.Buffer(ctx, cap * 8), upload(ctx, np.zeros(1, np.uint32)), upload(ctx, np.zeros(4, np.uint32))
    g = Guarded(ctx, call.col_ghost_scratch_bytes(n_slots, slot))
    rec_buf, lg_buf = upload(ctx, rec), upload(ctx, lg)
    call.col_traverse_ghost_slots(cq.stream, rec_buf.ptr, n_slots, slot, col._bounds_buf.ptr, m, lg_buf.ptr,
                                  pairs.ptr, counter.ptr, cap, flags.ptr, cb, g.window.ptr)
    count = int(download(cq, counter, np.uint32, 1)[0])
    got = download(cq, pairs, np.uint32, (min(count, cap), 2))
    llo, lhi = local[:, :3] - local[:, 3:4], local[:, :3] + local[:, 3:4]
    glo, ghi = ghosts[:, :3] - ghosts[:, 3:4], ghosts[:, :3] + ghosts[:, 3:4]
    expect = []
    for s in range(len(ghosts)):
        hit = ((ghi[s] > llo) & (glo[s] < lhi)).all(axis=1)
        expect += [(int(ggids[s]), int(lg[j])) for j in np.nonzero(hit)[0]]
    assert count == len(expect) <= cap and expect
    assert sorted(map(tuple, got.tolist())) == sorted(expect)
    g.check(cq)
