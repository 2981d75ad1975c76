"""The scene zoo (tests/zoo.py) through the device steps of the multi-GPU path (collision_amd/csrc/multi.hip), each in
isolation through the C ABI and bit for bit against NumPy and the oracle's Morton codes.  Until here these kernels had seen
unit-cube coordinates with radii in U(0.001, 0.004) only (tests/test_multi_kernels.py).  No tolerance anywhere: every result
is a min, a max, a compare, an integer or ONE correctly rounded operation (c - r, c + r, min - rmax, max + rmax), and
quantize()'s four operations are the oracle's.

"Local" is the family's scene at n = 4099 (seed 4), "other" the same family at 1500 with seed 5; rows are (x, y, z, r); the
global range is the centre range of local + other.  4099 = 17 chunks with crossing nodes in the local tree, 17 blocks of
the select kernel (the last with 3 rows), 5 tiles of k_owners; 1500 ghosts in slots of 512 = 24 packets, the last with 28.

Measured with these references (f32 / f64 where they differ):
  b. rows whose code octant is not the geometric-midpoint octant: 6-11 per family and dtype (range_overflow: none, one octant)
  c. halo list lengths, peers 0..3 (f32; f64 differs by one in a list of offset and of neg_offset):
       log_radii [1883, 2053, 2077, 1872]  zero_and_giant [1128, 4099, 1102, 1123]  offset [1285, 1387, 1308, 1263]
       neg_offset [1445, 1588, 1524, 1424] aniso [2116, 2303, 2002, 2008]          tiny = huge [1351, 1468, 1404, 1333]
       range_overflow [4099, 4099, 4099, 4099] (one octant: every peer's box 0 spans its whole range)
     zero_and_giant: 3078 empty boxes are in one of the three lists that are not everything, 977 in none of them
  d. ghost x local leaf-box overlaps: log_radii 15345, zero_and_giant 5607 (one ghost hits all 4099), offset 9499 / 9437,
     neg_offset 14723 / 14725, aniso 41509, tiny = huge 8297, range_overflow 8638"""
import ctypes as C

import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call, cdll
from collision_amd.multi import REGION_BOXES, SAMPLES, hash_owner
from tests.test_multi_kernels import _payload, _plan, _sample
from tests.test_multi_zoo_cpu import rows_of
from tests.util import download, upload
from tests.zoo import DTYPES, FAMILIES

pytestmark = pytest.mark.gpu

N_LOCAL, N_OTHER, WORLD = 4099, 1500, 4
GHOST_HITS = {   # family: (f32, f64), section d; measured with overlaps() below -- the test asserts NumPy's own figure
    "log_radii": (15345, 15345), "zero_and_giant": (5607, 5607), "offset": (9499, 9437), "neg_offset": (14723, 14725),
    "aniso": (41509, 41509), "tiny": (8297, 8297), "huge": (8297, 8297), "range_overflow": (8638, 8638),
}
_scenes = {}


# ------------------------------------------------------------------------------------------------ references (NumPy + oracle)
def scenes(family, dt):
    """(local rows, other rows, global centre range [2][4]); once per case, read-only."""
    key = (family, np.dtype(dt).name)
    if key not in _scenes:
        local, other = rows_of(family, N_LOCAL, dt), rows_of(family, N_OTHER, dt, seed=5)
        both = np.concatenate([local, other])
        grange = np.stack([both.min(axis=0), both.max(axis=0)])
        for a in (local, other, grange):
            a.setflags(write=False)
        _scenes[key] = (local, other, grange)
    return _scenes[key]


def octants(oracle, rows, grange):
    return (oracle.morton(rows, grange) >> 27).astype(np.int64)


def midpoint_octants(rows, grange):
    """The octant by the geometric 'side of the middle' test: what k_region_part must NOT compute."""
    with np.errstate(over="ignore"):
        mid = grange[0, :3] + (grange[1, :3] - grange[0, :3]) / 2
    side = rows[:, :3] >= mid
    return (side[:, 0].astype(np.int64) << 2) | (side[:, 1].astype(np.int64) << 1) | side[:, 2].astype(np.int64)


def region_boxes(rows, octant):
    """[8][2][4]: (min centre - max r, 0), (max centre + max r, 0) of each octant's rows in the rows' dtype; empty = inverted."""
    out = np.zeros((REGION_BOXES, 2, 4), rows.dtype)
    out[:, 0, :3], out[:, 1, :3] = np.inf, -np.inf
    for o in range(REGION_BOXES):
        sel = rows[octant == o]
        if len(sel):
            rmax = sel[:, 3].max()
            out[o, 0, :3], out[o, 1, :3] = sel[:, :3].min(axis=0) - rmax, sel[:, :3].max(axis=0) + rmax
    assert out.dtype == rows.dtype
    return out


def boxes_of(rows):
    lo, hi = rows[:, :3] - rows[:, 3:4], rows[:, :3] + rows[:, 3:4]
    assert lo.dtype == rows.dtype and hi.dtype == rows.dtype
    return lo, hi


def overlaps(a, b):
    """bool [len(a)][len(b)]: strict AABB overlap of the spheres' boxes, c -+ r computed in the rows' dtype."""
    alo, ahi = boxes_of(a)
    blo, bhi = boxes_of(b)
    hit = np.ones((len(a), len(b)), bool)
    for k in range(3):
        hit &= (ahi[:, None, k] > blo[None, :, k]) & (alo[:, None, k] < bhi[None, :, k])
    return hit


def peer_regions(oracle, other, grange):
    """[4][8][2][4]: `other` sorted by its code (stable), cut into 4 equal Morton ranges, each range's 8 region boxes."""
    order = np.argsort(oracle.morton(other, grange), kind="stable")
    pieces = np.split(other[order], WORLD)
    return np.stack([region_boxes(p, octants(oracle, p, grange)) for p in pieces])


def selected(local, regions):
    """[4] index arrays: the local spheres whose box strictly overlaps one of a peer's boxes."""
    lo, hi = boxes_of(local)
    out = []
    for q in range(len(regions)):
        hit = np.zeros(len(local), bool)
        for b in regions[q]:
            hit |= ((hi > b[0, :3]) & (lo < b[1, :3])).all(axis=1)
        out.append(np.nonzero(hit)[0])
    return out


def records(rows, gids, n_slots, slot):
    """Host-built transport slots: header = the list's length, then its records (4 scalars as words, gid)."""
    rw = rows.dtype.itemsize + 1
    rec = np.full((n_slots, slot + 1, rw), 0xCDCDCDCD, np.uint32)
    for k in range(n_slots):
        part = slice(k * slot, min((k + 1) * slot, len(rows)))
        cnt = len(rows[part])
        rec[k, 0] = 0
        rec[k, 0, 0] = cnt
        rec[k, 1:1 + cnt, :rw - 1] = np.ascontiguousarray(rows[part]).view(np.uint32).reshape(cnt, rw - 1)
        rec[k, 1:1 + cnt, rw - 1] = gids[part]
    return rec


def expected_pairs(ghosts, ghost_gids, local, local_gids):
    g, j = np.nonzero(overlaps(ghosts, local))
    return sorted(zip(ghost_gids[g].tolist(), local_gids[j].tolist()))


def _pairs_sorted(p):
    return sorted(map(tuple, np.asarray(p).tolist()))


# ------------------------------------------------------------------------------------------------ a. sample and plan
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_sample_and_plan(hip_env, oracle, family, dt):
    """k_range_part / k_range_fold, k_splitters, k_owners, k_owner_offsets on a hash split of the local scene: the payloads,
    the folded range (all four lanes), the splitters = exact order statistics of the oracle's codes of all gathered rows,
    dest, owner_counts.  range_overflow: every code is 0, so is every splitter, and every row goes to the last owner."""
    ctx, cq = hip_env
    local, _, _ = scenes(family, dt)
    owner = hash_owner(np.arange(N_LOCAL, dtype=np.uint32), WORLD)
    pieces = [np.ascontiguousarray(local[owner == q]) for q in range(WORLD)]
    payloads = []
    for piece in pieces:
        got, flags = _sample(ctx, cq, piece, dt)
        np.testing.assert_array_equal(got.view(np.uint8), _payload(piece).view(np.uint8))
        assert not flags.any()
        payloads.append(got)
    gathered = np.stack(payloads)
    rows = pieces[0]
    bufs, _ = _plan(ctx, cq, gathered, rows, WORLD, dt)
    grange = np.stack([gathered[:, SAMPLES].min(axis=0), gathered[:, SAMPLES + 1].max(axis=0)])
    np.testing.assert_array_equal(download(cq, bufs["range8"], dt, (2, 4)), grange)
    np.testing.assert_array_equal(grange, np.stack([local.min(axis=0), local.max(axis=0)]))
    codes = np.sort(oracle.morton(gathered.reshape(-1, 4), grange))
    want_split = codes[np.arange(1, WORLD) * (len(codes) // WORLD)]
    np.testing.assert_array_equal(download(cq, bufs["split"], np.uint32, 256)[:WORLD - 1], want_split)
    mine = oracle.morton(rows, grange)
    want_dest = np.searchsorted(want_split, mine, side="right").astype(np.uint32)
    np.testing.assert_array_equal(download(cq, bufs["dest"], np.uint32, len(rows)), want_dest)
    np.testing.assert_array_equal(download(cq, bufs["counts"], np.uint32, 256)[:WORLD], np.bincount(want_dest, minlength=WORLD))
    if family == "range_overflow":
        with np.errstate(over="ignore"):
            assert np.isinf(grange[1, :3] - grange[0, :3]).all()
        assert not want_split.any() and (want_dest == WORLD - 1).all()
    else:
        assert len(np.unique(want_split)) == WORLD - 1 and np.bincount(want_dest, minlength=WORLD).min() > len(rows) // 8


# ------------------------------------------------------------------------------------------------ b. region boxes
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_region_boxes(hip_env, oracle, family, dt):
    """k_region_part's octant is the top three bits of the row's OWN Morton code (a bisected threshold per axis over the
    ordered bit patterns of quantize()), and k_region_fold's box is min - rmax / max + rmax.  Every family has rows between
    the range's middle and the first coordinate that quantises to 512: a midpoint test puts them into another octant.
    range_overflow: (p - mn) / inf is 0 or NaN, no coordinate reaches 512 -- the kernel's NaN threshold, one octant."""
    ctx, cq = hip_env
    cb = np.dtype(dt).itemsize
    local, _, grange = scenes(family, dt)
    octant = octants(oracle, local, grange)
    used = np.unique(octant)
    if family == "range_overflow":
        assert list(used) == [0]
    else:
        assert list(used) == list(range(8))
        assert (octant != midpoint_octants(local, grange)).sum() >= 1
    want = region_boxes(local, octant)
    scratch = hip.Buffer(ctx, call.col_partition_scratch_bytes())
    counters = upload(ctx, np.full(8, 5, np.uint32))
    out = upload(ctx, np.full((REGION_BOXES, 2, 4), 77, dt))
    rows_buf, range_buf = upload(ctx, local), upload(ctx, grange)
    call.col_region_boxes(cq.stream, rows_buf.ptr, N_LOCAL, range_buf.ptr, scratch.ptr, out.ptr, counters.ptr, 8, cb)
    got = download(cq, out, dt, (REGION_BOXES, 2, 4))
    assert not download(cq, counters, np.uint32, 8).any()
    for o in range(REGION_BOXES):
        if o not in used:
            assert np.isposinf(got[o, 0, :3]).all() and np.isneginf(got[o, 1, :3]).all()
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(want[used]).all() and (got[:, :, 3] == 0).all()


# ------------------------------------------------------------------------------------------------ c. select and pack
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_select_and_pack(hip_env, oracle, family, dt):
    """k_select_multi forms c -+ r itself and tests strictly against the peers' region boxes; k_pack_slots copies the rows
    bit for bit.  zero_and_giant: an empty box is selected only where its point lies strictly inside a region box."""
    ctx, cq = hip_env
    cb = np.dtype(dt).itemsize
    rw = cb + 1
    n = N_LOCAL
    local, other, grange = scenes(family, dt)
    regions = peer_regions(oracle, other, grange)
    want = selected(local, regions)
    gids = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(9)
    rows_buf, gids_buf, boxes_buf = upload(ctx, local), upload(ctx, gids), upload(ctx, regions)
    lists, counts = hip.Buffer(ctx, 8 * n * 4), upload(ctx, np.zeros(8, np.uint32))
    call.col_select_overlap_multi(cq.stream, rows_buf.ptr, n, boxes_buf.ptr, (C.c_int * WORLD)(0, 1, 2, 3), WORLD, n,
                                  lists.ptr, counts.ptr, cb)
    got_counts = download(cq, counts, np.uint32, 8)
    got_lists = download(cq, lists, np.uint32, (8, n))
    assert list(got_counts[:WORLD]) == [len(w) for w in want] and not got_counts[WORLD:].any()
    for k in range(WORLD):
        np.testing.assert_array_equal(np.sort(got_lists[k, :len(want[k])]), want[k])
    assert sum(len(w) for w in want) > n                    # (no vacuous case: every family selects plenty)
    if family == "zero_and_giant":
        zero = local[:, 3] == 0
        in_lists = np.zeros((WORLD, n), bool)
        for k in range(WORLD):
            in_lists[k, want[k]] = True
        assert in_lists[:, n // 2].all()                    # the giant
        # the other scene has a giant of its own: the region of the peer that owns it contains the scene, so every sphere
        # is in THAT list; in the three other lists an empty box is in or out by the strict test on its point alone
        full = [k for k in range(WORLD) if len(want[k]) == n]
        assert len(full) == 1
        rest = np.delete(in_lists, full[0], axis=0)
        assert (rest.any(axis=0) & zero).any() and (~rest.any(axis=0) & zero).any()
    for slot in (n, 100):
        send = upload(ctx, np.full(WORLD * (slot + 1) * rw, 0xCDCDCDCD, np.uint32))
        call.col_pack_slots(cq.stream, rows_buf.ptr, gids_buf.ptr, lists.ptr, n, counts.ptr, WORLD, min(n, slot), send.ptr,
                            WORLD * (slot + 1), slot, cb)
        rec = download(cq, send, np.uint32, (WORLD, slot + 1, rw))
        for k in range(WORLD):
            cnt = min(len(want[k]), slot)
            assert rec[k, 0, 0] == len(want[k]) and not rec[k, 0, 1:].any()
            src = got_lists[k, :cnt]
            np.testing.assert_array_equal(rec[k, 1:1 + cnt, :rw - 1], local[src].view(np.uint32).reshape(cnt, rw - 1))
            np.testing.assert_array_equal(rec[k, 1:1 + cnt, rw - 1], gids[src])
            assert (rec[k, 1 + cnt:] == 0xCDCDCDCD).all()
        if slot == 100:
            assert all(len(w) > 100 for w in want)          # (every list overflows this slot: 100 records each)


# ------------------------------------------------------------------------------------------------ d. ghost walks
def _ghost_walks(ctx, cq, rec, n_slots, slot, bounds_ptr, n, lg_buf, cb, n_dev=None, cap=1 << 20):
    """Both walks -- packets (with scratch), lanes (without) -- over the same slots: [(count, pairs, flags)] * 2."""
    results = []
    rec_buf = upload(ctx, rec)
    for packets in (True, False):
        pairs, counter, flags = hip.Buffer(ctx, cap * 8), upload(ctx, np.zeros(1, np.uint32)), upload(ctx, np.zeros(4, np.uint32))
        scratch = hip.Buffer(ctx, call.col_ghost_scratch_bytes(n_slots, slot)) if packets else None
        if n_dev is None:
            call.col_traverse_ghost_slots(cq.stream, rec_buf.ptr, n_slots, slot, bounds_ptr, n, lg_buf.ptr, pairs.ptr,
                                          counter.ptr, cap, flags.ptr, cb, scratch.ptr if packets else None)
        else:
            call.col_traverse_ghost_slots_dev(cq.stream, rec_buf.ptr, n_slots, slot, bounds_ptr, n, lg_buf.ptr, pairs.ptr,
                                              counter.ptr, cap, flags.ptr, cb, scratch.ptr if packets else None, n_dev)
        count = int(download(cq, counter, np.uint32, 1)[0])
        assert count <= cap
        results.append((count, download(cq, pairs, np.uint32, (count, 2)) if count else np.empty((0, 2), np.uint32),
                        download(cq, flags, np.uint32, 4)))
    return results


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_ghost_walks_against_a_zoo_tree(hip_env, oracle, family, dt):
    """All 1500 spheres of the other scene as ghosts (3 slots of 512) against the tree over the local scene: k_ghost (lane
    per ghost) and k_ghost_codes + the packet walk, with the tree built without leaf blocks (k = 0), with the default
    criterion (3) and with every small node marked (1e30) -- the ghost walks read the marks.  Every (ghost, leaf) pair whose
    boxes overlap strictly, each once; count, flags[0] (longest header) and flags[1] (ghosts) exact.  Ghost centres outside
    the local centre range (and so on or beyond the edge of the root box's centres) go through k_ghost_codes' clamp."""
    from collision_amd.collision import Collider
    ctx, cq = hip_env
    cb = np.dtype(dt).itemsize
    local, other, _ = scenes(family, dt)
    ghost_gids = np.arange(N_OTHER, dtype=np.uint32) + 1000000
    lg = np.arange(N_LOCAL, dtype=np.uint32) + 5000000
    expect = expected_pairs(other, ghost_gids, local, lg)
    assert 0 < len(expect) < 1 << 20 and len(expect) == GHOST_HITS[family][DTYPES.index(dt)]
    if family == "zero_and_giant":
        assert (overlaps(other, local).sum(axis=1) == N_LOCAL).sum() == 1
    outside = ((other[:, :3] < local[:, :3].min(axis=0)) | (other[:, :3] > local[:, :3].max(axis=0))).any(axis=1).sum()
    if (family, dt) != ("offset", "float32"):
        assert outside >= 1
    slot, n_slots = 512, 3
    rec = records(other, ghost_gids, n_slots, slot)
    col = Collider(ctx, N_LOCAL, 16, 64, dt)
    rows_buf, radii_buf, lg_buf = upload(ctx, local), upload(ctx, np.ascontiguousarray(local[:, 3])), upload(ctx, lg)
    nb = hip.Buffer(ctx, 4)
    lib = cdll()
    lib.col_debug_leaf_blocks.argtypes = [C.c_float]
    try:
        for k in (0.0, 3.0, 1e30):
            lib.col_debug_leaf_blocks(C.c_float(k))
            col.get_collisions(cq, rows_buf, radii_buf, nb, None, 0)
            cq.finish()
            for count, got, flags in _ghost_walks(ctx, cq, rec, n_slots, slot, col._bounds_buf.ptr, N_LOCAL, lg_buf, cb):
                assert count == len(expect)
                assert _pairs_sorted(got) == expect
                assert flags[0] == slot and flags[1] == N_OTHER and not flags[2:].any()
    finally:
        lib.col_debug_leaf_blocks(C.c_float(3.0))


# ------------------------------------------------------------------------------------------------ e. trees of 0..3 spheres
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("count", [0, 1, 2, 3])
def test_ghost_walks_against_a_tree_of_a_few_spheres(hip_env, oracle, dt, count):
    """A rank that owns one sphere must still answer for it.  The tree is built under a DEVICE-side count (bound 5000) by
    col_minmax4_stage1_dev + col_collide_plan_dev with a Node array, then 300 ghosts (2 slots of 256: 256 + 44) walk it
    through col_traverse_ghost_slots_dev with n = the bound and the count word, packets and lanes.

    What the code does at a count of 1, read before this ran (csrc/lbvh.hip, k_chunk and run<T>; csrc/multi.hip, k_ghost;
    csrc/bvh.hip, k_traverse<GHOST> and launch_ghost):
    * k_chunk clamps its chunk count to ceil(count / 256) = 1; thread 0 of chunk 0 is the one valid leaf, p = 0 and
      leaf_start = count - 1 = 0, so `record_store(bounds, leaf_start + p, leaf, skip_leaf, id)` writes NODE 0 as a leaf:
      its box c -+ r, END as the skip link (p + 1 < n fails) in min.w and the sphere's id in max.w; with NODES the leaf
      tail goes to nodes[0].  The climb leaves at once (both adjacent deltas are -1: the root), `p >= leaf_start` returns
      every thread before the internal records, and k_cross finds chunk 0's crossing list all END.
    * every walk starts a ghost at index 0 and tests `idx >= leaf_start`: k_ghost in C++, the packet walk as
      `s_cmp_ge_u32 offset, leaf_start * 32 (64)` in the asm walks and `idx >= leaf_start` in the generic one -- index 0 IS
      a leaf when leaf_start is 0, the hit is staged with max.w as the local id, and the END skip link ends the walk.
    * at a count of 0: k_chunk leaves before it touches anything (`bid >= nb`), k_ghost keeps idx = END (`n > 0`), the
      packet walk's kernel returns (`n_dev && n < 1`); k_ghost_codes still gives the ghosts keys under whatever node 0
      holds (quantize() clamps, NaN -> 0) and counts them: no pairs, flags[1] = 300.
    So nothing had to change."""
    from collision_amd.collision import Collider
    ctx, cq = hip_env
    cb = np.dtype(dt).itemsize
    bound, n_ghosts, slot, n_slots = 5000, 300, 256, 2
    local = rows_of("log_radii", N_LOCAL, dt)[:count]
    ghosts = rows_of("log_radii", n_ghosts, dt, seed=6)        # (seed 5's ghosts miss sphere 0; these hit 3, 1 and 1 times)
    ghost_gids = np.arange(n_ghosts, dtype=np.uint32) + 1000000
    lg = np.arange(bound, dtype=np.uint32) + 5000000
    expect = expected_pairs(ghosts, ghost_gids, local, lg[:count])
    assert (len(expect) > 0) == (count > 0)
    if count:
        assert overlaps(ghosts, local).any(axis=0).all()        # every local sphere is somebody's hit
    col = Collider(ctx, bound, 16, 256, dt)
    col._allocate()
    rows = np.full((bound, 4), 7.0, dt)                        # rows beyond the count: never read as spheres
    rows[:count] = local
    rad = np.full(bound, 3.0, dt)
    rad[:count] = local[:, 3]
    rb, qb = upload(ctx, rows), upload(ctx, rad)
    cap = 1 << 16
    nb, pb, word = hip.Buffer(ctx, 4), hip.Buffer(ctx, cap * 8), upload(ctx, np.array([count, count], np.uint32))
    partials, parts = hip.Buffer(ctx, 256 * 8 * cb), C.c_uint32(0)
    call.col_minmax4_stage1_dev(cq.stream, rb.ptr, word.ptr, bound, cb, partials.ptr, C.byref(parts))
    call.col_collide_plan_dev(cq.stream, rb.ptr, qb.ptr, bound, col.padded_size, cb, col._codes_bufs[0].ptr, col._codes_bufs[1].ptr,
                              col._ids_bufs[0].ptr, col._ids_bufs[1].ptr, col._nodes_buf.ptr, col._bounds_buf.ptr, None,
                              col._alloc["scratch"].ptr, nb.ptr, pb.ptr, cap, 1, None, partials.ptr, parts.value, word.ptr)
    cq.finish()
    if count == 1:                                             # node 0 is the leaf record
        got = download(cq, col._bounds_buf, dt, (1, 2, 4))
        lo, hi = boxes_of(local)
        np.testing.assert_array_equal(got[0, 0, :3], lo[0])
        np.testing.assert_array_equal(got[0, 1, :3], hi[0])
        links = got.view(np.uint32 if cb == 4 else np.uint64)[0, :, 3]
        assert int(links[0]) & 0xFFFFFFFF == 0xFFFFFFFF and int(links[1]) & 0xFFFFFFFF == 0
    rec = records(ghosts, ghost_gids, n_slots, slot)
    for n_pairs, got, flags in _ghost_walks(ctx, cq, rec, n_slots, slot, col._bounds_buf.ptr, bound, upload(ctx, lg), cb,
                                            n_dev=word.ptr, cap=cap):
        assert n_pairs == len(expect)
        assert _pairs_sorted(got) == expect
        assert flags[0] == slot and flags[1] == n_ghosts
