"""The MSD plan's 1024-pair tile class has no global pass (csrc/morton.hip, k_morton_tile SORTED; csrc/radix.hip, k_bucket_sort
GATHER): the Morton kernel leaves every tile sorted by the bucket digit (code bits 22..29) with a table of (start, count)
words, and the workgroup of bucket d gathers its piece of every tile itself -- a piece of up to _piece(tiles) pairs by its
tile's own lanes, a longer one by a wave.  The tiles hold 1024 codes below BIG_FROM codes and 4096 from there on.  The sorted codes and ids must be np.argsort(kind="stable") of the oracle's codes plus pads,
bit for bit, whatever the tile count, the input order, the piece lengths, the bucket sizes around the LDS capacity and the
place of the device-side count."""
import ctypes as C

import numpy as np
import pytest

from collision_amd import hip
from collision_amd._lib import call
from collision_amd.collision import Collider
from tests.util import download, upload

pytestmark = pytest.mark.gpu

MSD = 1                     # sort_plan bit 0
PADS = 3                    # padded = n + PADS: the last tile stays ragged and ends in a few pads
TILE, BIG_TILE = 1024, 4096
BIG_FROM = 768 << 10        # COL_GATHER_BIG_FROM (csrc/col_common.h): 4096-code tiles from this many codes (pads included) on
BIG_N = 193 * BIG_TILE - 7  # a scene of 193 such tiles, the last one ragged
CAP = 8192                  # pairs of one bucket the LDS finish holds (k_bucket_sort<8>)


def _digit(codes):
    return (codes >> 22) & 255


def _tile_of(padded):
    return BIG_TILE if padded >= BIG_FROM else TILE


def _piece(tiles):
    """gather_piece (csrc/radix.hip): the longest piece a tile's own lanes copy -- 2^glog lanes of the workgroup's 1024 (at most
    16) with four 16-byte vectors each, at any alignment."""
    glog = 0
    while glog < 4 and (tiles << (glog + 1)) <= 1024:
        glog += 1
    return (16 << glog) - 3


def _cells_in_bucket(d, count, rng):
    """`count` random cells of the 1024^3 grid whose code has the top digit d (one digit, or one per cell): the digit is
    x9 y9 z9 x8 y8 z8 x7 y7."""
    d = np.asarray(d, np.int64)
    bit = lambda k: (d >> k) & 1
    xt, yt, zt = bit(7) << 2 | bit(4) << 1 | bit(1), bit(6) << 2 | bit(3) << 1 | bit(0), bit(5) << 1 | bit(2)
    q = np.empty((count, 3), np.int64)
    q[:, 0] = xt * 128 + rng.randint(0, 128, count)
    q[:, 1] = yt * 128 + rng.randint(0, 128, count)
    q[:, 2] = zt * 256 + rng.randint(0, 256, count)
    return q


def _rows_of_cells(q, dtype=np.float32):
    """Rows at the centres of grid cells, for a scene whose box is [0, 1]^3 (the callers put the two corners in)."""
    rows = np.zeros((len(q), 4), dtype)
    rows[:, :3] = (q + 0.5) / 1023.0
    rows[:, 3] = 12345.0                # lane w is ignored
    return rows


def _with_corners(rows):
    rows[0, :3], rows[1, :3] = 0.0, 1.0     # buckets 0 and 255
    return rows


def _uniform(n, seed=5, dtype=np.float32):
    rng = np.random.RandomState(seed)
    rows = np.zeros((n, 4), dtype)
    rows[:, :3] = rng.random_sample((n, 3))
    rows[:, 3] = 12345.0
    return rows


def _codes(oracle, rows):
    return oracle.morton(rows, oracle.bounds(rows))


def _expected(oracle, rows, padded):
    codes = np.full(padded, 0xFFFFFFFF, np.uint32)
    codes[:len(rows)] = _codes(oracle, rows)
    order = np.argsort(codes, kind="stable").astype(np.uint32)
    return codes[order], order


class _Path:
    """Buffers of a Collider with room for `bound` spheres and their pads, driven through the C ABI with any n <= bound."""

    def __init__(self, ctx, cq, bound, dtype=np.float32):
        self.ctx, self.cq, self.bound, self.dtype = ctx, cq, bound, np.dtype(dtype)
        self.col = Collider(ctx, bound + 16, 8, 8, coord_dtype=self.dtype)
        assert self.col.padded_size >= bound + PADS
        self.col._allocate()
        self.count = hip.Buffer(ctx, 4)
        word = C.c_void_p()
        call.col_host_alloc(C.byref(word), 64)
        self.word = word.value
        self.zeros = upload(ctx, np.zeros(bound, self.dtype))        # radii: empty boxes, no pairs

    def close(self):
        call.col_host_free(self.word)

    def oversize(self):
        return C.c_uint32.from_address(self.word).value

    def run(self, rows, entry="plan", bound=None):
        """entry: "plan" (bounds stage 1 inside the call), "partials" (host-known n), "dev" (n on the device, `bound` rows)."""
        col, cq = self.col, self.cq
        n = len(rows)
        for k in range(3):
            C.c_uint32.from_address(self.word + 4 * k).value = 0
        size = n if bound is None else bound
        padded = size + PADS
        held = np.full((size, 4), 7.0, self.dtype)
        held[:n] = rows
        rb = upload(self.ctx, held)
        cb = self.dtype.itemsize
        args = [cq.stream, rb.ptr, self.zeros.ptr, size, padded, cb, col._codes_bufs[0].ptr, col._codes_bufs[1].ptr,
                col._ids_bufs[0].ptr, col._ids_bufs[1].ptr, col._nodes_buf.ptr, col._bounds_buf.ptr, None,
                col._alloc["scratch"].ptr, self.count.ptr, None, 0, MSD, self.word]
        if entry == "plan":
            call.col_collide_plan(*args)
        else:
            nword = upload(self.ctx, np.array([n], np.uint32))
            partials, parts = hip.Buffer(self.ctx, 256 * 8 * cb), C.c_uint32(0)
            call.col_minmax4_stage1_dev(cq.stream, rb.ptr, nword.ptr, size, cb, partials.ptr, C.byref(parts))
            if entry == "partials":
                call.col_collide_plan_partials(*args, partials.ptr, parts.value)
            else:
                call.col_collide_plan_dev(*args, partials.ptr, parts.value, nword.ptr)
        cq.finish()
        return download(cq, col._codes_bufs[1], np.uint32, padded), download(cq, col._ids_bufs[1], np.uint32, padded)


@pytest.fixture()
def path(hip_env):
    made = []

    def make(bound, dtype=np.float32):
        made.append(_Path(*hip_env, bound, dtype))
        return made[-1]
    yield make
    for p in made:
        p.close()


def _check(oracle, p, rows, entry="plan", bound=None):
    codes, ids = p.run(rows, entry, bound)
    want_codes, want_ids = _expected(oracle, rows, (len(rows) if bound is None else bound) + PADS)
    np.testing.assert_array_equal(codes, want_codes)
    np.testing.assert_array_equal(ids, want_ids)


# ---- tile counts: n = tiles * 1024 - 7, padded = tiles * 1024 - 4; 768 is the most 1024-code tiles, 1024 of them (padded just
# ---- below 1 Mi, the end of the class) are 256 tiles of 4096 codes ----
@pytest.mark.parametrize("tiles", [1, 2, 3, 33, 65, 768, 1024])
def test_tile_counts(hip_env, oracle, path, tiles):
    n = tiles * TILE - 7
    p = path(n)
    _check(oracle, p, _uniform(n))
    assert p.oversize() == 0


def test_the_first_sizes_with_big_tiles(hip_env, oracle, path):
    """padded = 768 Ki exactly: 192 whole tiles of 4096 codes, the last pads in a full tile; then 193 tiles, the last ragged."""
    for n in (BIG_FROM - PADS, BIG_N):
        p = path(n)
        _check(oracle, p, _uniform(n))
        assert p.oversize() == 0


# ---- input order ----
@pytest.mark.parametrize("n", [300 * TILE - 7, BIG_N])
def test_input_already_sorted_by_code(hip_env, oracle, path, n):
    """Buckets of ~1200 / ~3100 pairs that come as one or two pieces of up to a whole tile: the wave copies."""
    tile = _tile_of(n + PADS)
    rows = _uniform(n)
    codes = _codes(oracle, rows)
    rows = rows[np.argsort(codes, kind="stable")]
    d = _digit(_codes(oracle, rows))
    assert (np.diff(d.astype(np.int64)) >= 0).all()
    per_tile = [np.bincount(d[t * tile:(t + 1) * tile], minlength=256).max() for t in range(n // tile)]
    assert max(per_tile) >= min(tile, 3000)            # some tile lies (all but) inside one bucket
    p = path(n)
    _check(oracle, p, rows)
    assert p.oversize() == 0


def test_input_reverse_sorted(hip_env, oracle, path):
    n = 33 * TILE - 7
    rows = _uniform(n)
    rows = rows[np.argsort(_codes(oracle, rows), kind="stable")[::-1]]
    p = path(n)
    _check(oracle, p, rows)
    assert p.oversize() == 0


def test_one_octant_leaves_digits_empty(hip_env, oracle, path):
    n = 33 * TILE - 7
    rows = _uniform(n)
    rows[:, :3] *= 0.5
    _with_corners(rows)
    assert len(np.unique(_digit(_codes(oracle, rows)))) < 64
    p = path(n)
    _check(oracle, p, rows)
    assert p.oversize() == 0


@pytest.mark.parametrize("n", [3 * TILE - 7, 600 * TILE - 7, BIG_N])      # 16 lanes per tile, one lane, four lanes (4096-code tiles)
def test_one_piece_one_pair_above_the_lane_limit(hip_env, oracle, path, n):
    """Every (tile, bucket) piece has at most _piece(tiles) pairs, but one: tile 1 holds one pair more of bucket 37."""
    rng = np.random.RandomState(11)
    tile = _tile_of(n + PADS)
    tiles = -(-(n + PADS) // tile)
    limit = _piece(tiles)
    assert limit == {3: 253, 600: 13, 193: 61}[tiles]
    digit = 40 + (np.arange(n) % 200)                   # about 5 (20) pairs per tile and bucket
    for t, k in ((0, limit), (1, limit + 1), (2, 3)):
        digit[t * tile + 100:t * tile + 100 + k] = 37
    rows = _with_corners(_rows_of_cells(_cells_in_bucket(digit, n, rng)))
    d = _digit(_codes(oracle, rows))
    pieces = np.array([np.bincount(d[t * tile:(t + 1) * tile], minlength=256) for t in range(tiles)])
    assert pieces[1, 37] == limit + 1 and (pieces > limit).sum() == 1 and pieces[0, 37] == limit
    p = path(n)
    _check(oracle, p, rows)
    assert p.oversize() == 0


# ---- stability ----
def test_equal_codes_from_many_tiles_keep_their_order(hip_env, oracle, path):
    rng = np.random.RandomState(12)
    n = 20000
    points = np.concatenate([_cells_in_bucket(int(d), 2, rng) for d in rng.choice(256, 20, replace=False)])     # 40 points
    rows = _with_corners(_rows_of_cells(points[rng.randint(0, 40, n)]))
    p = path(n)
    codes, ids = p.run(rows)
    want_codes, want_ids = _expected(oracle, rows, n + PADS)
    assert len(np.unique(want_codes)) <= 43
    np.testing.assert_array_equal(codes, want_codes)
    same = codes[1:] == codes[:-1]
    assert (ids[1:][same] > ids[:-1][same]).all()       # ids inside each run ascend
    np.testing.assert_array_equal(ids, want_ids)


# ---- the capacity edge ----
def _one_big_bucket(oracle, big, total=20 * TILE - 7, seed=13):
    """`big` pairs in bucket 100 (shuffled over all tiles), 3000 in bucket 101, the corners, and a uniform rest."""
    rng = np.random.RandomState(seed)
    rest = _uniform(total - big - 3000, seed)
    rest = rest[~np.isin(_digit(_codes(oracle, _with_corners(rest.copy()))), (100, 101))]
    rows = np.concatenate([rest[:2], _rows_of_cells(_cells_in_bucket(100, big, rng)),
                           _rows_of_cells(_cells_in_bucket(101, 3000, rng)), rest[2:]])
    body = rows[2:]
    body[:] = body[rng.permutation(len(body))]
    _with_corners(rows)
    sizes = np.bincount(_digit(_codes(oracle, rows)), minlength=256)
    assert sizes[100] == big and sizes[101] == 3000
    assert _tile_of(len(rows) + PADS) == _tile_of(total)
    return rows


@pytest.mark.parametrize("total", [20 * TILE - 7, BIG_N + 2 * BIG_TILE])
def test_a_bucket_of_exactly_the_capacity_fits(hip_env, oracle, path, total):
    rows = _one_big_bucket(oracle, CAP, total)
    p = path(len(rows))
    _check(oracle, p, rows)
    assert p.oversize() == 0


@pytest.mark.parametrize("total", [20 * TILE - 7, BIG_N + 2 * BIG_TILE])
def test_a_bucket_one_pair_above_the_capacity_is_sorted_and_reported(hip_env, oracle, path, total):
    rows = _one_big_bucket(oracle, CAP + 1, total)
    p = path(len(rows))
    _check(oracle, p, rows)
    assert p.oversize() == CAP + 1


def test_all_spheres_at_one_point(hip_env, oracle, path):
    n = 33 * TILE - 7                   # all in bucket 0
    rows = np.zeros((n, 4), np.float32)
    rows[:, :3] = 0.25
    p = path(n)
    _check(oracle, p, rows)
    assert p.oversize() == n


def test_the_slow_path_leaves_the_other_buckets_alone(hip_env, oracle, path):
    """20 000 spheres at one point of bucket 100 take the slow path while bucket 101 (5000 pairs) is gathered beside it."""
    rng = np.random.RandomState(14)
    q = np.concatenate([np.repeat(_cells_in_bucket(100, 1, rng), 20000, axis=0), _cells_in_bucket(101, 5000, rng),
                        _cells_in_bucket(99, 700, rng)])
    rows = _rows_of_cells(q[rng.permutation(len(q))])
    rows = _with_corners(np.concatenate([rows[:2], rows]))
    p = path(len(rows))
    _check(oracle, p, rows)
    assert p.oversize() == np.bincount(_digit(_codes(oracle, rows)), minlength=256)[100] >= 20000


# ---- the count on the device ----
@pytest.mark.parametrize("n", [40000, 40 * TILE, 1])
def test_count_on_the_device(hip_env, oracle, path, n):
    """n_dev in the middle of a tile, at a tile boundary, and one sphere: the rows from n on are pads in the order of their ids."""
    bound = 65 * TILE - 7
    p = path(bound)
    _check(oracle, p, _uniform(n), "dev", bound)
    assert p.oversize() == 0


def test_count_on_the_device_in_the_middle_of_a_big_tile(hip_env, oracle, path):
    p = path(BIG_N)
    _check(oracle, p, _uniform(500000), "dev", BIG_N)
    assert p.oversize() == 0
    _check(oracle, p, _uniform(2 * TILE - 7, seed=8))            # ... and a small scene on the scratch the 193 big tiles used
    _check(oracle, p, _uniform(BIG_N, seed=9), entry="partials")


def test_one_sphere(hip_env, oracle, path):
    p = path(1)
    _check(oracle, p, _uniform(1))
    assert p.oversize() == 0


def test_more_pads_than_a_bucket_holds(hip_env, oracle, path):
    bound, n = 65 * TILE - 7, 3000          # 63 k pads: written by formula, in nobody's bucket
    assert bound - n > CAP
    p = path(bound)
    _check(oracle, p, _uniform(n), "dev", bound)
    assert p.oversize() == 0


def test_a_smaller_scene_on_the_same_scratch(hip_env, oracle, path):
    """Stale table words or group sums of the first scene would misplace the second."""
    p = path(65 * TILE - 7)
    _check(oracle, p, _uniform(65 * TILE - 7))
    octant = _uniform(31 * TILE - 7, seed=6)
    octant[:, :3] *= 0.5
    _check(oracle, p, _with_corners(octant))
    _check(oracle, p, _uniform(40 * TILE - 7, seed=7), entry="partials")
    _check(oracle, p, _uniform(2 * TILE - 7, seed=8))
    _check(oracle, p, _uniform(500, seed=9), "dev", 3 * TILE - 7)


# ---- float64 coordinates ----
@pytest.mark.parametrize("n", [33 * TILE - 7, BIG_N])
def test_float64_coordinates(hip_env, oracle, path, n):
    p = path(n, np.float64)
    _check(oracle, p, _uniform(n, dtype=np.float64))
    assert p.oversize() == 0


# ---- the production path ----
def test_collider_pairs_at_100k(hip_env, oracle):
    ctx, cq = hip_env
    n, cap = 100000, 1 << 20
    rng = np.random.RandomState(15)
    coords = np.zeros((n, 4), np.float32)
    coords[:, :3] = rng.random_sample((n, 3))
    radii = np.full(n, 0.004, np.float32)
    collider = Collider(ctx, n, 8, 128)
    collider.sort_plan = "msd"
    ref = oracle.collide(coords, radii, padded=collider.padded_size, capacity=cap)
    cbuf, rbuf = hip.Buffer(ctx, hostbuf=coords), hip.Buffer(ctx, hostbuf=radii)
    nbuf, pbuf = hip.Buffer(ctx, 4), hip.Buffer(ctx, cap * 8)
    e = collider.get_collisions(cq, cbuf, rbuf, nbuf, pbuf, cap)
    count = int(hip.read_buffer(cq, nbuf, np.uint32, 1, wait_for=[e])[0])
    assert 0 < count == ref["count"] <= cap
    pairs = hip.read_buffer(cq, pbuf, np.uint32, (count, 2))
    codes = hip.read_buffer(cq, collider._codes_bufs[1], np.uint32, collider.padded_size)
    np.testing.assert_array_equal(codes, ref["codes"])
    key = lambda a: np.unique(a[:, 0].astype(np.uint64) << np.uint64(32) | a[:, 1].astype(np.uint64))
    got, want = key(pairs), key(ref["pairs"][:ref["count"]])
    assert len(got) == count
    np.testing.assert_array_equal(got, want)
    assert collider.oversize_bucket == 0
