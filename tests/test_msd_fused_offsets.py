"""The MSD plan inside col_collide_plan has no scan launch (csrc/radix.hip, k_scatter FUSED): the Morton kernel writes its
tile's digit counts and adds them into sums over groups of 32 tiles, and the one global pass adds up its own offsets from
them.  The sorted codes and ids must be np.argsort(kind="stable") of the oracle's codes, bit for bit, at every tile count
around the group size, in both tile classes, with empty digits, with one oversize bucket, on a scratch that another scene
has used, with the count on the device and through the partials entry (which clears the group sums with a memset)."""
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


def _scene(kind, n, seed=5):
    rng = np.random.RandomState(seed)
    rows = np.zeros((n, 4), np.float32)
    if kind == "uniform":
        rows[:, :3] = rng.random_sample((n, 3))
    elif kind == "octant":              # one octant of the scene's box, which two far corners span: most top digits stay empty
        rows[:, :3] = 0.5 * rng.random_sample((n, 3))
        rows[0, :3], rows[1, :3] = 0.0, 1.0
    else:                               # "point": every code equal, one bucket holds them all
        rows[:, :3] = 0.25
    rows[:, 3] = 12345.0                # lane w is ignored
    return rows


def _expected(oracle, rows, padded):
    codes = np.full(padded, 0xFFFFFFFF, np.uint32)
    codes[:len(rows)] = oracle.morton(rows, oracle.bounds(rows))
    order = np.argsort(codes, kind="stable").astype(np.uint32)
    return codes[order], order


class _Path:
    """Buffers of a Collider sized for `bound` spheres, driven through the C ABI with any n <= bound."""

    def __init__(self, ctx, cq, bound):
        self.ctx, self.cq, self.bound = ctx, cq, bound
        self.col = Collider(ctx, bound, 8, 8)            # padded_size = bound rounded up to 16 >= bound + PADS for bound = 16 k + 1 or 16 k + 9
        assert self.col.padded_size >= bound + PADS
        self.col._allocate()
        self.count = hip.Buffer(ctx, 4)
        word = C.c_void_p()
        call.col_host_alloc(C.byref(word), 64)
        self.word = word.value
        self.zeros = upload(ctx, np.zeros(bound, np.float32))        # radii: empty boxes, no pairs

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
        held = np.full((size, 4), 7.0, np.float32)
        held[:n] = rows
        rb = upload(self.ctx, held)
        args = [cq.stream, rb.ptr, self.zeros.ptr, size, padded, 4, col._codes_bufs[0].ptr, col._codes_bufs[1].ptr,
                col._ids_bufs[0].ptr, col._ids_bufs[1].ptr, col._nodes_buf.ptr, col._bounds_buf.ptr, None,
                col._alloc["scratch"].ptr, self.count.ptr, None, 0, MSD, self.word]
        if entry == "plan":
            call.col_collide_plan(*args)
        else:
            nword = upload(self.ctx, np.array([n], np.uint32))
            partials, parts = hip.Buffer(self.ctx, 256 * 8 * 4), C.c_uint32(0)
            call.col_minmax4_stage1_dev(cq.stream, rb.ptr, nword.ptr, size, 4, partials.ptr, C.byref(parts))
            if entry == "partials":
                call.col_collide_plan_partials(*args, partials.ptr, parts.value)
            else:
                call.col_collide_plan_dev(*args, partials.ptr, parts.value, nword.ptr)
        cq.finish()
        return download(cq, col._codes_bufs[1], np.uint32, padded), download(cq, col._ids_bufs[1], np.uint32, padded)


@pytest.fixture()
def path(hip_env):
    made = []

    def make(bound):
        made.append(_Path(*hip_env, bound))
        return made[-1]
    yield make
    for p in made:
        p.close()


def _check(oracle, p, rows, entry="plan"):
    codes, ids = p.run(rows, entry)
    want_codes, want_ids = _expected(oracle, rows, len(rows) + PADS)
    np.testing.assert_array_equal(codes, want_codes)
    np.testing.assert_array_equal(ids, want_ids)


# 1024-pair tiles (below 1 Mi): tile counts around the group of 32 tiles and two groups; padded = tiles * 1024 - 4
@pytest.mark.parametrize("kind,tiles", [("uniform", 1), ("uniform", 2), ("uniform", 31), ("uniform", 32), ("uniform", 33),
                                        ("uniform", 64), ("uniform", 65), ("octant", 33), ("octant", 65), ("point", 2)])
def test_small_tile_counts(hip_env, oracle, path, kind, tiles):
    n = tiles * 1024 - 7
    p = path(n)
    _check(oracle, p, _scene(kind, n))
    assert p.oversize() == 0


def test_one_oversize_bucket_is_sorted_and_reported(hip_env, oracle, path):
    n = 33 * 1024 - 7                   # all in bucket 0: more than the 8192 pairs of the LDS finish
    p = path(n)
    _check(oracle, p, _scene("point", n))
    assert p.oversize() == n


# 4096-pair tiles: just above 1 Mi (257 tiles, the last one ragged) and 2.0 M (489 tiles, the 16384-pair bucket finish)
@pytest.mark.parametrize("n", [(1 << 20) + 97, 2000001])
def test_big_tile_class(hip_env, oracle, path, n):
    p = path(n)
    _check(oracle, p, _scene("uniform", n))
    assert p.oversize() == 0


def test_a_smaller_scene_on_the_same_scratch(hip_env, oracle, path):
    """Stale group sums or bucket starts of the first scene would misplace the second."""
    p = path(65 * 1024 - 7)
    _check(oracle, p, _scene("uniform", 65 * 1024 - 7))
    _check(oracle, p, _scene("octant", 31 * 1024 - 7, seed=6))
    _check(oracle, p, _scene("uniform", 40 * 1024 - 7, seed=7), entry="partials")
    _check(oracle, p, _scene("uniform", 2 * 1024 - 7, seed=8))


def test_count_on_the_device(hip_env, oracle, path):
    """n_dev below the bound: the rows from n on are pads behind bucket 255's codes, in the order of their ids."""
    bound, n = 65 * 1024 - 7, 40000
    p = path(bound)
    rows = _scene("uniform", n)
    codes, ids = p.run(rows, "dev", bound)
    want_codes, want_ids = _expected(oracle, rows, bound + PADS)
    np.testing.assert_array_equal(codes, want_codes)
    np.testing.assert_array_equal(ids, want_ids)


def test_partials_entry(hip_env, oracle, path):
    n = 33 * 1024 - 7
    p = path(n)
    _check(oracle, p, _scene("uniform", n), entry="partials")
