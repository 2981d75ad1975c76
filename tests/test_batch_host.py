"""The batched collider's host side (col_collide_batch, BatchCollider): limits, scratch arithmetic, argument validation and
the ValueError contract.  No GPU needed: every call here returns before any HIP call."""
import itertools

import numpy as np
import pytest

from collision_amd import _lib, hip
from collision_amd.collision import BatchCollider

EINVAL = -1
P = 0x1000                       # a non-NULL pointer value; never dereferenced: the calls below return before any HIP call


@pytest.fixture(scope="module")
def ctx():
    return hip.Context()


def test_version_and_limits():
    c = _lib.call
    assert c.col_version() >= 103
    assert c.col_collide_batch_max_scene(4) >= 1024
    assert c.col_collide_batch_max_scene(8) >= 512
    for cb in (0, 1, 2, 3, 5, 16, -4):
        assert c.col_collide_batch_max_scene(cb) == 0


@pytest.mark.parametrize("cb", [4, 8])
def test_scratch_bytes_is_monotone_in_every_size_argument(cb):
    f = _lib.call.col_collide_batch_scratch_bytes
    limit = _lib.call.col_collide_batch_max_scene(cb)
    scenes = [1, 2, 63, 64, 1000, 4096, 1 << 20]
    totals = [1, 64, 65, 4096, 1 << 18, 1 << 24]
    sizes = sorted({1, 64, 65, 256, 257, 512, limit})
    for t, m in itertools.product(totals, sizes):
        v = [f(s, t, m, cb) for s in scenes]
        assert v == sorted(v)
    for s, m in itertools.product(scenes, sizes):
        v = [f(s, t, m, cb) for t in totals]
        assert v == sorted(v)
    for s, t in itertools.product(scenes, totals):
        v = [f(s, t, m, cb) for m in sizes]
        assert v == sorted(v)


def _batch(stream=None, coords=P, radii=P, offsets=P, n_scenes=3, total=100, max_scene=64, cb=4, codes=None, ids=None,
           scratch=None, counter=P, counts=P, pairs=P, capacity=10):
    return _lib.cdll().col_collide_batch(stream, coords, radii, offsets, n_scenes, total, max_scene, cb, codes, ids, scratch,
                                         counter, counts, pairs, capacity)


def test_einval_cases_return_before_any_hip_call():
    for cb in (0, 2, 3, 16):
        assert _batch(cb=cb) == EINVAL
    assert _batch(max_scene=0) == EINVAL
    for cb in (4, 8):
        limit = _lib.call.col_collide_batch_max_scene(cb)
        assert _batch(cb=cb, max_scene=limit + 1) == EINVAL
        assert _batch(cb=cb, max_scene=0xFFFFFFFF) == EINVAL
    assert _batch(pairs=None, capacity=1) == EINVAL
    assert _batch(counter=None) == EINVAL
    assert _batch(counts=None) == EINVAL
    assert _batch(offsets=None) == EINVAL
    # ... also with nothing to do: the arguments are checked first
    assert _batch(n_scenes=0, counter=None) == EINVAL
    assert _batch(n_scenes=0, cb=5) == EINVAL


def test_no_scenes_is_ok_and_launches_nothing():
    for cb in (4, 8):
        assert _batch(n_scenes=0, total=0, cb=cb) == 0
        assert _batch(n_scenes=0, total=0, cb=cb, pairs=None, capacity=0) == 0
        assert _batch(n_scenes=0, cb=cb, max_scene=_lib.call.col_collide_batch_max_scene(cb)) == 0


def test_batch_collider_value_errors(ctx):
    with pytest.raises(ValueError, match="Invalid dtype"):
        BatchCollider(ctx, 100, 3, 64, np.dtype("int32"))
    for dt in ("float32", "float64"):
        limit = _lib.call.col_collide_batch_max_scene(np.dtype(dt).itemsize)
        for bad in (0, -1, limit + 1):
            with pytest.raises(ValueError):
                BatchCollider(ctx, 100, 3, bad, dt)
        col = BatchCollider(ctx, 100, 3, limit, dt)
        assert (col.total_size, col.n_scenes, col.max_scene) == (100, 3, limit)
        with pytest.raises(ValueError):
            col.resize(max_scene=limit + 1)
        with pytest.raises(ValueError):
            col.resize(max_scene=0)
        assert col.max_scene == limit                       # a refused resize changes nothing
        col.resize(total_size=7, n_scenes=2, max_scene=5)
        assert (col.total_size, col.n_scenes, col.max_scene) == (7, 2, 5)
        with pytest.raises(ValueError, match="Invalid collisions_buf for n_collisions > 0"):
            col.get_collisions(None, None, None, None, None, None, None, 1)


def test_alias_module_exports_the_same_class():
    import collision.collision
    import collision_amd.collision
    assert collision.collision.BatchCollider is collision_amd.collision.BatchCollider
