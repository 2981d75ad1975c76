"""The scene zoo (tests/zoo.py) through the multi-GPU PROTOCOL on the CPU: LoopbackWorld with the NumPy/oracle engine double
(tests/dist_worker.py: OracleEngine), hash arrival, two steps, both partitions, both dtypes.  The double runs the protocol's own
slot layouts, splitters, octant regions and ghost hand-over, so this shows that the protocol is sound on these values -- and with
that, that oracle.brute_force on the whole scene is a valid reference for the real engines (tests/test_multi_zoo_world.py).

World 8 at n = 4099 for every case; world 4 at n = 1500 for the float64 Morton cases as well.  Three of the float64 Morton runs
-- range_overflow at 1500 / world 4, zero_and_giant and aniso at 4099 / world 8 -- hand the double a received slot of 0 or 1
records: `rec[:n, :8].contiguous()` copies nothing there, the odd storage offset of a 9-word record survives and
`.view(float64)` raised.  OracleEngine.unpack5 / ghost_queries copy for real now; these three cases fail without that.

slack = world + 1: range_overflow under Morton sends every sphere to the last rank (every code is 0, so is every splitter),
which must hold the whole scene.

Pair counts (= tests/test_oracle_zoo.py's, n = 4099, (f32, f64) where they differ): log_radii 10392, zero_and_giant 4105,
offset 7704 / 7744, neg_offset 11295 / 11300, aniso 41971, tiny 6503 / 6504, huge 6504, range_overflow 7021."""
import numpy as np
import pytest

from collision_amd.multi import LoopbackWorld, hash_owner
from tests.util import packed_pairs
from tests.zoo import DTYPES, FAMILIES, cached_scene

SIZES = [(8, 4099)]
CASES = [(f, dt, p, w, n) for f in FAMILIES for dt in DTYPES for p in ("morton", "hash") for w, n in SIZES]
CASES += [(f, "float64", "morton", 4, 1500) for f in FAMILIES]
_refs = {}


def rows_of(family, n, dt, seed=4):
    """The scene as (x, y, z, r) rows."""
    coords, radii = cached_scene(family, n, dt, seed)
    rows = np.zeros((n, 4), dt)
    rows[:, :3], rows[:, 3] = coords, radii
    return rows


def undirected(p):
    p = np.asarray(p, dtype=np.uint32).reshape(-1, 2)
    return packed_pairs(np.stack([p.min(axis=1), p.max(axis=1)], axis=1))


def brute_force_of(oracle, family, n, dt):
    """(count, sorted undirected pair keys) of oracle.brute_force on the whole scene; once per scene, read-only."""
    key = (family, n, np.dtype(dt).name)
    if key not in _refs:
        rows = rows_of(family, n, dt)
        cnt, ref = oracle.brute_force(rows, np.ascontiguousarray(rows[:, 3]))
        keys = undirected(ref)
        keys.setflags(write=False)
        _refs[key] = (cnt, keys)
    return _refs[key]


def load_by_hash(lw, rows, world):
    gids = np.arange(len(rows), dtype=np.uint32)
    owner = hash_owner(gids, world)
    for r in range(world):
        mine = owner == r
        lw.set_local_spheres(r, rows[mine], rows[mine, 3], gids[mine])
    return owner


def check_world(lw, oracle, family, n, dt):
    """Pair union == brute force, each pair once; the counter agrees; the owned sets partition the gids."""
    pairs = lw.pairs()
    cnt, want = brute_force_of(oracle, family, n, dt)
    got = undirected(np.concatenate(pairs))
    assert len(got) == cnt == lw.global_pair_count()
    assert (np.diff(got) != 0).all()
    np.testing.assert_array_equal(got, want)
    owned = np.concatenate([dc.own_gids[:dc.n_owned].cpu().numpy().view(np.uint32) for dc in lw.ranks])
    np.testing.assert_array_equal(np.sort(owned), np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("family,dt,partition,world,n", CASES)
def test_zoo_through_the_protocol(oracle, family, dt, partition, world, n):
    from tests.dist_worker import OracleEngine
    rows = rows_of(family, n, dt)
    owner = load_owner = hash_owner(np.arange(n, dtype=np.uint32), world)
    lw = LoopbackWorld(None, world, [int((owner == r).sum()) for r in range(world)],
                       engine=lambda cap: OracleEngine(cap, 1 << 22, np.dtype(dt)), group_size=64, pair_capacity=1 << 22,
                       partition=partition, coord_dtype=np.dtype(dt), slack=world + 1)
    assert (load_by_hash(lw, rows, world) == load_owner).all()
    for _ in range(2):
        lw.step()
    check_world(lw, oracle, family, n, dt)
    owned = [dc.n_owned for dc in lw.ranks]
    ghosts = [dc.stats["ghosts"] for dc in lw.ranks]
    # ---- the scenes do what they are here for
    if partition == "hash":
        assert all(g > 2 * m for g, m in zip(ghosts, owned)), (ghosts, owned)
    elif family == "range_overflow":             # every code 0, every splitter 0: the last rank owns the scene, nothing to exchange
        assert owned == [0] * (world - 1) + [n] and not any(ghosts)
    else:
        assert sum(g > 0 for g in ghosts) >= (6 if world == 8 else 3), ghosts
        if family == "zero_and_giant" and world == 8:      # the giant's handlers receive everyone: one rank, 2048 or more
            assert sum(g >= 2048 for g in ghosts) == 1, ghosts
