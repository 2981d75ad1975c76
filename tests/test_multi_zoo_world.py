"""The scene zoo (tests/zoo.py) through the WHOLE multi-GPU step with real engines: LoopbackWorld, four ranks with a
HipEngine each on the one GPU, n = 4099, hash arrival, both partitions, both dtypes, step / synchronize / step -- and once
more with COLLISION_GHOST_WALK=packets (the default takes the lane walk below 400 000 ghosts, so the packet walk would
otherwise never meet a zoo scene inside the protocol).  The reference is oracle.brute_force on the whole scene, which
tests/test_multi_zoo_cpu.py shows to be what the protocol gives on these scenes; every rank's sorted codes / ids / nodes /
boxes are the oracle's on what it owns (tests/dist_worker.py: per_rank_parity).

range_overflow under Morton: every code is 0, every splitter is 0, every row goes to the last owner: ranks 0-2 own NOTHING
after the repartition and run the step at a device-side count of 0 with the real halo branch behind it.  Read before this
ran -- why that is safe:
* every kernel that takes the count reads it through count_of(n, n_dev) = min(bound, *n_dev) (csrc/col_common.h);
* col_collide_plan_dev at a count of 0 is tests/test_pipeline_parity.py::test_count_on_the_device_gives_the_same_arrays's
  case (0, 5000): k_chunk's workgroups leave at `bid >= nb` / `k >= xcd_chunks(nb, ..)` with nb = 0 chunks, k_cross clamps
  its chunk count to 0, k_traverse returns at `n_dev && n < 2`; nothing is written, the counter stays 0;
* col_region_boxes_dev: k_region_part's row loop `i0 < n` never runs (so `rows[min(.., n - 1)]` is never formed), the
  partials stay +inf / -inf and k_region_fold writes eight inverted boxes (+inf - (-inf) = +inf): nothing overlaps them, so
  the rank that owns the scene selects nothing for these peers;
* col_select_overlap_multi_dev: k_select_multi leaves its row loop at `i >= n` for every thread, every mask is 0, the
  block total is 0 and `continue` (block-uniform) skips reservation and stores; col_pack_slots then writes headers of 0;
* col_traverse_ghost_slots_dev, lane walk: k_ghost reads a record only under `g < min(len, slot) && n > 0`, idx stays END
  and the loop is not entered (leaf_start = n - 1 wraps but is never used); packet walk: k_ghost_codes loads node 0's box
  and a record only under `g < cnt` (cnt = 0 here: every header is 0 -- and were it not, quantize() clamps whatever the
  stale box gives, NaN -> 0), the sort runs over 0xFFFF keys, and k_traverse<GHOST> returns at `n_dev && n < 1`.
So no path needed a guard added."""
import numpy as np
import pytest

from collision_amd.multi import LoopbackWorld, hash_owner
from tests.test_multi_zoo_cpu import check_world, load_by_hash, rows_of
from tests.zoo import DTYPES, FAMILIES

pytestmark = pytest.mark.gpu

WORLD, N = 4, 4099


@pytest.mark.parametrize("walk", ["auto", "packets"])
@pytest.mark.parametrize("partition", ["morton", "hash"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_zoo_through_the_whole_step(hip_env, oracle, monkeypatch, family, dt, partition, walk):
    from tests.dist_worker import per_rank_parity
    ctx, _ = hip_env
    if walk == "packets":
        monkeypatch.setenv("COLLISION_GHOST_WALK", "packets")
    else:
        monkeypatch.delenv("COLLISION_GHOST_WALK", raising=False)
    rows = rows_of(family, N, dt)
    owner = hash_owner(np.arange(N, dtype=np.uint32), WORLD)
    lw = LoopbackWorld(ctx, WORLD, [int((owner == r).sum()) for r in range(WORLD)], group_size=64, pair_capacity=1 << 20,
                       partition=partition, coord_dtype=np.dtype(dt), slack=5.0)
    assert all(bool(dc.engine.device_count) for dc in lw.ranks)
    load_by_hash(lw, rows, WORLD)
    lw.step()
    lw.synchronize()
    lw.step()
    check_world(lw, oracle, family, N, dt)          # pair union == brute force, each pair once; the owned sets partition the gids
    for dc in lw.ranks:
        assert per_rank_parity(dc) == "ok"
    owned = [dc.n_owned for dc in lw.ranks]
    ghosts = [dc.stats["ghosts"] for dc in lw.ranks]
    assert sum(owned) == N
    if partition == "hash":                         # a rank answers for everything its one or two peers own
        assert all(g >= min(owned) for g in ghosts), (ghosts, owned)
    elif family == "range_overflow":
        assert owned == [0, 0, 0, N] and not any(ghosts)
    else:
        assert min(owned) > N // 8 and sum(g > 0 for g in ghosts) >= 2, (owned, ghosts)
