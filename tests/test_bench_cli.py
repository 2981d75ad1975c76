"""bench.py's command line: the plain run prints the headline line alone, --dump-outputs files what the last
timed step returned, --full is where every other leg lives."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_dump_outputs_writes_the_pairs_in_a_fixed_order(tmp_path):
    import bench
    pairs = np.array([[7, 9], [2, 5], [7, 8], [0, 4000000000], [2, 3]], np.uint32)
    bench.dump_outputs(tmp_path / "a", 5, pairs)
    bench.dump_outputs(tmp_path / "b", 5, pairs[::-1])          # another append order, the same set
    got = np.load(tmp_path / "a" / "pairs.npy")
    assert got.dtype == np.float64 and got.shape == (5, 2)
    assert got.tolist() == [[0, 4000000000], [2, 3], [2, 5], [7, 8], [7, 9]]
    assert (got == np.load(tmp_path / "b" / "pairs.npy")).all()
    count = np.load(tmp_path / "a" / "count.npy")
    assert count.dtype == np.float64 and count.tolist() == [5]
    bench.dump_outputs(tmp_path / "a", 0, np.zeros((0, 2), np.uint32), "_rank1")
    assert np.load(tmp_path / "a" / "pairs_rank1.npy").shape == (0, 2)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_last_step(tmp_path):
    out = tmp_path / "dump"
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                           "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 1 and res["steps"] == 3 and res["warmup"] == 2
    assert res["unit"] == "M spheres/s" and res["higher_is_better"] is True and res["dtype"].startswith("f32")
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 1e6 / res["ms_per_step"] / 1e3) <= 0.01 * res["value"]        # 1 M spheres per step
    # nothing beside the headline ran
    assert res["roofline"] is None and res["cpu_baseline"] is None
    assert not {"radix_sort", "stage_ms", "count_only_ms", "config3_clustered", "config2_f64"} & set(res)
    # the files hold what get_collisions returned in the last timed step
    count = np.load(out / "count.npy")
    pairs = np.load(out / "pairs.npy")
    assert count.dtype == np.float64 and pairs.dtype == np.float64
    assert count.tolist() == [res["pairs_found"]] and res["pairs_found"] > 1000
    assert pairs.shape == (res["pairs_found"], 2)
    ids = pairs.astype(np.int64)
    assert (ids == pairs).all() and ids.min() >= 0 and ids.max() < 1000000 and (ids[:, 0] != ids[:, 1]).all()
    keys = ids[:, 0] * 1000000 + ids[:, 1]
    assert (np.diff(keys) > 0).all()                                                        # sorted, each pair once
