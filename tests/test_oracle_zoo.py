"""The CPU oracle on the scene zoo (tests/zoo.py).  The oracle is the reference of every GPU parity test, and until here it
was pinned against brute force on unit-cube, constant-radius scenes only.  For every family x dtype x n in {300, 4099}:

* the scene is what it is here for (the conditions below, so that no GPU test on it is vacuous);
* oracle.collide's pair set equals oracle.brute_force's and a NumPy restatement written here (lo = c - r, hi = c + r in the
  scene's dtype, strict inequalities), as unordered pairs; capacity n (n - 1) / 2, so no list is cut;
* pairs are oriented by sorted position; codes are sorted with ids increasing inside a run of equal codes; leaf boxes are
  c -+ r of their sphere and every internal box is exactly the min / max of its two children's.

And exact power-of-two scaling of log_radii changes nothing but the boxes, which scale exactly.

Oracle pair counts (seed 4), n = 300 / 4099 -- the same for both dtypes unless two are given (f32, f64):
  log_radii 803 / 10392; zero_and_giant 300 / 4105; offset 507, 518 / 7704, 7744; neg_offset 776 / 11295, 11300;
  aniso 856 / 41971; tiny 455 / 6503, 6504; huge 455 / 6504; range_overflow 201 / 7021."""
import numpy as np
import pytest

from tests.zoo import DTYPES, FAMILIES, cached_scene

SIZES = [300, 4099]
COUNTS = {   # family: {n: (f32, f64)}, measured with this oracle; the conditions below do not depend on them
    "log_radii": {300: (803, 803), 4099: (10392, 10392)}, "zero_and_giant": {300: (300, 300), 4099: (4105, 4105)},
    "offset": {300: (507, 518), 4099: (7704, 7744)}, "neg_offset": {300: (776, 776), 4099: (11295, 11300)},
    "aniso": {300: (856, 856), 4099: (41971, 41971)}, "tiny": {300: (455, 455), 4099: (6503, 6504)},
    "huge": {300: (455, 455), 4099: (6504, 6504)}, "range_overflow": {300: (201, 201), 4099: (7021, 7021)},
}


def _unordered(pairs):
    p = np.sort(np.asarray(pairs, dtype=np.uint64).reshape(-1, 2), axis=1)
    return np.sort((p[:, 0] << np.uint64(32)) | p[:, 1])


def _numpy_pairs(coords, radii):
    """Every i < j whose boxes overlap strictly on all three axes, boxes computed in the scene's dtype."""
    lo, hi = coords - radii[:, None], coords + radii[:, None]
    assert lo.dtype == coords.dtype and hi.dtype == coords.dtype
    out = []
    for a in range(0, len(coords), 512):
        hit = np.ones((min(512, len(coords) - a), len(coords)), bool)
        for k in range(3):
            hit &= (hi[a:a + 512, None, k] > lo[None, :, k]) & (lo[a:a + 512, None, k] < hi[None, :, k])
        i, j = np.nonzero(hit)
        keep = i + a < j
        out.append(np.stack([i[keep] + a, j[keep]], axis=1))
    return np.concatenate(out)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_on_the_zoo(oracle, family, dtype, n):
    coords, radii = cached_scene(family, n, dtype)
    dt = np.dtype(dtype)
    assert coords.dtype == dt and radii.dtype == dt and coords.shape == (n, 3) and radii.shape == (n,)
    lo, hi = coords - radii[:, None], coords + radii[:, None]
    ref = oracle.collide(oracle.pad4(coords), radii, capacity=n * (n - 1) // 2)
    count, pairs, codes, ids, nodes, bounds = (ref[k] for k in ("count", "pairs", "codes", "ids", "nodes", "bounds"))

    # ---- the conditions on the inputs
    assert (radii >= 0).all() and np.isfinite(lo).all() and np.isfinite(hi).all()
    assert n / 2 <= count <= 16 * n, count
    if family == "tiny":
        tiny = np.finfo(dt).tiny
        assert ((lo != 0) & (np.abs(lo) < tiny)).sum() + ((hi != 0) & (np.abs(hi) < tiny)).sum() >= 3 * n
        assert (np.abs(hi) < tiny).all() and (np.abs(lo) < tiny).all()
    if family == "range_overflow":
        with np.errstate(over="ignore"):
            assert np.isinf(coords.max(axis=0) - coords.min(axis=0)).all()
        assert len(np.unique(codes[:n])) == 1 and codes[0] == 0
    if family == "zero_and_giant":
        g = int(np.argmax(radii))
        others = np.arange(n) != g
        assert (radii == 0).sum() > n * 0.98 and (lo[g] < lo[others]).all() and (hi[g] > hi[others]).all()
    if family == "offset" and dt == np.float32:
        assert len(np.unique(coords[:, 0])) < n                     # the 2^-11 grid: coordinates coincide exactly
    assert count == COUNTS[family][n][DTYPES.index(dtype)]          # (the figures of the docstring, kept honest)

    # ---- the pair set: brute force in C, brute force in NumPy
    bcount, bpairs = oracle.brute_force(oracle.pad4(coords), radii, capacity=n * (n - 1) // 2)
    assert bcount == count == len(pairs) == len(bpairs)
    got = _unordered(pairs)
    assert (np.diff(got) != 0).all()                                # each pair once
    np.testing.assert_array_equal(got, _unordered(bpairs))
    np.testing.assert_array_equal(got, _unordered(_numpy_pairs(coords, radii)))

    # ---- orientation, sort order, boxes
    pos = np.empty(n, np.int64)
    pos[ids[:n].astype(np.int64)] = np.arange(n)
    assert (np.sort(ids[:n]) == np.arange(n)).all()
    assert (pos[pairs[:, 0].astype(np.int64)] < pos[pairs[:, 1].astype(np.int64)]).all()
    assert (np.diff(codes[:n].astype(np.int64)) >= 0).all()
    eq = codes[1:n] == codes[:n - 1]
    assert (ids[1:n][eq] > ids[:n - 1][eq]).all()                   # the stable tie-break
    leaf = n - 1
    np.testing.assert_array_equal(nodes["data"][leaf:, 0], ids[:n])
    bits = np.uint32 if dt.itemsize == 4 else np.uint64
    np.testing.assert_array_equal(bounds[leaf:, 0, :3].view(bits), lo[ids[:n]].view(bits))
    np.testing.assert_array_equal(bounds[leaf:, 1, :3].view(bits), hi[ids[:n]].view(bits))
    kids = nodes["data"][:leaf].astype(np.int64)
    assert len(np.unique(kids)) == 2 * leaf and kids.min() == 1     # every node but the root is a child once
    np.testing.assert_array_equal(bounds[:leaf, 0, :3], np.minimum(bounds[kids[:, 0], 0, :3], bounds[kids[:, 1], 0, :3]))
    np.testing.assert_array_equal(bounds[:leaf, 1, :3], np.maximum(bounds[kids[:, 0], 1, :3], bounds[kids[:, 1], 1, :3]))


def test_tiny_loses_a_pair_to_subnormal_rounding(oracle):
    """tiny and huge are one scene at two scales; at f32 the subnormal grid (2^-149 under coordinates below 2^-130: 19 bits)
    rounds box edges together that the exact scaling keeps apart: a build that flushes subnormals, or rounds them
    differently, cannot give both counts."""
    n = 4099
    count = {}
    for family in ("tiny", "huge"):
        coords, radii = cached_scene(family, n, "float32")
        count[family] = oracle.collide(oracle.pad4(coords), radii, capacity=0, want=False)["count"]
    tiny, _ = cached_scene("tiny", n, "float32")
    huge, _ = cached_scene("huge", n, "float32")
    assert (tiny.astype(np.float64) * 2.0 ** 250 != huge).any()       # not an exact scaling of each other
    assert count["tiny"] == count["huge"] - 1 == COUNTS["tiny"][n][0]


@pytest.mark.parametrize("k", [-60, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_power_of_two_scaling_changes_only_the_boxes(oracle, dtype, k):
    n = 4099
    coords, radii = cached_scene("log_radii", n, dtype)
    f = np.asarray(2.0 ** k, dtype)
    sc, sr = coords * f, radii * f
    assert (sc / f == coords).all() and (sr / f == radii).all()      # exact: nothing left the normal range
    a = oracle.collide(oracle.pad4(coords), radii, capacity=n * (n - 1) // 2)
    b = oracle.collide(oracle.pad4(sc), sr, capacity=n * (n - 1) // 2)
    np.testing.assert_array_equal(a["codes"], b["codes"])
    np.testing.assert_array_equal(a["ids"], b["ids"])
    assert a["nodes"].tobytes() == b["nodes"].tobytes()
    assert a["count"] == b["count"]
    np.testing.assert_array_equal(_unordered(a["pairs"]), _unordered(b["pairs"]))
    np.testing.assert_array_equal(a["pairs"], b["pairs"])            # (the same walk: the same list, row for row)
    bits = np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64
    np.testing.assert_array_equal(b["bounds"][:, :, :3].view(bits), (a["bounds"][:, :, :3] * f).view(bits))
