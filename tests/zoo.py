"""The scene zoo: fixed-seed scenes whose VALUES are the edge cases -- radii over five decades, empty boxes, large offsets,
coordinates that coincide, subnormal and near-overflow scales, a scene whose range overflows.  A plain helper module: the
CPU tests pin the oracle on these scenes (tests/test_oracle_zoo.py), the GPU tests run them through every variant of the path
(tests/test_scene_zoo.py) and through the multi-GPU step -- the protocol on the CPU double (tests/test_multi_zoo_cpu.py), the
device steps of csrc/multi.hip one by one (tests/test_multi_zoo.py: rows (x, y, z, r); seed 5 gives a family's "other" rank) and
the whole step with real engines (tests/test_multi_zoo_world.py) --, tools/fuzz_parity.py draws from the same definitions.

scene(family, n, dtype, seed=4) -> (coords[n, 3], radii[n]).  Everything is drawn from one np.random.RandomState(seed) in
float64 -- u ~ U[0,1)^3 first, then the radii -- and cast to `dtype` at the end.  s = n^(-1/3) is the mean spacing of u.

  log_radii       u, r = s * 10^U(-4, 0.3): five decades, a few giants that overlap hundreds of spheres
  zero_and_giant  u, r = 0 except every 97th (0, 97, ...) = 0.3 s and sphere n // 2 with r = 2, which contains the scene: an
                  empty box pairs with nobody except a box that strictly contains its point
  offset          f32: 4096 + u (a 2^-11 grid: many coordinates coincide exactly), f64: 2^40 + u; r = 0.4 s
  neg_offset      -1000 + 3 u, r ~ U(0, 2.4 s)
  aniso           u * (1e3, 1, 1e-3); r = U(0.2, 1.8) * 80 / sqrt(n): the boxes are cubes, so every box spans the whole z
                  range and most of y -- the pairs are decided on the long axis, the codes on all three.  The densest
                  family (5 n pairs at n = 1024, 10 n at 4099): the one that overflows col_collide_batch's staged list
  tiny            u * 2^-130 (f32) / u * 2^-1040 (f64), r = U(0.1, 0.6) * s * the same factor: every box edge is subnormal
  huge            the same scene scaled by 2^120 / 2^1000 instead
  range_overflow  (2 u - 1) * 0.9 * finfo.max: max - min overflows to inf, every Morton code is 0;
                  r = U(0.7, 1) * min(0.81 s, 0.09) * finfo.max (0.81 s = 0.45 spacings of the 1.8 max wide scene; the cap
                  keeps |c| + r <= 0.99 finfo.max at every n)
"""
import numpy as np

FAMILIES = ["log_radii", "zero_and_giant", "offset", "neg_offset", "aniso", "tiny", "huge", "range_overflow"]
DTYPES = ["float32", "float64"]


def scene(family, n, dtype, seed=4):
    dtype = np.dtype(dtype)
    f32 = dtype == np.float32
    rng = np.random.RandomState(seed)
    u = rng.random_sample((n, 3))
    s = max(n, 1) ** (-1.0 / 3.0)
    if family == "log_radii":
        coords, radii = u, s * 10.0 ** rng.uniform(-4, 0.3, size=n)
    elif family == "zero_and_giant":
        coords, radii = u, np.zeros(n)
        radii[::97] = 0.3 * s
        radii[n // 2:n // 2 + 1] = 2.0
    elif family == "offset":
        coords, radii = (4096.0 if f32 else 2.0 ** 40) + u, np.full(n, 0.4 * s)
    elif family == "neg_offset":
        coords, radii = -1000.0 + 3.0 * u, rng.uniform(0, 2.4 * s, size=n)
    elif family == "aniso":
        coords, radii = u * np.array([1e3, 1.0, 1e-3]), rng.uniform(0.2, 1.8, size=n) * 80.0 / np.sqrt(max(n, 1))
    elif family in ("tiny", "huge"):
        k = {("tiny", True): -130, ("tiny", False): -1040, ("huge", True): 120, ("huge", False): 1000}[family, f32]
        coords, radii = np.ldexp(u, k), np.ldexp(rng.uniform(0.1, 0.6, size=n) * s, k)
    elif family == "range_overflow":
        top = float(np.finfo(dtype).max)
        coords, radii = (2.0 * u - 1.0) * 0.9 * top, rng.uniform(0.7, 1.0, size=n) * min(0.81 * s, 0.09) * top
    else:
        raise ValueError(family)
    return coords.astype(dtype), radii.astype(dtype)


_cache = {}


def cached_scene(family, n, dtype, seed=4):
    """scene(), computed once per argument tuple and handed out read-only."""
    key = (family, n, np.dtype(dtype).name, seed)
    if key not in _cache:
        coords, radii = scene(family, n, dtype, seed)
        coords.setflags(write=False)
        radii.setflags(write=False)
        _cache[key] = (coords, radii)
    return _cache[key]
