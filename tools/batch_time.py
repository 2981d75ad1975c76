"""Batched collider against the two things a caller could do before it had one, per shape (scenes x spheres per scene)
and dtype -- one JSON line per leg:
  batch   one BatchCollider.get_collisions over all scenes;
  loop    Collider.get_collisions scene by scene over the same arrays (one collider, every scene its own counter and its
          own part of the pair list);
  single  one Collider call on ONE scene with the same total number of spheres: the floor for that many spheres.
Times are device events around a whole repetition (the loop's includes what the host cannot enqueue fast enough: that is
what the loop costs); median with min and max over --reps repetitions after --warmup.

The loop and the single scene run code the batched path does not touch: time them from a build of the commit before it,
    COLLISION_AMD_LIB=tools/ab/libcollision_hip_prev.so python tools/batch_time.py --legs loop,single
next to `python tools/batch_time.py` on the same box (tools/ab_builds.sh says how to make that build)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collision_amd import hip                                   # noqa: E402
from collision_amd._lib import call                             # noqa: E402
from collision_amd.collision import Collider                    # noqa: E402

SHAPES = [(1024, 256), (4096, 64), (256, 1024)]


def scenes(n_scenes, n, dt, seed=0):
    """n_scenes scenes of n spheres in the same unit cube: coords U[0,1)^3, radii U(0.2, 0.6) n^(-1/3) (~2 pairs per sphere)."""
    rs = np.random.RandomState(seed)
    coords = np.zeros((n_scenes * n, 4), dt)
    coords[:, :3] = rs.random_sample((n_scenes * n, 3))
    radii = (rs.uniform(0.2, 0.6, size=n_scenes * n) * n ** (-1.0 / 3.0)).astype(dt)
    return coords, radii


def timed(cq, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    cq.finish()
    ts = []
    for _ in range(reps):
        start, stop = hip.Event(), hip.Event()
        call.col_event_record(start.handle, cq.stream)
        fn()
        call.col_event_record(stop.handle, cq.stream)
        stop.wait()
        ts.append(start.elapsed_ms(stop))
    ts.sort()
    return dict(ms_median=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default="batch,loop,single")
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES), help="scenes x spheres per scene, comma separated")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    legs = args.legs.split(",")
    ctx = hip.Context()
    cq = hip.CommandQueue(ctx)
    tag = os.environ.get("COLLISION_AMD_LIB", "tree")[-32:]
    for shape in args.shapes.split(","):
        n_scenes, n = (int(v) for v in shape.split("x"))
        total = n_scenes * n
        for dt in (np.dtype(d) for d in args.dtypes.split(",")):
            coords, radii = scenes(n_scenes, n, dt)
            cbuf, rbuf = hip.Buffer(ctx, hostbuf=coords), hip.Buffer(ctx, hostbuf=radii)
            cap = 8 * total
            pairs_buf, counts_buf, n_buf = hip.Buffer(ctx, 8 * cap), hip.Buffer(ctx, 4 * n_scenes), hip.Buffer(ctx, 4)
            row = 4 * dt.itemsize
            base = dict(lib=tag, scenes=n_scenes, per_scene=n, dtype=dt.name, version=int(call.col_version()))

            def report(leg, t, pairs):
                print(json.dumps(dict(base, leg=leg, pairs=int(pairs), **{k: round(v, 5) for k, v in t.items()})), flush=True)

            if "batch" in legs:
                from collision_amd.collision import BatchCollider
                obuf = hip.Buffer(ctx, hostbuf=(np.arange(n_scenes + 1, dtype=np.uint64) * n).astype(np.uint32))
                bc = BatchCollider(ctx, total, n_scenes, n, dt)
                t = timed(cq, lambda: bc.get_collisions(cq, cbuf, rbuf, obuf, n_buf, counts_buf, pairs_buf, cap), args.reps, args.warmup)
                report("batch", t, hip.read_buffer(cq, n_buf, np.uint32, 1)[0])
            if "loop" in legs:
                col = Collider(ctx, n, 8, 64, coord_dtype=dt)
                per = cap // n_scenes
                views = [(hip.Buffer.from_ptr(ctx, cbuf.ptr + s * n * row, n * row), hip.Buffer.from_ptr(ctx, rbuf.ptr + s * n * dt.itemsize, n * dt.itemsize),
                          hip.Buffer.from_ptr(ctx, counts_buf.ptr + 4 * s, 4), hip.Buffer.from_ptr(ctx, pairs_buf.ptr + 8 * per * s, 8 * per))
                         for s in range(n_scenes)]

                def loop():
                    for c, r, k, p in views:
                        col.get_collisions(cq, c, r, k, p, per)
                t = timed(cq, loop, args.reps, args.warmup)
                report("loop", t, hip.read_buffer(cq, counts_buf, np.uint32, n_scenes).astype(np.uint64).sum())
                del col, views
            if "single" in legs:
                one_c, one_r = scenes(1, total, dt, seed=1)
                ocb, orb = hip.Buffer(ctx, hostbuf=one_c), hip.Buffer(ctx, hostbuf=one_r)
                col = Collider(ctx, total, 64, 256, coord_dtype=dt)
                t = timed(cq, lambda: col.get_collisions(cq, ocb, orb, n_buf, pairs_buf, cap), args.reps, args.warmup)
                report("single", t, hip.read_buffer(cq, n_buf, np.uint32, 1)[0])
                del col, ocb, orb


if __name__ == "__main__":
    main()
