"""Timing of the device rollout (mnav_follow_rollout) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the resident
vector maps of a 7 168-plan Dijkstra batch, set up as tools/follow_perf.py does: `--ticks` controller ticks of 1, 1 024,
14 336 and 1 048 576 robots (robot i on plan i mod 7 168) in the "stay" and "mixed" mixes of follow_perf, two ways:

  (a) one mnav_follow_rollout call: wall clock around the call (it ends in a stream synchronise; inputs up, every output
      down) and the device time of its kernels (HIP events around each block of ticks);
  (b) the only way to do this without it: `--ticks` mnav_follow_batch calls with the unicycle advanced on the host between
      them (numpy, vectorised over the robots, in double); the time inside the calls is kept apart from the whole loop.

(a) and (b) alternate, medians of `--reps` repetitions after `--warmup` of each shape, with the spread of the repeats, the
per-tick figures and the share of idle lanes at the last tick (robots that had stopped: compaction is not done).

    python tools/rollout_perf.py [--reps K] [--ticks T] [--sizes a,b,c] [--plans N] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from follow_perf import make_robots  # noqa: E402
from mesh_navigation_amd import capi, meshgen  # noqa: E402


def rollout_once(ctx, r, cfg, ro):
    t0 = time.perf_counter()
    out = ctx.rollout(r["pos"], r["dir"], r["up"], r["face_in"], r["slot"], config=cfg, rollout=ro)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, ctx.rollout_stats(), out


def loop_once(ctx, r, cfg, ticks, dt):
    """the loop of one-tick calls: returns (ms of the whole loop, ms inside the calls, ms of their kernels, robots still OK)"""
    pos, d, face = r["pos"].copy(), r["dir"].astype(np.float64), r["face_in"].copy()
    up = r["up"].astype(np.float64)
    alive = np.ones(pos.shape[0], bool)
    calls = kern = 0.0
    t_loop = time.perf_counter()
    for _ in range(ticks):
        t0 = time.perf_counter()
        o = ctx.follow(pos, d.astype(np.float32), r["up"], face, r["slot"], config=cfg, outputs=("code", "face", "pos", "cmd"))
        calls += (time.perf_counter() - t0) * 1e3
        kern += ctx.follow_stats()["ms_kernels"]
        alive &= o.code == capi.FOLLOW_OK                              # a robot that lost the map or the field stops (its row is still sent)
        step = np.where(alive, o.cmd[:, 0], 0.0) * dt
        th = np.where(alive, o.cmd[:, 1], 0.0) * dt
        pos = np.where(alive[:, None], o.pos.astype(np.float64) + d * step[:, None], pos).astype(np.float32)
        face = np.where(alive, o.face, face).astype(np.uint32)
        c, s = np.cos(th)[:, None], np.sin(th)[:, None]
        nd = d * c + np.cross(up, d) * s + up * ((up * d).sum(axis=1, keepdims=True) * (1.0 - c))
        d = nd / np.linalg.norm(nd, axis=1, keepdims=True)
    return (time.perf_counter() - t_loop) * 1e3, calls, kern, int(alive.sum())


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,1024,14336,1048576")
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    sizes = [int(s) for s in args.sizes.split(",")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=args.plans, reps=args.reps, warmup=args.warmup, ticks=args.ticks, dt=args.dt, shapes={})
    cfg = capi.FollowConfig()
    ro = capi.RolloutConfig(dt=args.dt, ticks=args.ticks)
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(5)
        seeds = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        targets = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        r = ctx.plan_dijkstra_batch(seeds, targets, path_cap=4096, want_stats=False)
        res["plan_codes"] = sorted(set(int(c) for c in r["codes"]))
        res["resident_field_bytes"] = 12 * mesh.V * args.plans
        res["engine"] = ctx.last_engine()
        del r
        ctx.locate(mesh.xyz[:8])                                          # the lookup index exists before anything is timed
        for n in sizes:
            for mix in ("stay", "mixed"):
                rb = make_robots(mesh, targets, n, args.plans, mix, 10 + n)
                a_wall, a_kern, b_loop, b_calls, b_kern = [], [], [], [], []
                for rep in range(args.warmup + args.reps):
                    wall, st, out = rollout_once(ctx, rb, cfg, ro)
                    loop, calls, kern, ok = loop_once(ctx, rb, cfg, args.ticks, args.dt)
                    if rep >= args.warmup:
                        a_wall.append(wall); a_kern.append(st["ms_kernels"]); b_loop.append(loop); b_calls.append(calls); b_kern.append(kern)
                a, b = stats(a_wall), stats(b_loop)
                spread = max(a["max"] - a["min"], b["max"] - b["min"])
                res["shapes"]["%d_%s" % (n, mix)] = dict(
                    rollout_ms_call_wall=a, rollout_ms_kernels=stats(a_kern), loop_ms_wall=b, loop_ms_in_calls=stats(b_calls), loop_ms_kernels=stats(b_kern),
                    rollout_ms_per_tick_wall=a["median"] / args.ticks, rollout_ms_per_tick_kernels=float(np.median(a_kern)) / args.ticks,
                    loop_ms_per_tick_kernels=float(np.median(b_kern)) / args.ticks, loop_ms_per_tick_in_calls=float(np.median(b_calls)) / args.ticks,
                    speedup_vs_loop=b["median"] / a["median"], speedup_vs_calls_alone=float(np.median(b_calls)) / a["median"],
                    faster_by_more_than_the_spread=bool(b["median"] - a["median"] > spread), spread_ms=spread,
                    robot_ticks=st["robot_ticks"], stayed=st["stayed"], neighbour=st["neighbour"], global_search=st["global"],
                    final_status=dict(running=st["running"], reached=st["reached"], out_of_map=st["out_of_map"], no_field=st["no_field"]),
                    idle_lane_share_last_tick=1.0 - st["running"] / n, loop_robots_ok_at_end=ok)
                print("%d_%s" % (n, mix), json.dumps(res["shapes"]["%d_%s" % (n, mix)]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
