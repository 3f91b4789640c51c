"""Timing of the yielding fleet rollout (mnav_fleet_rollout_yield) on the mesh and fields of tools/fleet_rollout_perf.py: the
1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the resident vector maps of a 7 168-plan Dijkstra batch, robot i on plan
i mod 7 168 in the "stay" mix.  A `--ticks`-tick call with a check every 1 and every 10 ticks for 1, 14 336 and 1 048 576
robots, and for 14 336 robots on `--few` plans only (a fleet that converges on few goals, where queues form), three ways:

  (y) one mnav_fleet_rollout_yield call: wall clock around the call, the device time of all its kernels, of the kernels of
      its checks and of the pair passes alone (mnav_fleet_yield_stats), and what the rule did (robots held, held ticks);
  (a) one mnav_fleet_rollout call over the same robots with the same separation config: what the check costs without the
      rule.  The difference to (y) is what yielding costs -- in time; the motion differs, held robots have no tick.  With
      `--fleet-only` the tool measures nothing but (a), and with `--tree DIR` it takes the package (capi.py and libmnav.so)
      from another checkout: the parent commit's, for an A/B of (a) in one visit (parent, head, parent, head);
  (b) the only way to the same motion without the entry point: one mnav_fleet_rollout call per check interval (check_stride
      ticks, no separation), position, heading, face and status downloaded, the decision on the host (scipy's
      cKDTree.query_pairs where scipy is there, else the numpy grid of tools/fleet_rollout_perf.py; the rule in numpy float32
      over the pairs), held robots given start_tick = check_stride for the next interval.  Timed on `--intervals` intervals
      and scaled to ticks / check_stride of them: an EXTRAPOLATION wherever that is more intervals than were timed (recorded
      as `b_intervals_timed` / `b_intervals`).  From 100 000 robots on (b) is left out unless `--big-parent-way` is given (then:
      one interval, once): the fleet of a million stands 146 to a face, 71 M near pairs per check, minutes and gigabytes of
      host search per interval.  Stopped robots are fed back like the others (they stop again at their first
      tick): (b) is a timing of the round trip, not a second implementation of the rule.

(y), (a) and (b) alternate, medians of `--reps` repetitions after `--warmup`, with the spread of the repeats.

    python tools/fleet_yield_perf.py [--reps K] [--ticks T] [--sizes a,b,c] [--radius R] [--fleet-only] [--tree DIR] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(_tree))                            # the package of this tree first
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_navigation_amd import capi, meshgen  # noqa: E402  (before the tools below, which put this tree's package first)
from fleet_rollout_perf import pairs_of_row  # noqa: E402
from follow_perf import make_robots  # noqa: E402
from rollout_perf import stats  # noqa: E402

F32 = np.float32


def host_decision(pos, direction, status, waiting, radius, c, priority):
    """the rule of include/mnav.h on the host over the near pairs of one check (REACHED robots present): hold per robot"""
    n = pos.shape[0]
    ok = np.isfinite(pos).all(axis=1)
    ids = np.nonzero(ok)[0]
    hold = np.zeros(n, bool)
    if ids.size < 2:
        return hold
    pr = ids[pairs_of_row(np.ascontiguousarray(pos[ok], np.float64), radius)]
    if not pr.shape[0]:
        return hold
    i, j = np.concatenate([pr[:, 0], pr[:, 1]]), np.concatenate([pr[:, 1], pr[:, 0]])
    e = pos[j] - pos[i]
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    c2 = F32(c) * F32(c)

    def ahead(a, ee):
        dot = (direction[a, 0] * ee[:, 0] + direction[a, 1] * ee[:, 1]) + direction[a, 2] * ee[:, 2]
        return (dot > 0) & (dot * dot >= c2 * d2)

    mover = (status == 0) & ~waiting
    a_ij, a_ji = ahead(i, e), ahead(j, -e)
    before = (priority[j] < priority[i]) | ((priority[j] == priority[i]) & (j < i))
    yields = mover[i] & a_ij & (~mover[j] | ~a_ji | before)
    hold[i[yields]] = True
    return hold


def parent_way(ctx, rb, g, cfg, args, stride, priority, intervals):
    """(b): `intervals` check intervals; returns the wall ms of all of them"""
    n = rb["pos"].shape[0]
    pos, direction, face = rb["pos"], rb["dir"], rb["face_in"]
    start = np.zeros(n, np.uint32)
    ro = capi.RolloutConfig(dt=args.dt, ticks=stride, dist_tolerance=0.3, angle_tolerance=3.2)
    t0 = time.perf_counter()
    for _ in range(intervals):
        out = ctx.fleet_rollout(pos, direction, rb["up"], face, rb["slot"], None, g[0], g[1], cfg, ro, start, None, outputs=("status", "pos", "dir", "face"))
        pos, direction, face = out.pos, out.dir, out.face
        hold = host_decision(pos, direction, out.status, np.zeros(n, bool), args.radius, args.ahead_cos, priority)
        start = np.where(hold, stride, 0).astype(np.uint32)
    return (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--few", type=int, default=16)
    ap.add_argument("--sizes", default="1,14336,1048576")
    ap.add_argument("--strides", default="1,10")
    ap.add_argument("--radius", type=float, default=0.25)
    ap.add_argument("--ahead-cos", type=float, default=0.5)
    ap.add_argument("--intervals", type=int, default=4)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--fleet-only", action="store_true")
    ap.add_argument("--big-parent-way", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_yield_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    shapes = [(int(s), args.plans, "all_plans") for s in args.sizes.split(",")]
    shapes = [s for s in shapes if s[0] < 100000] + [(14336, args.few, "few_goals")] + [s for s in shapes if s[0] >= 100000]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=args.plans, few=args.few, reps=args.reps, warmup=args.warmup, ticks=args.ticks, dt=args.dt, radius=args.radius,
               ahead_cos=args.ahead_cos, tree=os.path.relpath(os.path.abspath(args.tree), ROOT), fleet_only=args.fleet_only,
               host_search="scipy cKDTree.query_pairs" if "cKDTree" in pairs_of_row.__globals__ and pairs_of_row.__globals__["cKDTree"] is not None else "numpy grid",
               shapes={})
    cfg = capi.FollowConfig()
    flags = capi.SEP_WAITING_PRESENT | capi.SEP_REACHED_PRESENT
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(5)
        seeds = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        targets = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        r = ctx.plan_dijkstra_batch(seeds, targets, path_cap=4096, want_stats=False)
        res["engine"] = ctx.last_engine()
        del r
        ctx.locate(mesh.xyz[:8])                                          # the lookup index exists before anything is timed
        for n, n_slots, name in shapes:
            rb = make_robots(mesh, targets, n, n_slots, "stay", 10 + n)
            goals = None
            if name == "few_goals":                                       # the goal of every plan, so that robots arrive and stay
                goals = (np.ascontiguousarray(mesh.xyz[seeds[rb["slot"]]], np.float32), np.tile(np.array([1, 0, 0], np.float32), (n, 1)))
            priority = (np.arange(n) % 4).astype(np.uint32)
            for stride in [int(s) for s in args.strides.split(",")]:
                ro = capi.RolloutConfig(dt=args.dt, ticks=args.ticks, dist_tolerance=0.3, angle_tolerance=3.2)
                sep = capi.SeparationConfig(radius=args.radius, check_stride=stride, flags=flags)
                g = (None, None) if goals is None else goals
                total = args.ticks // stride
                timed = min(args.intervals, total) if n < 100000 else 1
                with_b = not args.fleet_only and (n < 100000 or args.big_parent_way)
                y_wall, y_kern, y_sep, y_pair, a_wall, a_kern, a_sep, b_wall = [], [], [], [], [], [], [], []
                ys = fs = None
                for rep in range(args.warmup + args.reps):
                    if not args.fleet_only:
                        t0 = time.perf_counter()
                        ctx.fleet_rollout_yield(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"], None, g[0], g[1], cfg, ro, None, sep,
                                                capi.YieldConfig(ahead_cos=args.ahead_cos), priority)
                        wall = (time.perf_counter() - t0) * 1e3
                        ys = ctx.fleet_yield_stats()
                    t0 = time.perf_counter()
                    ctx.fleet_rollout(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"], None, g[0], g[1], cfg, ro, None, sep)
                    fleet = (time.perf_counter() - t0) * 1e3
                    fs = ctx.fleet_rollout_stats()
                    if with_b and (n < 100000 or rep == args.warmup):     # (a large fleet's round trip is timed once)
                        way = parent_way(ctx, rb, g, cfg, args, stride, priority, timed) * total / timed
                    if rep >= args.warmup:
                        a_wall.append(fleet); a_kern.append(fs["ms_kernels"]); a_sep.append(fs["ms_separation"])
                        if not args.fleet_only:
                            y_wall.append(wall); y_kern.append(ys["ms_kernels"]); y_sep.append(ys["ms_separation"]); y_pair.append(ys["ms_pair"])
                            if with_b:
                                b_wall.append(way)
                key = "%d_%s_stride%d" % (n, name, stride)
                row = dict(fleet_ms_call_wall=stats(a_wall), fleet_ms_kernels=stats(a_kern), fleet_ms_separation=stats(a_sep), checks_run=fs["checks_run"],
                           fleet_near_pairs=fs["near_pairs"], fleet_final_status=dict(running=fs["running"], reached=fs["reached"], out_of_map=fs["out_of_map"], no_field=fs["no_field"]))
                if not args.fleet_only:
                    y, a = stats(y_wall), row["fleet_ms_call_wall"]
                    if with_b:
                        b = stats(b_wall)
                        row.update(parent_way_ms_wall=b, b_intervals_timed=timed, b_intervals=total, b_extrapolated=bool(timed < total),
                                   parent_way_over_yield=b["median"] / y["median"])
                    else:
                        row.update(parent_way_ms_wall="not measured")
                    row.update(yield_ms_call_wall=y, yield_ms_kernels=stats(y_kern), yield_ms_separation=stats(y_sep), yield_ms_pair=stats(y_pair),
                               yield_minus_fleet_ms=y["median"] - a["median"], yield_over_fleet=y["median"] / a["median"],
                               ms_pair_per_check=float(np.median(y_pair)) / max(ys["checks_run"], 1), robots_held=ys["robots_held"], held_ticks=ys["held_ticks"],
                               max_held=ys["max_held"], max_held_tick=ys["max_held_tick"], held_last=ys["held_last"], checks_skipped=ys["checks_skipped"])
                res["shapes"][key] = row
                print(key, json.dumps(row), flush=True)
                if args.out:                                              # after every shape: a run cut short leaves what it measured
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
