"""Timing of the fleet rollout's separation check (mnav_fleet_rollout) on the mesh and fields of tools/rollout_perf.py: the
1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the resident vector maps of a 7 168-plan Dijkstra batch, robot i on plan
i mod 7 168 in the "stay" mix.  A `--ticks`-tick call with a check every 1 and every 10 ticks for 1, 14 336 and 1 048 576
robots, and for 14 336 robots on `--few` plans only (a fleet that converges on few goals, REACHED robots staying in the way),
two ways:

  (a) one mnav_fleet_rollout call: wall clock around the call, the device time of all its kernels and of the separation
      kernels alone, the distance tests performed and tests per second, the cost of a check relative to a tick;
  (b) the way to the same answer without it: mnav_follow_rollout with trace_stride = check_stride, the trace downloaded, and
      a neighbour search on the host per trace row (scipy's cKDTree.query_pairs where scipy is there, else a numpy grid), which
      yields the pairs, the partners per robot and the closest distance per robot.  Beyond `--host-rows` rows the search is
      timed on that many evenly spaced rows and scaled to all of them (recorded as `host_rows_timed`); from 100 000 robots on
      it is timed on one row, in one repetition.  (b) sees RUNNING and
      stopped robots alike, as the flags WAITING_PRESENT | REACHED_PRESENT do, which is what (a) runs with.

(a) and (b) alternate, medians of `--reps` repetitions after `--warmup`, with the spread of the repeats.

    python tools/fleet_rollout_perf.py [--reps K] [--ticks T] [--sizes a,b,c] [--radius R] [--out FILE]"""
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
from rollout_perf import stats  # noqa: E402

try:
    from scipy.spatial import cKDTree
except ImportError:                                                    # the numpy grid below
    cKDTree = None


def pairs_of_row(pos, radius):
    """the near pairs (i < j) of one trace row"""
    if cKDTree is not None:
        return cKDTree(pos).query_pairs(radius, output_type="ndarray")
    cell = np.floor(pos / radius).astype(np.int64)
    cell -= cell.min(axis=0)
    dims = cell.max(axis=0) + 3
    key = ((cell[:, 0] + 1) * dims[1] + cell[:, 1] + 1) * dims[2] + cell[:, 2] + 1
    order = np.argsort(key, kind="stable")
    skey = key[order]
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                other = key + (dx * dims[1] + dy) * dims[2] + dz
                lo, hi = np.searchsorted(skey, other, "left"), np.searchsorted(skey, other, "right")
                rep = hi - lo
                i = np.repeat(np.arange(pos.shape[0]), rep)
                j = order[np.repeat(lo, rep) + (np.arange(rep.sum()) - np.repeat(np.cumsum(rep) - rep, rep))]
                keep = (i < j) & (((pos[i] - pos[j]) ** 2).sum(axis=1) <= radius * radius)
                out.append(np.stack([i[keep], j[keep]], axis=1))
    return np.concatenate(out)


def host_search(trace, radius, max_rows):
    """(b)'s host part: per row the pairs, the partners per robot and the closest partner's d2 per robot; returns (ms for
    all rows -- scaled when only `max_rows` of them were timed --, rows timed, near pairs of the rows timed)"""
    n, rows = trace.shape[0], trace.shape[1]
    pick = np.arange(rows) if rows <= max_rows else np.unique(np.linspace(0, rows - 1, max_rows).astype(np.int64))
    near_checks, min_d2, total = np.zeros(n, np.int64), np.full(n, np.inf), 0
    t0 = time.perf_counter()
    for k in pick:
        pos = np.ascontiguousarray(trace[:, k], np.float64)
        ok = np.isfinite(pos).all(axis=1)
        ids = np.nonzero(ok)[0]
        pr = ids[pairs_of_row(pos[ok], radius)] if ids.size > 1 else np.zeros((0, 2), np.int64)
        total += pr.shape[0]
        if pr.shape[0]:
            d2 = ((pos[pr[:, 0]] - pos[pr[:, 1]]) ** 2).sum(axis=1)
            partners = np.bincount(pr.ravel(), minlength=n)
            near_checks += partners > 0
            np.minimum.at(min_d2, pr[:, 0], d2)
            np.minimum.at(min_d2, pr[:, 1], d2)
    ms = (time.perf_counter() - t0) * 1e3
    return ms * rows / len(pick), len(pick), total


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
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_rollout_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    shapes = [(int(s), args.plans, "all_plans") for s in args.sizes.split(",")] + [(14336, args.few, "few_goals")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=args.plans, few=args.few, reps=args.reps, warmup=args.warmup, ticks=args.ticks, dt=args.dt, radius=args.radius,
               host_search="scipy cKDTree.query_pairs" if cKDTree is not None else "numpy grid", shapes={})
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
            for stride in [int(s) for s in args.strides.split(",")]:
                ro = capi.RolloutConfig(dt=args.dt, ticks=args.ticks, dist_tolerance=0.3, angle_tolerance=3.2)
                rt = capi.RolloutConfig(dt=args.dt, ticks=args.ticks, dist_tolerance=0.3, angle_tolerance=3.2, trace_stride=stride)
                sep = capi.SeparationConfig(radius=args.radius, check_stride=stride, flags=flags)
                g = (None, None) if goals is None else goals
                a_wall, a_kern, a_sep, b_wall, b_call, b_host, plain = [], [], [], [], [], [], []
                for rep in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    out = ctx.fleet_rollout(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"], None, g[0], g[1], cfg, ro, None, sep)
                    wall = (time.perf_counter() - t0) * 1e3
                    st = ctx.fleet_rollout_stats()
                    t0 = time.perf_counter()
                    tr = ctx.rollout(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"], None, g[0], g[1], cfg, rt)
                    call = (time.perf_counter() - t0) * 1e3
                    if n < 100000 or rep == args.warmup:                  # (a large fleet's host search is timed once: it takes minutes)
                        host, rows_timed, host_pairs = host_search(tr.trace, args.radius, args.host_rows if n < 100000 else 1)
                    del tr
                    t0 = time.perf_counter()
                    ctx.rollout(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"], None, g[0], g[1], cfg, ro, outputs=("status",))
                    no_check = (time.perf_counter() - t0) * 1e3
                    if rep >= args.warmup:
                        a_wall.append(wall); a_kern.append(st["ms_kernels"]); a_sep.append(st["ms_separation"])
                        b_wall.append(call + host); b_call.append(call); b_host.append(host); plain.append(no_check)
                a, b = stats(a_wall), stats(b_wall)
                spread = max(a["max"] - a["min"], b["max"] - b["min"])
                checks = max(st["checks_run"], 1)
                sep_ms, kern_ms = float(np.median(a_sep)), float(np.median(a_kern))
                tick_ms = (kern_ms - sep_ms) / args.ticks
                key = "%d_%s_stride%d" % (n, name, stride)
                res["shapes"][key] = dict(
                    fleet_ms_call_wall=a, fleet_ms_kernels=stats(a_kern), fleet_ms_separation=stats(a_sep), rollout_without_check_ms_wall=stats(plain),
                    parent_ms_wall=b, parent_ms_rollout_with_trace=stats(b_call), parent_ms_host_search=stats(b_host), host_rows_timed=rows_timed,
                    host_rows=args.ticks // stride, speedup_vs_parent=b["median"] / a["median"], faster_by_more_than_the_spread=bool(b["median"] - a["median"] > spread),
                    spread_ms=spread, checks_run=st["checks_run"], checks_skipped=st["checks_skipped"], first_skipped_tick=st["first_skipped_tick"],
                    tests=st["tests"], tests_per_second=st["tests"] / (sep_ms * 1e-3) if sep_ms > 0 else 0.0, near_pairs=st["near_pairs"], max_pairs=st["max_pairs"],
                    max_cell=st["max_cell"], robots_near=st["robots_near"], ms_per_check=sep_ms / checks, ms_per_tick_without_checks=tick_ms,
                    check_cost_in_ticks=(sep_ms / checks) / tick_ms if tick_ms > 0 else 0.0, host_pairs_in_rows_timed=host_pairs,
                    final_status=dict(running=st["running"], reached=st["reached"], out_of_map=st["out_of_map"], no_field=st["no_field"]))
                print(key, json.dumps(res["shapes"][key]), flush=True)
                if args.out:                                              # after every shape: a run cut short leaves what it measured
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
