"""mnav_replan_dijkstra_batch against mnav_plan_dijkstra_batch (engine `auto`) on the same final map: the 1M-vertex C2 mesh,
terrain(1000, 0.1, 2), uploaded weights, one plan and 64 plans, resident outputs on in both contexts (both leave dist, pred
and the vector map on the device; nothing V-sized is downloaded).

Events: a square patch of 11 x 11 vertices on the line from the wave's seed to the robot, blocked (cost 1.5) and freed
again in turn, so that every repetition is a real event with the same rewind level; the patch sits at 0.95, 0.75, 0.5,
0.25 and 0.05 of the way, which puts L / cut_old near those values for the single plan (the measured ratio is recorded,
with cut_old = goal_cut(d_old[robot], offset) of mnav_eval.h; for the 64 plans, whose seeds are random, the minimum and
the median over all plans -- the minimum is what the policy option replan_fresh_below compares).  Target-only moves: the
robot hops between two vertices 1 m apart, with an empty log.

Method: context A replans, context B plans afresh; per repetition the event goes to A, A's call is timed (wall clock
around the call, which synchronises), then the same for B -- alternating, after warm-up repetitions, medians with the
spread (min, max) of at least 7 repetitions.  Both timed calls are the binding's wrapper with want_stats off: the same
buffers, the C call, mnav_get_timing; mnav_replan_stats and the downloads for the ratio come after the clock stopped.
The replan is split by mnav_replan_stats into level, rewind, rounds and finalize; `tail` is the rest of the call (tables
rebuilt for the new costs, path walks, vector map, result download).

    python tools/replan_perf.py [--reps K] [--out FILE]

--repair-engine 0,5 runs the same cases once per value of the option replan_repair_engine on context A (0 the tile rounds, 5
the tile-batch engine started from the rewound fields by k_tb_warm) and appends the rows, each with its `repair_engine` and the
figures of mnav_replan_warm_stats, to the list `repair_engine_cases` of the file, next to the old rows."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402

N = 1000
FRACTIONS = (0.95, 0.75, 0.5, 0.25, 0.05)


def spread(xs):
    xs = sorted(xs)
    return dict(median=float(np.median(xs)), min=float(xs[0]), max=float(xs[-1]), n=len(xs))


def patch(cx, cy, r=5):
    return np.array([y * N + x for y in range(cy - r, cy + r + 1) for x in range(cx - r, cx + r + 1)], np.uint32)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def old_cuts(ctx, n, target, offset):
    """goal_cut (mnav_eval.h) of every plan's resident potential at the robot vertex, in float32 as on the device"""
    dt = np.array([ctx.download_output("dist", i)[target] for i in range(n)], np.float32)
    goal = (dt.astype(np.float64) + offset).astype(np.float32)
    return np.where(np.isfinite(dt), np.maximum(goal, dt), np.float32(np.inf))


def run_case(A, B, seeds, target0, events, reps, warm):
    """events(k) -> (ids, value or None, target): the k-th event and robot vertex.  Returns the record of the case."""
    n = len(seeds)
    tg = np.full(n, target0, np.uint32)
    A.plan_dijkstra_batch(seeds, tg, 0.3)
    B.plan_dijkstra_batch(seeds, tg, 0.3)
    cut = old_cuts(A, n, target0, 0.3)
    rec = dict(replan=[], fresh=[], level=[], rewind=[], rounds=[], finalize=[], kept=[], rewound=[], tiles_woken=[], ratio_min=[], ratio_median=[], reason=[])
    for k in range(warm + reps):
        ids, val, t = events(k)
        tg = np.full(n, t, np.uint32)
        if ids is not None:
            A.update_costs(ids, np.full(ids.size, val, np.float32))
        ms_a, a = timed(lambda: A.replan_dijkstra(tg, 0.3, want_stats=False))
        if ids is not None:
            B.update_costs(ids, np.full(ids.size, val, np.float32))
        ms_b, b = timed(lambda: B.plan_dijkstra_batch(seeds, tg, 0.3, want_stats=False))
        assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["path_len"], b["path_len"]), "replan and fresh plan differ"
        rp = A.replan_stats(n)
        if k >= warm:
            rec.setdefault("warm", []).append(A.replan_warm_stats())
            rec["replan"].append(ms_a); rec["fresh"].append(ms_b)
            for key in ("level", "rewind", "rounds", "finalize"):
                rec[key].append(rp["ms_" + key])
            for key in ("kept", "rewound", "tiles_woken", "reason"):
                rec[key].append(rp[key])
            if rp["levels"] is not None:
                vote = np.isfinite(cut) & (cut > 0)                                        # (plans with an infinite old cut do not vote)
                ratio = rp["levels"][vote].astype(np.float64) / cut[vote]
                rec["ratio_min"].append(float(ratio.min())); rec["ratio_median"].append(float(np.median(ratio)))
        cut = old_cuts(A, n, t, 0.3)                                                       # the next repetition's old cut
    out = dict(plans=n, fresh_ms=spread(rec["fresh"]), replan_ms=spread(rec["replan"]),
               split_ms={k: float(np.median(rec[k])) for k in ("level", "rewind", "rounds", "finalize")},
               kept=int(np.median(rec["kept"])), rewound=int(np.median(rec["rewound"])), tiles_woken=int(np.median(rec["tiles_woken"])),
               reasons=sorted(set(rec["reason"])),
               level_over_cut=dict(min=float(np.median(rec["ratio_min"])), median=float(np.median(rec["ratio_median"]))) if rec["ratio_min"] else None)
    out["split_ms"]["tail"] = out["replan_ms"]["median"] - sum(out["split_ms"].values())
    out["speedup"] = out["fresh_ms"]["median"] / out["replan_ms"]["median"]
    out["warm"] = {k: float(np.median([x[k] for x in rec["warm"]])) for k in ("plans", "iterations", "pairs_woken", "words", "ms_warm", "ms_engine", "ms_finalize", "fallback")}
    print(json.dumps(out), flush=True)
    return out


def all_cases(A, B, batches, robot, reps, warm, engine):
    """every patch position and the target-only move for every batch; engine: A's replan_repair_engine (None: unset)"""
    cases = []
    for n, seeds in batches.items():
        for f in FRACTIONS:
            ids = patch(int(round((0.1 + 0.8 * f) * (N - 1))), (N - 1) // 2)
            rec = run_case(A, B, seeds, robot, lambda k: (ids, 1.5 if k % 2 == 0 else 0.0, robot), reps, warm)
            if rec["reasons"] != [0]:
                raise SystemExit("a replan planned afresh: nothing to compare")
            # leave the map as it was (an even number of events frees the patch again)
            if (warm + reps) % 2:
                for c in (A, B):
                    c.update_costs(ids, np.zeros(ids.size, np.float32))
            rec.update(kind="patch", placed_at=f)
            cases.append(rec)
        hop = robot - 10
        rec = run_case(A, B, seeds, robot, lambda k: (None, None, hop if k % 2 == 0 else robot), reps, warm)
        rec.update(kind="target only", placed_at=None)
        cases.append(rec)
    if engine is not None:
        for rec in cases:
            rec.update(repair_engine=engine)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repair-engine", default="", help="values of replan_repair_engine to run the cases with (0,5): rows go to repair_engine_cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_perf.json"))
    args = ap.parse_args()
    reps = max(7, args.reps)
    mesh = meshgen.terrain(N, 0.1, 2)
    w = meshgen.edge_lengths(mesh)
    costs = np.zeros(mesh.V, np.float32)
    A, B = capi.MnavContext(0), capi.MnavContext(0)
    for c in (A, B):
        c.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        c.upload_costs(costs, w)
        c.set_resident_outputs(True)
    A.set_option("replan_fresh_below", 0)                              # the repair is what is measured, at every level
    seed, robot = mesh.vertex_at(0.1, 0.5), mesh.vertex_at(0.9, 0.5)
    rng = np.random.default_rng(64)
    batches = {1: np.array([seed], np.uint32), 64: rng.choice(mesh.V, 64, replace=False).astype(np.uint32)}
    result = dict(mesh="terrain(1000, 0.1, 2): 1 000 000 vertices, uploaded weights (edge_cost_factor 0)", offset=0.3, repetitions=reps,
                  method="alternating replan (context A) / fresh plan under auto (context B) on the same final map, wall ms per call, resident outputs on",
                  cases=[])
    engines = [int(x) for x in args.repair_engine.split(",") if x]
    for engine in engines or [None]:
        A.set_option("replan_repair_engine", engine)
        result["cases"] += all_cases(A, B, batches, robot, reps, args.warmup, engine)
    if engines:                                                        # next to the old rows, not over them
        rows = result["cases"]
        result = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                result = json.load(fh)
        result["repair_engine_cases"] = rows
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        A.close(); B.close()
        return
    # where the curves cross: the largest measured L / cut_old at which the fresh plan still wins (median against median)
    for n in batches:
        rows = sorted((c for c in result["cases"] if c["plans"] == n and c["kind"] == "patch"), key=lambda c: c["level_over_cut"]["min"])
        lost = [c["level_over_cut"]["min"] for c in rows if c["replan_ms"]["median"] >= c["fresh_ms"]["median"]]
        won = [c["level_over_cut"]["min"] for c in rows if c["replan_ms"]["median"] < c["fresh_ms"]["median"]]
        result["crossover_%d_plans" % n] = dict(fresh_wins_up_to=max(lost) if lost else None, replan_wins_from=min(won) if won else None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    A.close(); B.close()


if __name__ == "__main__":
    main()
