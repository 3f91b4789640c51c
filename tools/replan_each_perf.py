"""mnav_replan_dijkstra_each against mnav_replan_dijkstra_batch (default policy) and mnav_plan_dijkstra_batch (engine `auto`)
on the same final map: the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), uploaded weights, resident outputs on in every context
(dist, pred and the vector map stay on the device; nothing V-sized is downloaded), random robots, 64, 1 024 and 7 168 plans.

Events: an 11 x 11 patch, blocked (cost 1.5) and freed again in turn, so that every repetition is a real event -- in the
middle of the mesh, where most fields of a uniform batch reach it, and (`patch, corner`, uniform goals) 30 cells from a corner,
where few do; and (`patch, local fleet`) the middle patch under a fleet whose robots stand within 60 cells of their goals: small
fields, most of which never meet the event.  A random goal is FRESH only when it lies next to the patch, a few per cent of a uniform batch; to move the FRESH
share the batch takes a share phi of its goals from the ring of 8 .. 40 cells around the patch (their fields meet the event
within the first quarter of their cut: FRESH) and the rest uniformly from the mesh.  phi runs over SHARES; the classes the
device found are recorded, and the measured FRESH share, not phi, is what the crossing is read from.  The robot-only case:
no event, every robot hops to a vertex ten columns away and back.

The share policy is off in the measured context (replan_each_fresh_share 1): its default is what these numbers set.

Method: one context per entry point -- `each`, `batch`, `fresh` --, all on the same map; per repetition the event goes to a
context and its call is timed (wall clock around the binding's wrapper with want_stats off, which synchronises), context after
context, after warm-up repetitions; medians with the spread (min, max).  With --sequential (7 168 plans: 143 GB of resident
outputs per context) the contexts live one after the other instead and the repetitions do not alternate.

One batch size per process, every GPU step under its own time limit, chained:

    timeout -k 10 600 python tools/replan_each_perf.py --plans 64 &&
    timeout -k 10 600 python tools/replan_each_perf.py --plans 1024 --append &&
    timeout -k 10 1100 python tools/replan_each_perf.py --plans 7168 --append --sequential

--repair-engine 0,5 measures the repair engines of the REPAIRED plans against each other instead (option replan_repair_engine:
0 the tile rounds, 5 the tile-batch engine started from the rewound fields by k_tb_warm): one `each` context per value and the
fresh plan, in the same run, no `batch` context; the rows go to the list `repair_engine_cases` of the file, next to the old
rows, with the warm start's own figures (mnav_replan_warm_stats: plans, iterations, ms of k_tb_warm, of the engine and of the
finalize pass, and k_tb_warm's GB/s over NP * S * 8 bytes) and, for comparison, the iterations of the fresh batch and the rate
of a 1 GiB device-to-device copy taken in the same process."""
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
SHARES = (0.0, 0.05, 0.1, 0.25, 0.5, 0.75, 1.0)
PATH_CAP = 8192                                                        # ids per path row on the host (a path has ~1.4 sqrt(V) hops)
KINDS = ("each", "batch", "fresh")


def spread(xs):
    xs = sorted(xs)
    return dict(median=float(np.median(xs)), min=float(xs[0]), max=float(xs[-1]), n=len(xs))


def patch(cx, cy, r=5):
    return np.array([y * N + x for y in range(cy - r, cy + r + 1) for x in range(cx - r, cx + r + 1)], np.uint32)


def goals(rng, n, phi):
    """n goals: round(phi n) from the ring of 8 .. 40 cells around the patch, the rest uniform"""
    k = int(round(phi * n))
    c = (N - 1) // 2
    out = []
    while len(out) < k:
        dx, dy = rng.integers(-40, 41, 2)
        if max(abs(dx), abs(dy)) >= 8:
            out.append((c + dy) * N + c + dx)
    out += rng.integers(0, N * N, n - k).tolist()
    return np.array(out, np.uint32)


def make(mesh, w, costs):
    c = capi.MnavContext(0)
    c.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
    c.upload_costs(costs, w)
    c.set_resident_outputs(True)
    c.set_option("replan_each_fresh_share", 1)                         # the per-plan path is what is measured, at every share
    return c


def copy_rate():
    """GB/s (read + written) of a 1 GiB device-to-device copy, best of 5 after a warm-up; None without torch"""
    try:
        import torch
    except ImportError:
        return None
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1.0)
    best = None
    for k in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if k and (best is None or ms < best):
            best = ms
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * (1 << 30) / (best * 1e-3) / 1e9


def call(kind, ctx, seeds, tg):
    if kind.startswith("each"):
        return ctx.replan_dijkstra_each(tg, 0.3, path_cap=PATH_CAP, want_stats=False)
    if kind == "batch":
        return ctx.replan_dijkstra(tg, 0.3, path_cap=PATH_CAP, want_stats=False)
    return ctx.plan_dijkstra_batch(seeds, tg, 0.3, path_cap=PATH_CAP, want_stats=False)


def run_case(ctxs, seeds, robots, events, reps, warm):
    """ctxs: kind -> context, all holding the same map; events(k) -> (ids or None, value, robots of repetition k).  Every context
    sees every event; returns kind -> record."""
    n = len(seeds)
    rec = {kind: dict(ms=[], codes=None) for kind in ctxs}
    for kind, c in ctxs.items():
        c.plan_dijkstra_batch(seeds, robots, 0.3, path_cap=PATH_CAP, want_stats=False)
    for k in range(warm + reps):
        ids, val, tg = events(k)
        first = None
        for kind, c in ctxs.items():
            if ids is not None:
                c.update_costs(ids, np.full(ids.size, val, np.float32))
            t0 = time.perf_counter()
            out = call(kind, c, seeds, tg)
            ms = 1e3 * (time.perf_counter() - t0)
            if first is None:
                first = out
            assert np.array_equal(out["codes"], first["codes"]) and np.array_equal(out["path_len"], first["path_len"]), "the entry points differ"
            r = rec[kind]
            if k >= warm:
                r["ms"].append(ms)
                if kind.startswith("each@"):
                    wm = c.replan_warm_stats()
                    for key in ("plans", "iterations", "pairs_woken", "words", "ms_warm", "ms_engine", "ms_finalize", "fallback"):
                        r.setdefault("warm_" + key, []).append(wm[key])
                    r["warm_kernel"] = wm["kernel"]
                if kind == "fresh":
                    r.setdefault("iterations", []).append(c.timing().get("steps", 0))
                    r["engine"] = c.last_engine()
                if kind.startswith("each"):
                    e = c.replan_each_stats(n)
                    for key in ("kept_plans", "repaired_plans", "fresh_plans", "kept", "rewound", "tiles_woken", "rounds", "whole_fresh", "reason",
                                "ms_classify", "ms_rewind", "ms_rounds", "ms_finalize", "ms_fresh"):
                        r.setdefault(key, []).append(e[key])
                    r["fresh_engine"] = e["fresh_engine"]
                if kind == "batch":
                    r.setdefault("reason", []).append(c.replan_stats()["reason"])
    out = {}
    for kind, r in rec.items():
        o = dict(ms=spread(r["ms"]))
        if kind.startswith("each@"):
            o["warm"] = {key: float(np.median(r["warm_" + key])) for key in ("plans", "iterations", "pairs_woken", "words", "ms_warm", "ms_engine", "ms_finalize", "fallback")}
            o["warm"]["kernel"] = r["warm_kernel"]
            if o["warm"]["ms_warm"] > 0:
                o["warm"]["k_tb_warm_GBps"] = 8.0 * o["warm"]["words"] / (o["warm"]["ms_warm"] * 1e-3) / 1e9
        if kind == "fresh":
            o["iterations"] = int(np.median(r["iterations"])); o["engine"] = r["engine"]
        if kind.startswith("each"):
            for key in ("kept_plans", "repaired_plans", "fresh_plans", "kept", "rewound", "tiles_woken", "rounds"):
                o[key] = int(np.median(r[key]))
            o["split_ms"] = {key[3:]: float(np.median(r[key])) for key in ("ms_classify", "ms_rewind", "ms_rounds", "ms_finalize", "ms_fresh")}
            o["whole_fresh"] = bool(max(r["whole_fresh"])); o["reasons"] = sorted(set(r["reason"])); o["fresh_engine"] = r["fresh_engine"]
            o["fresh_share"] = o["fresh_plans"] / n
        if kind == "batch":
            o["reasons"] = sorted(set(r["reason"]))
        out[kind] = o
    return out


def crossing(rows):
    """the smallest FRESH share at which `each` stops beating `batch` (median against median), linear between the two
    measured shares around it; None: it won at every share"""
    rows = sorted(rows, key=lambda c: c["each"]["fresh_share"])
    prev = None
    for c in rows:
        x, d = c["each"]["fresh_share"], c["each"]["ms"]["median"] - c["batch"]["ms"]["median"]
        if d >= 0:
            if prev is None or prev[1] >= 0 or d == prev[1]:
                return x
            return prev[0] + (x - prev[0]) * (0 - prev[1]) / (d - prev[1])
        prev = (x, d)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shares", default=",".join(str(s) for s in SHARES), help="shares of goals near the middle patch; empty: none of these cases")
    ap.add_argument("--no-corner", action="store_true")
    ap.add_argument("--only", default="", help="run the cases of this kind only")
    ap.add_argument("--sequential", action="store_true", help="one context at a time (resident outputs of a large batch fill the device)")
    ap.add_argument("--append", action="store_true", help="add this batch size to an existing file")
    ap.add_argument("--repair-engine", default="", help="values of replan_repair_engine to measure against each other (0,5): rows go to repair_engine_cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_each_perf.json"))
    args = ap.parse_args()
    n, reps, warm = args.plans, args.reps, args.warmup
    engines = [int(x) for x in args.repair_engine.split(",") if x]
    kinds = tuple("each@%d" % e for e in engines) + ("fresh",) if engines else KINDS
    d2d = copy_rate() if engines else None
    shares = [float(s) for s in args.shares.split(",") if s]
    mesh = meshgen.terrain(N, 0.1, 2)
    w = meshgen.edge_lengths(mesh)
    costs = np.zeros(mesh.V, np.float32)
    mid, corner = patch((N - 1) // 2, (N - 1) // 2), patch(30, 30)
    cases = [("patch", phi) for phi in shares] + ([] if args.no_corner else [("patch, corner", 0.0)]) + [("patch, local fleet", 0.0), ("robots only", 0.0)]
    cases = [c for c in cases if not args.only or c[0] == args.only]
    inputs = []
    for kind, phi in cases:
        rng = np.random.default_rng(1000 * n + int(100 * phi) + {"patch": 0, "robots only": 7, "patch, corner": 13, "patch, local fleet": 17}[kind])
        ids = corner if kind == "patch, corner" else mid
        seeds = goals(rng, n, phi)
        robots = rng.integers(0, N * N, n).astype(np.uint32)
        if kind == "patch, local fleet":
            x = np.clip(seeds % N + rng.integers(-60, 61, n), 0, N - 1); y = np.clip(seeds // N + rng.integers(-60, 61, n), 0, N - 1)
            robots = (y * N + x).astype(np.uint32)
        robots = np.where(robots == seeds, (robots + 7) % (N * N), robots).astype(np.uint32)
        robots = np.where(np.isin(robots, ids), (robots + 20 * N) % (N * N), robots).astype(np.uint32)   # (no robot on the patch)
        hop = np.where(robots % N >= 10, robots - 10, robots + 10).astype(np.uint32)
        hop = np.where((hop == seeds) | np.isin(hop, ids), robots, hop).astype(np.uint32)
        if kind != "robots only":
            ev = (lambda robots, ids: lambda k: (ids, 1.5 if k % 2 == 0 else 0.0, robots))(robots, ids)
        else:
            ev = (lambda robots, hop: lambda k: (None, None, hop if k % 2 == 0 else robots))(robots, hop)
        inputs.append((kind, phi, seeds, robots, ev, ids))
    records = [dict(plans=n, kind=kind, goals_near_the_patch=phi) for kind, phi, *_ in inputs]
    groups = [[k] for k in kinds] if args.sequential else [list(kinds)]
    for group in groups:
        ctxs = {kind: make(mesh, w, costs) for kind in group}
        for kind, c in ctxs.items():
            if kind.startswith("each@"):
                c.set_option("replan_repair_engine", int(kind[5:]))
        for rec, (kind, phi, seeds, robots, ev, ids) in zip(records, inputs):
            rec.update(run_case(ctxs, seeds, robots, ev, reps, warm))
            if kind != "robots only" and (warm + reps) % 2:            # leave the map as it was
                for c in ctxs.values():
                    c.update_costs(ids, np.zeros(ids.size, np.float32))
            print(json.dumps({k: rec[k] for k in rec if k in group or k in ("plans", "kind", "goals_near_the_patch")}), flush=True)
        for c in ctxs.values():
            c.close()
    result = dict(mesh="terrain(1000, 0.1, 2): 1 000 000 vertices, uploaded weights (edge_cost_factor 0)", offset=0.3,
                  method="wall ms per call, resident outputs on, one context per entry point on the same final map; medians of the repetitions after the warm-ups",
                  cases=[], crossing={})
    if (args.append or engines) and os.path.exists(args.out):
        with open(args.out) as fh:
            result = json.load(fh)
    if engines:                                                        # next to the old rows, not over them
        rows = result.setdefault("repair_engine_cases", [])
        done = {(r["kind"], r["goals_near_the_patch"]) for r in records}
        rows[:] = [c for c in rows if c["plans"] != n or (c["kind"], c["goals_near_the_patch"]) not in done]
        for rec in records:
            rec.update(repetitions=reps, warmups=warm, alternated=not args.sequential, d2d_copy_GBps=d2d)
            rows.append(rec)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        return
    if args.append and os.path.exists(args.out):
        done = {(r["kind"], r["goals_near_the_patch"]) for r in records}
        result["cases"] = [c for c in result["cases"] if c["plans"] != n or (c["kind"], c["goals_near_the_patch"]) not in done]
    for rec in records:
        rec.update(repetitions=reps, warmups=warm, alternated=not args.sequential)
        if rec["kind"] != "robots only":
            rec["each_over_batch"] = rec["each"]["ms"]["median"] / rec["batch"]["ms"]["median"]
            rec["each_over_fresh"] = rec["each"]["ms"]["median"] / rec["fresh"]["ms"]["median"]
        result["cases"].append(rec)
    result["crossing"][str(n)] = crossing([c for c in result["cases"] if c["plans"] == n and c["kind"] != "robots only"])
    found = [x for x in result["crossing"].values() if x is not None]
    result["replan_each_fresh_share"] = min(found) if found else 1.0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
