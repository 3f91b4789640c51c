"""Timing of fleet dispatch (mnav_fleet_costs, mnav_fleet_assign) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2).

The fields: one Dijkstra batch of 7 168 plans with a large offset (every wave runs out: every pair of a reachable vertex
is feasible), columns = the first m of them, robots on random vertices.

Matrix: mnav_fleet_costs for 1 024 x 64, 14 336 x 1 024 and 14 336 x 7 168 with every matrix output NULL but the two
nearest arrays (kernels by HIP events, whole call by the wall clock), and with the matrix downloaded; beside what the
library offered before: mnav_fleet_paths over the same pairs (1 024 x 64 only: it walks every chain) and the download of
the m fields plus a numpy gather (not at 7 168 columns: 29 GB).  Achieved gather rate = 8 bytes (dist and pred) per pair
over the kernel time.

Assignment: mnav_fleet_assign at N = 256, 1 024, 4 096 (square) and 14 336 x 7 168 with dispatch_tail_bidders at its
default and, up to 4 096, at 0 / 16 / 256 / 1 024; phases, rounds, the tail's share; beside the download of the matrix
and scipy.optimize.linear_sum_assignment on the same padded integer problem (up to N = 4 096; its absence is recorded).
A call that reaches --max-rounds is recorded as failed with the library's message.  Medians of alternated repetitions
after warm-up calls, with min and max: the matrix alternates device only / downloaded after two warm-ups; the assignment
warms every option value up once, then alternates them (3 rounds when a call takes 2 s or more, 1 from 8 s on); scipy
gets one warm-up run and 3 runs (1 at N = 4 096) alternated with a device call.

    python tools/dispatch_perf.py [--reps K] [--out FILE] [--mesh N] [--plans N] [--skip matrix,assign]"""
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

BIG_OFFSET = 1e9
QUANTUM = 1e-3


def spread(x):
    x = [float(v) for v in x]
    return dict(median=float(np.median(x)), min=min(x), max=max(x), runs=len(x))


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def save(res, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")


def matrix_case(ctx, mesh, n, m, reps, res):
    rng = np.random.default_rng(n + m)
    vtx = rng.integers(0, mesh.V, n).astype(np.uint32)
    slots = np.arange(m, dtype=np.uint32)
    for _ in range(2):
        ctx.fleet_costs(vtx, slots=slots, want_matrix=False)
    kern, w_dev, w_down = [], [], []
    for _ in range(reps):                                                    # alternated: matrix kept on the device / downloaded
        ms, _r = wall(lambda: ctx.fleet_costs(vtx, slots=slots, want_matrix=False))
        w_dev.append(ms); kern.append(ctx.dispatch_stats()["ms_costs"])
        ms, full = wall(lambda: ctx.fleet_costs(vtx, slots=slots))
        w_down.append(ms)
    st = ctx.dispatch_stats()
    k = float(np.median(kern))
    e = dict(robots=n, columns=m, pairs=n * m, outcome={x: st[x] for x in ("served", "beyond_field", "no_path", "invalid", "feasible")},
             ms_kernels=spread(kern), ms_call_nearest_only=spread(w_dev), ms_call_matrix_downloaded=spread(w_down), matrix_bytes=5 * n * m,
             pairs_per_s=n * m / (k * 1e-3), gather_bytes_per_s=8.0 * n * m / (k * 1e-3), store_bytes_per_s=5.0 * n * m / (k * 1e-3))
    if n * m <= 1 << 16:                                                     # mnav_fleet_paths over the same pairs
        ps, pv = np.tile(slots, n), np.repeat(vtx, m)
        ctx.fleet_paths(ps, pv, ids_cap=0)
        w, kk = [], []
        for _ in range(reps):
            ms, p = wall(lambda: ctx.fleet_paths(ps, pv, ids_cap=0)); w.append(ms); kk.append(ctx.fleet_stats()["ms_kernels"])
            ctx.fleet_costs(vtx, slots=slots, want_matrix=False)
        e["fleet_paths_over_the_pairs"] = dict(ms_call_wall=spread(w), ms_kernels=spread(kk), ids_walked=int(p["total"]),
                                               same_codes=bool(np.array_equal(p["codes"], full["codes"].ravel())),
                                               same_potential_bits=bool(np.array_equal(p["potential"].view(np.uint32), full["potential"].ravel().view(np.uint32))))
    if m <= 1024:                                                            # the fields come down, numpy gathers
        runs = []
        for _ in range(1 if m > 64 else 3):
            t0 = time.perf_counter()
            host = np.empty((n, m), np.float32)
            for j in range(m):
                host[:, j] = ctx.download_output("dist", j)[vtx]
            runs.append((time.perf_counter() - t0) * 1e3)
        rule4 = (full["codes"] == 0) & (full["potential"] > 0)                  # (a robot on a seed has potential 0 by rule 3)
        e["download_fields_and_numpy_gather"] = dict(ms_wall=spread(runs), bytes_down=4 * mesh.V * m, same_potential_bits=bool(np.array_equal(host[rule4], full["potential"][rule4])))
    else:
        e["download_fields_and_numpy_gather"] = dict(not_run="%d fields of %d floats: %.1f GB over PCIe" % (m, mesh.V, 4e-9 * mesh.V * m))
    res["matrix_%dx%d" % (n, m)] = e
    print("matrix", json.dumps(e), flush=True)


def host_solve(q, feasible):
    """scipy on the padded integer problem of the device; None when scipy does not import"""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return None
    n, m = q.shape
    N = max(n, m)
    M = N * (int(q[feasible].max()) if feasible.any() else 0) + 1
    cost = np.zeros((N, N), np.int64)
    cost[:n, :m] = np.where(feasible, q, M)
    r, c = linear_sum_assignment(cost)
    ok = (r < n) & (c < m)
    ok[ok] = feasible[r[ok], c[ok]]
    return int(ok.sum()), int(q[r[ok], c[ok]].sum())


def assign_case(ctx, mesh, n, m, reps, tails, max_rounds, scipy_max, res):
    rng = np.random.default_rng(7 * n + m)
    vtx = rng.integers(0, mesh.V, n).astype(np.uint32)
    slots = np.arange(m, dtype=np.uint32)
    ctx.set_option("dispatch_max_rounds", max_rounds)
    e = dict(robots=n, columns=m, N=max(n, m), quantum=QUANTUM, max_rounds=max_rounds, warmup_calls_per_setting=1, tails={})
    key_of = lambda tail: "default" if tail is None else str(tail)

    def call(tail):
        ctx.set_option("dispatch_tail_bidders", tail)
        t0 = time.perf_counter()
        try:
            out = ctx.fleet_assign(vtx, slots=slots, quantum=QUANTUM)
        except RuntimeError as err:
            return (time.perf_counter() - t0) * 1e3, None, str(err)
        return (time.perf_counter() - t0) * 1e3, out, ctx.dispatch_stats()

    first, live, warm_ms = None, [], {}
    for tail in tails:                                                       # one warm-up call per setting: buffers, code objects
        ms, out, st = call(tail)
        warm_ms[key_of(tail)] = ms
        if out is None:
            e["tails"][key_of(tail)] = dict(failed=st, ms_wall=ms)
            print("assign", n, m, key_of(tail), "failed", st, flush=True)
            continue
        first = first or out
        live.append(tail)
    k = reps if max(warm_ms.values()) < 2000 else (3 if max(warm_ms.values()) < 8000 else 1)
    w, dev = {key_of(t): [] for t in live}, {key_of(t): [] for t in live}
    last = {}
    for _ in range(k):                                                       # alternated over the settings
        for tail in live:
            ms, out, st = call(tail)
            w[key_of(tail)].append(ms); dev[key_of(tail)].append(st["ms_assign"]); last[key_of(tail)] = (out, st)
    for tail in live:
        out, st = last[key_of(tail)]
        e["tails"][key_of(tail)] = dict(ms_call_wall=spread(w[key_of(tail)]), ms_assign=spread(dev[key_of(tail)]), ms_warmup_call=warm_ms[key_of(tail)], ms_costs=st["ms_costs"],
                                        assigned=out["assigned"], total_q=out["total_q"], phases=st["phases"], rounds=st["rounds"], tail_rounds=st["tail_rounds"],
                                        tail_share=st["tail_rounds"] / max(1, st["rounds"]), bids=st["bids"],
                                        same_as_first=bool(np.array_equal(out["slot_of_robot"], first["slot_of_robot"])))
        print("assign", n, m, key_of(tail), json.dumps(e["tails"][key_of(tail)]), flush=True)
    ctx.set_option("dispatch_tail_bidders", None)
    ctx.set_option("dispatch_max_rounds", None)
    # the host's way: the matrix comes down, scipy solves (one warm-up, then runs alternated with a device call)
    if max(n, m) <= scipy_max:
        down, solve, best = [], [], None
        runs = 1 + (3 if max(n, m) <= 1024 else 1)
        for r in range(runs):
            ms_down, full = wall(lambda: ctx.fleet_costs(vtx, slots=slots))
            feasible = (full["codes"] == 0) & np.isfinite(full["potential"])
            q = np.where(feasible, np.floor(full["potential"].astype(np.float64) / QUANTUM + 0.5), -1).astype(np.int64)
            ms_solve, best = wall(lambda: host_solve(q, feasible))
            if best is None:
                break
            if r:
                down.append(ms_down); solve.append(ms_solve)
            if live:
                call(live[0])
        e["host"] = dict(scipy="not importable") if best is None else dict(
            ms_matrix_call_and_download=spread(down), ms_scipy=spread(solve), ms_total=spread([a + b for a, b in zip(down, solve)]), warmup=1, size=best[0], total_q=best[1],
            device_is_optimal=bool(first is not None and (first["assigned"], first["total_q"]) == best))
    else:
        e["host"] = dict(not_run="N above --scipy-max")
    res["assign_%dx%d" % (n, m)] = e
    print("assign", json.dumps(e), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--max-rounds", type=int, default=400000)
    ap.add_argument("--scipy-max", type=int, default=4096)
    ap.add_argument("--skip", default="", help="comma list of: matrix, assign, assign_big")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dispatch_perf.json"))
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), reps=args.reps, warmup=2, offset_of_the_fields=BIG_OFFSET, plans=args.plans)
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(args.plans)
        seeds = rng.choice(mesh.V, args.plans, replace=False).astype(np.uint32)
        targets = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        ms, r = wall(lambda: ctx.plan_dijkstra_batch(seeds, targets, BIG_OFFSET, path_cap=4096, want_stats=False))
        res["ms_plan_batch"], res["engine"] = ms, ctx.last_engine()
        del r
        big = min(args.plans, 7168)
        if "matrix" not in skip:
            for n, m in ((1024, 64), (14336, min(1024, big)), (14336, big)):
                matrix_case(ctx, mesh, n, m, args.reps, res)
                save(res, args.out)
        if "assign" not in skip:
            for N in (256, 1024, 4096):
                if N <= big:
                    assign_case(ctx, mesh, N, N, args.reps, (None, 0, 16, 256, 1024), args.max_rounds, args.scipy_max, res)
                    save(res, args.out)
            if "assign_big" not in skip:
                assign_case(ctx, mesh, 14336, big, 3, (None,), args.max_rounds, args.scipy_max, res)
    print(json.dumps(res))
    save(res, args.out)


if __name__ == "__main__":
    main()
