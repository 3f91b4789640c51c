"""Timing of the fleet schedule (mnav_fleet_schedule) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the resident
fields of a 7 168-plan Dijkstra batch with a large offset (every wave runs out: every robot is inside its field), with the
robots of tools/timed_traffic_perf.py: robot i at a random vertex on plan i mod 7 168.  64 windows; tau = twice the largest
potential of plan 0 over the windows; random departures in the first ten windows, paces in 0.5 .. 1.5, keys = indices;
capacity 1, max_delay = windows - 1, no flag (arrivals at the seeds are rationed too).

Per case, alternated in one process after warm-up calls, medians with (min .. max):
  schedule   mnav_fleet_schedule -- its kernels (HIP events) and the whole call (wall clock of the C call into buffers
             that exist before the clock starts); rounds, committed and NO_SLOT robots, claims;
  stagger    what the parent offers: the loop "mnav_fleet_timed_traffic, depart[i] += tau where yield_hops[i] > 0" with
             free_count = capacity, run for as many rounds as fit into the wall time the schedule call took (at least one);
             the over cells and yielding robots it is left with.
  chunks     the schedule call with schedule_chunk_rounds = 1, 4, 8, 16, 64 and with schedule_clean_fill = 1 (alternated).

Kernel by kernel: run `--profile N` (one case: a warm-up and `--reps` calls, nothing else) under
`rocprofv3 --kernel-trace --stats` in a run of its own and pass the resulting kernel statistics with `--kernel-stats CSV
--into FILE`: per k_schedule_* kernel the milliseconds per round, and for the probe the bytes of cell rows read per second
(64 lanes x 4 bytes per hop and block of candidates -- an upper bound: lanes beyond max_delay and lanes that stopped fitting
still load).

    python tools/schedule_perf.py [--reps K] [--out FILE] [--mesh N] [--plans N] [--sizes a,b,c] [--windows B]
    python tools/schedule_perf.py --profile N
    python tools/schedule_perf.py --kernel-stats CSV --into FILE --rounds R --calls K"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402
from tools.timed_traffic_perf import BIG_OFFSET, RawTimed  # noqa: E402
from tools.traffic_perf import NODES, spread, vp  # noqa: E402

CAPACITY = 1
F = np.float32
COUNTS = ("contributing", "committed", "no_slot", "open", "rounds", "delayed", "max_delay_used", "claims", "committed_visits")


class RawSchedule:
    """mnav_fleet_schedule through the C ABI into buffers that exist before the clock starts"""

    def __init__(self, ctx, slots, vtx, depart, pace, windows, tau):
        n = len(slots)
        self.ctx, self.n, self.windows, self.tau = ctx, n, windows, tau
        self.slots, self.vtx = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.depart, self.pace = np.ascontiguousarray(depart, F), np.ascontiguousarray(pace, F)
        self.ints = [np.zeros(n, np.uint32) for _ in range(5)]
        self.pot, self.out = np.zeros(n, F), np.zeros(n, F)

    def __call__(self):
        c, i = self.ctx, self.ints
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_schedule(c._h, self.n, vp(self.slots), vp(self.vtx), None, None, vp(self.depart), vp(self.pace), None, self.windows, self.tau, CAPACITY,
                                      self.windows - 1, 0, 0, 0, vp(i[0]), vp(i[1]), vp(self.pot), vp(i[2]), vp(i[3]), vp(self.out), vp(i[4]))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, c._err())
        return ms, c.schedule_stats()


def stagger(ctx, slots, vtx, depart, pace, windows, tau, budget_ms):
    """the parent's loop for `budget_ms` of wall time (at least one round): (rounds, over cells, yielding robots, ms)"""
    timed = RawTimed(ctx, slots, vtx, depart.copy(), pace, windows, tau)
    t0 = time.perf_counter()
    rounds = 0
    while True:
        c, i = timed.ctx, timed.ints
        rc = c._L.mnav_fleet_timed_traffic(c._h, timed.n, vp(timed.slots), vp(timed.vtx), None, None, vp(timed.depart), vp(timed.pace), None, windows, tau, CAPACITY, 0,
                                           vp(i[0]), vp(i[1]), vp(timed.pot), vp(i[2]), vp(i[3]), vp(i[4]), vp(i[5]), vp(timed.ft))
        assert rc == 0, (rc, c._err())
        rounds += 1
        st = c.timed_traffic_stats()
        if (time.perf_counter() - t0) * 1e3 >= budget_ms:
            return rounds, st["over_cells"], st["yielding"], (time.perf_counter() - t0) * 1e3
        timed.depart[i[3] > 0] += F(tau)                                      # yield_hops > 0: leave one window later


def robots_of(n, plans, V, windows, tau, rng):
    return ((np.arange(n) % plans).astype(np.uint32), rng.integers(0, V, n).astype(np.uint32), (rng.random(n) * 10 * tau).astype(F), (0.5 + rng.random(n)).astype(F))


def case(ctx, name, slots, vtx, depart, pace, windows, tau, reps, res):
    n = len(slots)
    k = max(3, reps // 4) if n > 100000 else reps
    sched = RawSchedule(ctx, slots, vtx, depart, pace, windows, tau)
    sched()
    sw, sk, left = [], [], []
    for _ in range(k):                                                       # alternated: the schedule, then the loop for the same wall time
        ms, st = sched()
        sw.append(ms); sk.append(st["ms_kernels"])
        left.append(stagger(ctx, slots, vtx, depart, pace, windows, tau, ms))
    ms, st = sched()
    cells = ctx.timed_traffic_stats()
    e = dict(robots=n, windows=windows, tau=float(tau), capacity=CAPACITY, max_delay=windows - 1, stats={x: st[x] for x in COUNTS},
             cells_after=dict(over_cells=cells["over_cells"], largest_cell=cells["largest_cell"], occupied_cells=cells["occupied_cells"]),
             schedule_ms_kernels=spread(sk), schedule_ms_call_wall=spread(sw),
             stagger_same_wall=dict(rounds=spread([x[0] for x in left]), over_cells=spread([x[1] for x in left]), yielding=spread([x[2] for x in left]),
                                    ms=spread([x[3] for x in left])))
    variants = [("schedule_chunk_rounds", c) for c in (1, 4, 8, 16, 64)] + [("schedule_clean_fill", 1)]
    times = {v: [] for v in variants}
    for _ in range(k):                                                       # alternated over the variants
        for v in variants:
            ctx.set_option(v[0], v[1])
            ms, st2 = sched()
            ctx.set_option(v[0], None)
            assert {x: st2[x] for x in COUNTS} == {x: st[x] for x in COUNTS}, v
            times[v].append(ms)
    e["variants_ms_call_wall"] = {"%s=%d" % v: spread(t) for v, t in times.items()}
    res["cases"][name] = e
    print("case", name, json.dumps(e), flush=True)


def setup(ctx, mesh, plans, B):
    V = mesh.V
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
    ctx.layer_upload(0, np.zeros(V, np.float32))                             # the map of tools/traffic_perf.py: the same fields
    ctx.layer_timed_traffic(1)
    ctx.map_configure(NODES, 2, 1.0)
    ctx.map_compute()
    ctx.set_resident_outputs(True)
    rng = np.random.default_rng(plans)
    seeds, targets = rng.integers(0, V, plans).astype(np.uint32), rng.integers(0, V, plans).astype(np.uint32)
    t0 = time.perf_counter()
    r = ctx.plan_dijkstra_batch(seeds, targets, BIG_OFFSET, path_cap=4096, want_stats=False)
    ms = (time.perf_counter() - t0) * 1e3
    codes = sorted(set(int(c) for c in r["codes"]))
    del r
    d0 = ctx.download_output("dist", 0)
    return rng, float(F(2.0 * float(d0[np.isfinite(d0)].max()) / B)), ms, codes


def merge_kernel_stats(path, into, rounds, calls):
    """per k_schedule_* kernel of a rocprofv3 --stats table: calls, total and milliseconds per round that ran"""
    res = json.load(open(into))
    rows = {}
    for r in csv.DictReader(open(path)):
        for k in ("k_schedule_init", "k_schedule_probe", "k_schedule_claim", "k_schedule_decide", "k_schedule_commit", "k_schedule_next", "k_timed_peak", "k_fleet_len"):
            if k + "(" in r["Name"]:
                rows[k] = dict(launches=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) * 1e-6, ms_per_round=float(r["TotalDurationNs"]) * 1e-6 / (rounds * calls),
                               min_us=float(r["MinNs"]) * 1e-3, max_us=float(r["MaxNs"]) * 1e-3)
    res["kernel_stats"] = dict(rounds_per_call=rounds, calls=calls, kernels=rows,
                               note="launches include the rounds enqueued after the loop had ended (they return at once); ms_per_round divides by the rounds that ran")
    with open(into, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res["kernel_stats"]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,262144")
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--into", default="")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schedule_perf.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.into or args.out, args.rounds, args.calls)
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    V, plans, B = mesh.V, args.plans, args.windows
    with capi.MnavContext(0) as ctx:
        rng, tau, ms_plan, codes = setup(ctx, mesh, plans, B)
        if args.profile:                                                     # for the profiler: one case, nothing else
            sched = RawSchedule(ctx, *robots_of(args.profile, plans, V, B, tau, rng), B, tau)
            sched()
            for _ in range(args.reps):
                ms, st = sched()
            print(json.dumps(dict(profile=args.profile, calls=args.reps + 1, stats={x: st[x] for x in COUNTS})))
            return
        res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=plans, reps=args.reps, windows=B, offset_of_the_fields=BIG_OFFSET, bytes=20 * V * B, ms_plan_batch=ms_plan,
                   engine=ctx.last_engine(), codes=codes, cases={})
        for n in (int(s) for s in args.sizes.split(",")):
            case(ctx, str(n), *robots_of(n, plans, V, B, tau, rng), B, tau, args.reps, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
