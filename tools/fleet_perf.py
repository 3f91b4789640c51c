"""Timing of the fleet calls (mnav_fleet_paths, mnav_fleet_walks) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2).

Paths: the resident fields of a 64-plan and a 7 168-plan Dijkstra batch with a large offset (every wave runs out, so
every robot is inside its field), robot i on plan i mod plans at a random vertex; mnav_fleet_paths for 1, 14 336 and
1 048 576 robots, kernels (HIP events) and whole call (wall clock of the C call that writes the ids, per-robot outputs
and the dense id copy included; the sizing call is timed separately), beside the two ways to the same paths without it:

  * mnav_plan_dijkstra_batch with one plan per robot, paths only (seed = the goal, target = the robot's vertex, offset
    0.3: the cheapest wave that still gives the path), for 1 and 14 336 robots;
  * mnav_download_output(slot, 1) for every used slot plus a numpy predecessor walk (all robots hop together).

The million robots are also timed sorted by slot (robots of one plan in adjacent lanes), to decide whether a
device-side order would pay.  Walks: 128 CVP plans, one robot per plan and 16 per plan, mnav_fleet_walks beside
mnav_backtrack_cvp_batch (once, and 16 calls).  Medians of alternated repetitions after warm-up calls, with min and max.

    python tools/fleet_perf.py [--reps K] [--out FILE] [--mesh N] [--big-plans N]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402

BIG_OFFSET = 1e9


def spread(x):
    x = [float(v) for v in x]
    return dict(median=float(np.median(x)), min=min(x), max=max(x), runs=len(x))


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


class RawPaths:
    """mnav_fleet_paths through the C ABI into buffers that exist before the clock starts (a caller's loop reuses its own)"""

    def __init__(self, ctx, slots, vtx, cap):
        n = len(slots)
        self.ctx, self.n, self.slots, self.vtx = ctx, n, np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.codes, self.vout, self.lens = (np.zeros(n, np.uint32) for _ in range(3))
        self.pot, self.off, self.ids = np.zeros(n, np.float32), np.zeros(n + 1, np.uint64), np.zeros(max(int(cap), 1), np.uint32)
        self.total = C.c_uint64(0)

    def __call__(self):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_paths(c._h, self.n, vp(self.slots), vp(self.vtx), None, vp(self.codes), vp(self.vout), vp(self.pot), vp(self.lens), vp(self.off),
                                   vp(self.ids), self.ids.size, C.byref(self.total))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, c._err())
        return ms, c.fleet_stats()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_walk(ctx, seeds, slots, vtx, keep_hops):
    """the paths without the fleet call: the predecessors of every used slot come down (one V-sized array at a time), its
    robots hop together"""
    ms_down = ms_walk = 0.0
    lens = np.zeros(len(slots), np.int64)
    hops = {} if keep_hops else None
    order = np.argsort(slots, kind="stable")
    bounds = np.flatnonzero(np.diff(slots[order].astype(np.int64), prepend=-1, append=-1))
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = order[lo:hi]
        s = int(slots[idx[0]])
        t0 = time.perf_counter()
        pred = ctx.download_output("pred", s)
        t1 = time.perf_counter()
        u = vtx[idx].astype(np.int64)
        active = np.flatnonzero(u != seeds[s])
        while active.size:
            u[active] = pred[u[active]]
            lens[idx[active]] += 1
            if hops is not None:
                for i in active:
                    hops.setdefault(int(idx[i]), []).append(int(u[i]))
            active = active[u[active] != seeds[s]]
        ms_down += (t1 - t0) * 1e3
        ms_walk += (time.perf_counter() - t1) * 1e3
    return ms_down, ms_walk, lens, hops


def paths_case(ctx, mesh, plans, sizes, reps, res):
    rng = np.random.default_rng(plans)
    seeds = rng.integers(0, mesh.V, plans).astype(np.uint32)
    targets = rng.integers(0, mesh.V, plans).astype(np.uint32)
    ms, r = wall(lambda: ctx.plan_dijkstra_batch(seeds, targets, BIG_OFFSET, path_cap=4096, want_stats=False))
    out = dict(ms_plan_batch=ms, engine=ctx.last_engine(), codes=sorted(set(int(c) for c in r["codes"])), sizes={})
    del r
    for n in sizes:
        slots = (np.arange(n) % plans).astype(np.uint32)
        vtx = rng.integers(0, mesh.V, n).astype(np.uint32)
        ms_size, first = wall(lambda: ctx.fleet_paths(slots, vtx, ids_cap=0))    # the sizing call: everything but the ids
        total = first["total"]
        k = reps if n <= 100000 else max(3, reps // 4)
        call = RawPaths(ctx, slots, vtx, total)
        for _ in range(2):
            call()
        w, kern = [], []
        for _ in range(k):
            ms, st = call()
            w.append(ms); kern.append(st["ms_kernels"])
        e = dict(robots=n, ids=total, mean_hops=total / n, outcome={x: st[x] for x in ("served", "beyond_field", "no_path", "invalid")},
                 ms_sizing_call=ms_size, ms_kernels=spread(kern), ms_call_wall=spread(w), bytes_down=int(4 * total + 24 * n))
        if n >= 100000:                                                      # robots of one plan in adjacent lanes
            order = np.argsort(slots, kind="stable")
            by_slot = RawPaths(ctx, slots[order], vtx[order], total)
            by_slot()
            w2, k2, w1, k1 = [], [], [], []
            for _ in range(k):                                               # alternated with the caller's order
                ms, st = by_slot(); w2.append(ms); k2.append(st["ms_kernels"])
                ms, st = call(); w1.append(ms); k1.append(st["ms_kernels"])
            del by_slot
            e["sorted_by_slot"] = dict(ms_kernels=spread(k2), ms_call_wall=spread(w2), ms_kernels_callers_order=spread(k1), ms_call_wall_callers_order=spread(w1))
        if n <= 20000 or plans <= 64:                                        # (a million robots over 7 168 plans: the same 7 168 downloads as for 14 336)
            # cheap cases (few slots, few robots): one warm-up, then 5 runs alternated with the fleet call; the others run ONCE
            cheap = n <= 20000 and np.unique(slots).size <= 64
            tot_ms = []
            if cheap:
                host_walk(ctx, seeds, slots, vtx, False)
                for _ in range(5):
                    call()
                    a, b, _l, _h = host_walk(ctx, seeds, slots, vtx, False)
                    tot_ms.append(a + b)
            ms_down, ms_walk, lens, hops = host_walk(ctx, seeds, slots, vtx, n <= 20000)
            tot_ms.append(ms_down + ms_walk)
            same = bool(np.array_equal(lens, call.lens))
            if hops is not None:
                same = same and all(np.array_equal(np.array(hops.get(i, [])[::-1], np.uint32), call.ids[int(call.off[i]): int(call.off[i + 1])]) for i in range(n))
            e["download_pred_and_numpy_walk"] = dict(ms_download=ms_down, ms_walk=ms_walk, ms_total=ms_down + ms_walk, slots_downloaded=int(np.unique(slots).size),
                                                     bytes_down=int(4 * mesh.V * np.unique(slots).size), same_paths=same, ms_total_runs=spread(tot_ms), warmup=1 if cheap else 0, alternated_with_fleet_call=bool(cheap),
                                                     note="ms_download / ms_walk / ms_total are the last run, which up to 20 000 robots also records every hop in Python for the comparison of the paths (slower: see ms_total_runs)" + ("" if cheap else "; a single run, no warm-up (every run downloads all used slots again)"))
        out["sizes"][str(n)] = e
        del call
        print("paths", plans, n, json.dumps(e), flush=True)
    # one plan per robot, paths only: this takes the resident fields, so it comes last
    ctx.set_resident_outputs(False)
    for n in [s for s in sizes if s <= 20000]:
        slots = (np.arange(n) % plans).astype(np.uint32)
        vtx = np.random.default_rng(n).integers(0, mesh.V, n).astype(np.uint32)
        ms = []
        for _ in range(1 + min(reps, 3)):
            t, r = wall(lambda: ctx.plan_dijkstra_batch(seeds[slots], vtx, 0.3, path_cap=4096, want_stats=False))
            ms.append(t)
        out["sizes"][str(n)]["one_plan_per_robot_paths_only"] = dict(ms_call_wall=spread(ms[1:]), engine=ctx.last_engine(), offset=0.3, warmup=1,
                                                                       note="not alternated with the fleet call: these plans take the resident fields, so they run at the end")
        print("one plan per robot", plans, n, json.dumps(out["sizes"][str(n)]["one_plan_per_robot_paths_only"]), flush=True)
        del r
    ctx.set_resident_outputs(True)
    res["paths_%d_plans" % plans] = out


def walks_case(ctx, mesh, reps, res, plans=128, per_plan=16, step=0.2, cap=4096):
    rng = np.random.default_rng(7)
    a = rng.uniform(0.1, 0.9, (plans, 2))
    ang = rng.uniform(0, 2 * np.pi, plans)
    b = np.clip(a + 0.12 * np.stack([np.cos(ang), np.sin(ang)], axis=1), 0.02, 0.98)
    off = np.array([0.023, 0.011, 0.0], np.float32)
    goal = np.array([mesh.xyz[mesh.vertex_at(*p)] for p in a], np.float32) + off
    t = np.linspace(1.0, 0.35, per_plan)                                     # robot 0 of a plan stands at the plan's own target
    start = np.array([[mesh.xyz[mesh.vertex_at(*(a[p] + t[k] * (b[p] - a[p])))] for k in range(per_plan)] for p in range(plans)], np.float32) + off
    gf = ctx.locate(goal)["face"]
    sf = ctx.locate(start.reshape(-1, 3))["face"].reshape(plans, per_plan)
    ms, r = wall(lambda: ctx.plan_cvp_batch(goal, gf, sf[:, 0], 0.3))
    out = dict(plans=plans, ms_plan_cvp_batch=ms, codes=sorted(set(int(c) for c in r["codes"])), step_width=step, walk_cap=cap)
    for k in (1, per_plan):
        pos = np.ascontiguousarray(start[:, :k].transpose(1, 0, 2).reshape(-1, 3))       # robot-major: call j of the old API is rows j * plans ...
        face = np.ascontiguousarray(sf[:, :k].T.reshape(-1))
        slots = np.tile(np.arange(plans, dtype=np.uint32), k)
        first = ctx.fleet_walks(slots, goal, gf, pos, face, step_width=step, walk_cap=cap)
        total = first["total"]

        def new():
            return ctx.fleet_walks(slots, goal, gf, pos, face, step_width=step, walk_cap=cap, entries_cap=max(total, 1))

        def old():
            return [ctx.backtrack_cvp_batch(goal, gf, pos[j * plans: (j + 1) * plans], face[j * plans: (j + 1) * plans], step_width=step, cap=cap) for j in range(k)]

        o, n_ = old(), new()
        same = all(o[j][p][0] == n_["status"][j * plans + p] and
                   np.array_equal(o[j][p][1].view(np.uint32), n_["positions"][int(n_["offsets"][j * plans + p]): int(n_["offsets"][j * plans + p + 1])].view(np.uint32))
                   for j in range(k) for p in range(plans))
        wn, kn, wo = [], [], []
        for _ in range(reps):
            ms, _r = wall(new); wn.append(ms); kn.append(ctx.fleet_stats()["ms_kernels"])
            ms, _r = wall(old); wo.append(ms)
        st = ctx.fleet_stats()
        out["%d_per_plan" % k] = dict(robots=plans * k, entries=total, reached=int((n_["status"] == 1).sum()), same_as_backtrack_cvp_batch=bool(same),
                                      fleet_walks_ms_kernels=spread(kn), fleet_walks_ms_call_wall=spread(wn), backtrack_cvp_batch_calls=k,
                                      backtrack_cvp_batch_ms_wall=spread(wo))
        print("walks", k, json.dumps(out["%d_per_plan" % k]), flush=True)
    res["walks"] = out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--small-plans", type=int, default=64)
    ap.add_argument("--big-plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,1048576")
    ap.add_argument("--skip", default="", help="comma list of: small, big, walks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_perf.json"))
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    sizes = [int(s) for s in args.sizes.split(",")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), reps=args.reps, warmup=2, offset_of_the_fields=BIG_OFFSET)
    with capi.MnavContext(0) as ctx:
        vn = None
        if "walks" not in skip:                                              # the CVP planner needs the vertex normals
            from oracle import oracle as O
            vn = O.OracleMesh(mesh.xyz, mesh.faces).vertex_normals()
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, vn)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        if "walks" not in skip:
            walks_case(ctx, mesh, args.reps, res)
        if "small" not in skip:
            paths_case(ctx, mesh, args.small_plans, sizes, args.reps, res)
        if "big" not in skip:
            paths_case(ctx, mesh, args.big_plans, sizes, args.reps, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
