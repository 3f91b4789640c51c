"""Timing of timed fleet traffic (mnav_fleet_timed_traffic) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the
resident fields of a 7 168-plan Dijkstra batch with a large offset (every wave runs out: every robot is inside its field),
with the robots of tools/traffic_perf.py: 1, 14 336 and 1 048 576 robots at random vertices, robot i on plan i mod 7 168,
and 1 048 576 robots all on ONE plan (every contributor's last visit on one vertex).  64 windows; tau = twice the largest
potential of plan 0 over the windows; random departures in the first ten windows, paces in 0.5 .. 1.5, keys = indices.

Per case, alternated in one process after warm-up calls, medians with (min .. max):
  timed      mnav_fleet_timed_traffic -- its kernels (HIP events) and the whole call (wall clock of the C call into buffers
             that exist before the clock starts);
  traffic    mnav_fleet_traffic over the same robots: the parent's nearest capability (no time axis);
  host       what the parent offers for the same cells: mnav_fleet_paths with the ids downloaded, the used fields
             downloaded (V floats per plan), and the binning in numpy.  Run where a case uses ONE field (one robot, and the
             million robots on one plan); the cases that use all 7 168 fields would download 28.7 GB of potentials and are
             not run.  The host's cells are compared with the device's.

    python tools/timed_traffic_perf.py [--reps K] [--out FILE] [--mesh N] [--plans N] [--sizes a,b,c] [--windows B]"""
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
from tools.traffic_perf import NODES, RawTraffic, spread, vp  # noqa: E402

BIG_OFFSET = 1e9
FREE = 4
F = np.float32


class RawTimed:
    """mnav_fleet_timed_traffic through the C ABI into buffers that exist before the clock starts"""

    def __init__(self, ctx, slots, vtx, depart, pace, windows, tau):
        n = len(slots)
        self.ctx, self.n, self.windows, self.tau = ctx, n, windows, tau
        self.slots, self.vtx = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.depart, self.pace = np.ascontiguousarray(depart, F), np.ascontiguousarray(pace, F)
        self.ints = [np.zeros(n, np.uint32) for _ in range(6)]
        self.pot, self.ft = np.zeros(n, F), np.zeros(n, F)

    def __call__(self):
        c, i = self.ctx, self.ints
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_timed_traffic(c._h, self.n, vp(self.slots), vp(self.vtx), None, None, vp(self.depart), vp(self.pace), None, self.windows, self.tau, FREE, 0,
                                           vp(i[0]), vp(i[1]), vp(self.pot), vp(i[2]), vp(i[3]), vp(i[4]), vp(i[5]), vp(self.ft))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, c._err())
        return ms, c.timed_traffic_stats()


class HostCells:
    """the parent's way to the same cells for robots of ONE plan: the ids and the plan's potentials come down, numpy bins"""

    def __init__(self, ctx, slots, vtx, depart, pace, windows, tau, total, V):
        n = len(slots)
        assert (slots == slots[0]).all()
        self.ctx, self.n, self.V, self.B, self.tau, self.plan = ctx, n, V, windows, F(tau), int(slots[0])
        self.slots, self.vtx = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.depart, self.pace = np.ascontiguousarray(depart, F), np.ascontiguousarray(pace, F)
        self.codes, self.vout, self.lens = (np.zeros(n, np.uint32) for _ in range(3))
        self.pot, self.off, self.ids = np.zeros(n, F), np.zeros(n + 1, np.uint64), np.zeros(max(int(total), 1), np.uint32)
        self.total = C.c_uint64(0)
        self.cells = None

    def bin(self, cells, u, P, dep, pc):
        with np.errstate(over="ignore"):
            t = dep + np.fmax(P - self.dist[u], F(0)) * pc
            q = t / self.tau
        inside = q < F(self.B)
        idx = u[inside].astype(np.int64) * self.B + q[inside].astype(np.int64)
        cells += np.bincount(idx, minlength=cells.size)

    def __call__(self):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_paths(c._h, self.n, vp(self.slots), vp(self.vtx), None, vp(self.codes), vp(self.vout), vp(self.pot), vp(self.lens), vp(self.off),
                                   vp(self.ids), self.ids.size, C.byref(self.total))
        t1 = time.perf_counter()
        assert rc == 0, (rc, c._err())
        self.dist = c.download_output("dist", self.plan)
        t2 = time.perf_counter()
        cells = np.zeros(self.V * self.B, np.int64)
        off = self.off.astype(np.int64)
        step = max(1, (1 << 25) // max(1, int(self.lens.max())))               # robots per piece: about 2^25 ids
        for a in range(0, self.n, step):
            b = min(self.n, a + step)
            reps = self.lens[a:b].astype(np.int64)
            self.bin(cells, self.ids[off[a]:off[b]], np.repeat(self.pot[a:b], reps), np.repeat(self.depart[a:b], reps), np.repeat(self.pace[a:b], reps))
        on = (self.codes == 0) & np.isfinite(self.pot)
        self.bin(cells, self.vtx[on], self.pot[on], self.depart[on], self.pace[on])                  # the robots' own vertices
        self.cells = cells.astype(np.uint32)
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def case(ctx, V, name, slots, vtx, windows, tau, reps, res, rng):
    n = len(slots)
    depart, pace = (rng.random(n) * 10 * tau).astype(F), (0.5 + rng.random(n)).astype(F)
    first = ctx.fleet_paths(slots, vtx, ids_cap=0)                           # the sizing call: everything but the ids
    total = int(first["total"])
    heavy = n > 100000
    k = max(3, reps // 4) if heavy else reps
    timed, plain = RawTimed(ctx, slots, vtx, depart, pace, windows, tau), RawTraffic(ctx, slots, vtx)
    one_field = bool((slots == slots[0]).all())
    host = HostCells(ctx, slots, vtx, depart, pace, windows, tau, total, V) if one_field else None
    timed(); plain()
    tw, tk, pw, pk, hp, hf, hb = [], [], [], [], [], [], []
    for r in range(k):                                                       # alternated: timed, untimed, the host's way
        ms, st = timed()
        tw.append(ms); tk.append(st["ms_kernels"])
        ms, ps = plain()
        pw.append(ms); pk.append(ps["ms_kernels"])
        if host is not None and (not heavy or r < 2):
            a, b, c = host()
            hp.append(a); hf.append(b); hb.append(c)
    ms, st = timed()
    e = dict(robots=n, ids=total, windows=windows, tau=float(tau), free_count=FREE,
             stats={x: st[x] for x in ("contributing", "adds", "beyond_horizon", "total_weight", "occupied_cells", "over_cells", "largest_cell", "yielding")},
             timed_ms_kernels=spread(tk), timed_ms_call_wall=spread(tw), traffic_ms_kernels=spread(pk), traffic_ms_call_wall=spread(pw),
             visits_per_second_kernels=(st["adds"] + st["beyond_horizon"]) / (1e-3 * float(np.median(tk))) if np.median(tk) > 0 else None)
    if host is not None:
        same = bool(np.array_equal(ctx.timed_traffic_download()["cells"].ravel(), host.cells))
        e["host"] = dict(fleet_paths_ids_down_ms=spread(hp), field_down_ms=spread(hf), numpy_binning_ms=spread(hb),
                         total_ms=spread([a + b + c for a, b, c in zip(hp, hf, hb)]), bytes_down=int(4 * total + 24 * n + 4 * V), same_cells=same)
    else:
        fields = len(set(int(s) for s in slots))
        e["host"] = dict(not_run="uses %d fields: %.1f GB of potentials would come down" % (fields, 4e-9 * V * fields))
    res["cases"][name] = e
    print("case", name, json.dumps(e), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,1048576")
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_traffic_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    V, plans, B = mesh.V, args.plans, args.windows
    sizes = [int(s) for s in args.sizes.split(",")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=plans, reps=args.reps, windows=B, offset_of_the_fields=BIG_OFFSET, cell_bytes=8 * V * B, cases={})
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.layer_upload(0, np.zeros(V, np.float32))                         # the map of tools/traffic_perf.py: the same fields
        ctx.layer_timed_traffic(1)
        ctx.map_configure(NODES, 2, 1.0)
        ctx.map_compute()
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(plans)
        seeds, targets = rng.integers(0, V, plans).astype(np.uint32), rng.integers(0, V, plans).astype(np.uint32)
        t0 = time.perf_counter()
        r = ctx.plan_dijkstra_batch(seeds, targets, BIG_OFFSET, path_cap=4096, want_stats=False)
        res["ms_plan_batch"] = (time.perf_counter() - t0) * 1e3
        res["engine"] = ctx.last_engine()
        res["codes"] = sorted(set(int(c) for c in r["codes"]))
        del r
        d0 = ctx.download_output("dist", 0)
        tau = float(F(2.0 * float(d0[np.isfinite(d0)].max()) / B))
        for n in sizes:
            case(ctx, V, str(n), (np.arange(n) % plans).astype(np.uint32), rng.integers(0, V, n).astype(np.uint32), B, tau, args.reps, res, rng)
        n = max(sizes)
        case(ctx, V, "%d_on_one_plan" % n, np.zeros(n, np.uint32), rng.integers(0, V, n).astype(np.uint32), B, tau, args.reps, res, rng)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
