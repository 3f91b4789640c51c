"""Timing of fleet traffic (mnav_fleet_traffic, mnav_map_traffic) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over
the resident fields of a 7 168-plan Dijkstra batch with a large offset (every wave runs out: every robot is inside its
field).  A static zero layer and the traffic layer sit under one COMBINE_AVG node of the layer graph, edge_cost_factor 1.

Counts: 1, 14 336 and 1 048 576 robots at random vertices, robot i on plan i mod 7 168, and 1 048 576 robots all on ONE
plan (every contributor's last add on one address).  mnav_fleet_traffic -- kernels (HIP events) and whole call (wall clock
of the C call into buffers that exist before the clock starts) -- with traffic_combine on (the keys traffic_ms_*) and off
(the keys combine_off_ms_*: the library's default), alternated, beside what the library offered before, in the same process: mnav_fleet_paths with the ids downloaded plus np.bincount over them and
over the contributors' own vertices.  The two count arrays are compared.
Layer: mnav_map_traffic beside the host's way from host counts: the cost rule in numpy plus mnav_map_update_layer with V
costs.  The two alternate with two gains, so every call changes the cost of every occupied vertex.
Medians of alternated repetitions after warm-up calls, with min and max.

    python tools/traffic_perf.py [--reps K] [--out FILE] [--mesh N] [--plans N] [--sizes a,b,c]"""
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
NODES = [dict(layer=0, kind="input"), dict(layer=1, kind="input"), dict(layer=2, kind="avg", inputs=[0, 1], weights=[1.0, 1.0])]
FREE, CAP, GAINS = 4, 0.5, (0.001, 0.002)


def spread(x):
    x = [float(v) for v in x]
    return dict(median=float(np.median(x)), min=min(x), max=max(x), runs=len(x))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class RawTraffic:
    """mnav_fleet_traffic through the C ABI into buffers that exist before the clock starts"""

    def __init__(self, ctx, slots, vtx):
        n = len(slots)
        self.ctx, self.n, self.slots, self.vtx = ctx, n, np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.codes, self.vout, self.pot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)

    def __call__(self):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_traffic(c._h, self.n, vp(self.slots), vp(self.vtx), None, None, 0, vp(self.codes), vp(self.vout), vp(self.pot))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, c._err())
        return ms, c.traffic_stats()


class HostCounts:
    """what the library offered before: mnav_fleet_paths with the ids downloaded, then the histogram on the host"""

    def __init__(self, ctx, slots, vtx, total, V):
        n = len(slots)
        self.ctx, self.n, self.V, self.slots, self.vtx = ctx, n, V, np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        self.codes, self.vout, self.lens = (np.zeros(n, np.uint32) for _ in range(3))
        self.pot, self.off, self.ids = np.zeros(n, np.float32), np.zeros(n + 1, np.uint64), np.zeros(max(int(total), 1), np.uint32)
        self.total = C.c_uint64(0)
        self.counts = None

    def __call__(self):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_paths(c._h, self.n, vp(self.slots), vp(self.vtx), None, vp(self.codes), vp(self.vout), vp(self.pot), vp(self.lens), vp(self.off),
                                   vp(self.ids), self.ids.size, C.byref(self.total))
        t1 = time.perf_counter()
        assert rc == 0, (rc, c._err())
        total = int(self.total.value)
        counts = np.zeros(self.V, np.int64)
        for lo in range(0, total, 1 << 26):                                  # (in pieces: np.bincount widens its input to 8 bytes per id)
            counts += np.bincount(self.ids[lo: min(total, lo + (1 << 26))], minlength=self.V)
        on = (self.codes == 0) & np.isfinite(self.pot)
        counts += np.bincount(self.vtx[on], minlength=self.V)
        self.counts = counts.astype(np.uint32)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def host_cost(counts, free_count, gain, cap):
    e = np.where(counts > free_count, counts - np.uint32(free_count), 0).astype(np.uint32)
    return np.where(e == 0, np.float32(0), np.minimum(e.astype(np.float32) * np.float32(gain), np.float32(cap))).astype(np.float32)


def counts_case(ctx, V, name, slots, vtx, reps, res):
    first = ctx.fleet_paths(slots, vtx, ids_cap=0)                           # the sizing call: everything but the ids
    total = int(first["total"])
    heavy = len(slots) > 100000
    k = max(3, reps // 4) if heavy else reps
    dev, host = RawTraffic(ctx, slots, vtx), HostCounts(ctx, slots, vtx, total, V)
    for combine in (1, 0):
        ctx.set_option("traffic_combine", combine)
        dev()
    host()
    w = {1: [], 0: []}
    kern = {1: [], 0: []}
    paths_ms, hist_ms = [], []
    for r in range(k):                                                       # alternated: combine on, combine off, the host's way
        for combine in (1, 0):
            ctx.set_option("traffic_combine", combine)
            ms, st = dev()
            w[combine].append(ms); kern[combine].append(st["ms_kernels"])
        if not heavy or r < 3:
            a, b = host()
            paths_ms.append(a); hist_ms.append(b)
    ctx.set_option("traffic_combine", None)
    ms, st = dev()
    same = bool(np.array_equal(ctx.traffic_download(), host.counts))
    e = dict(robots=len(slots), ids=total, stats={x: st[x] for x in ("contributing", "adds", "total_weight", "occupied", "peak")},
             traffic_ms_kernels=spread(kern[1]), traffic_ms_call_wall=spread(w[1]),
             combine_off_ms_kernels=spread(kern[0]), combine_off_ms_call_wall=spread(w[0]),
             adds_per_second_kernels=st["adds"] / (1e-3 * float(np.median(kern[1]))) if np.median(kern[1]) > 0 else None,
             before=dict(fleet_paths_ids_down_ms=spread(paths_ms), bincount_ms=spread(hist_ms), total_ms=spread([a + b for a, b in zip(paths_ms, hist_ms)]),
                         bytes_down=int(4 * total + 24 * len(slots))),
             same_counts=same)
    res["counts"][name] = e
    print("counts", name, json.dumps(e), flush=True)
    return host.counts


def map_case(ctx, V, counts, reps, res):
    """the counts of the last traffic call are resident; `counts` is the host's copy of them"""
    ids = np.arange(V, dtype=np.uint32)
    dev_ms, dev_dev, host_rule, host_call, changed = [], [], [], [], []
    ctx.map_traffic(1, FREE, GAINS[1], CAP)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        a = ctx.map_traffic(1, FREE, GAINS[0], CAP)
        t1 = time.perf_counter()
        cost = host_cost(counts, FREE, GAINS[1], CAP)
        t2 = time.perf_counter()
        b = ctx.map_update_layer(1, ids, cost)
        t3 = time.perf_counter()
        if r:                                                                # (the first pair is the warm-up)
            dev_ms.append((t1 - t0) * 1e3); dev_dev.append(a["stats"]["ms_total"]); host_rule.append((t2 - t1) * 1e3); host_call.append((t3 - t2) * 1e3)
            changed.append((int(a["changed"].size), int(b["changed"].size)))
    layer = ctx.layer_download(1)[0]
    same = bool(np.array_equal(layer.view(np.uint32), host_cost(counts, FREE, GAINS[1], CAP).view(np.uint32)))
    ctx.map_traffic(1, FREE, GAINS[0], CAP)
    same = same and bool(np.array_equal(ctx.layer_download(1)[0].view(np.uint32), host_cost(counts, FREE, GAINS[0], CAP).view(np.uint32)))
    e = dict(free_count=FREE, gains=GAINS, cap=CAP, default_changed=changed[-1], map_traffic_ms_call_wall=spread(dev_ms), map_traffic_ms_device=spread(dev_dev),
             before=dict(numpy_rule_ms=spread(host_rule), map_update_layer_ms=spread(host_call), total_ms=spread([x + y for x, y in zip(host_rule, host_call)]),
                         bytes_up=int(8 * V)), same_layer=same)
    res["map_traffic"] = e
    print("map", json.dumps(e), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    V, plans = mesh.V, args.plans
    sizes = [int(s) for s in args.sizes.split(",")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=plans, reps=args.reps, offset_of_the_fields=BIG_OFFSET, counts={},
               variants=dict(combine="traffic_combine: a wave whose contributors all end on one vertex issues one add (on / off in every case)",
                             lds_merge="lanes meeting on one (slot, vertex) at one hop hand their weight over through LDS: not tried"))
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.layer_upload(0, np.zeros(V, np.float32))
        ctx.layer_traffic(1)
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
        counts = None
        for n in sizes:
            counts = counts_case(ctx, V, str(n), (np.arange(n) % plans).astype(np.uint32), rng.integers(0, V, n).astype(np.uint32), args.reps, res)
        n = max(sizes)
        counts = counts_case(ctx, V, "%d_on_one_plan" % n, np.zeros(n, np.uint32), rng.integers(0, V, n).astype(np.uint32), args.reps, res)
        map_case(ctx, V, counts, args.reps, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
