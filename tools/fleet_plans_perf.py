"""Timing of the fleet plans (mnav_fleet_plans, mnav_fleet_walk_plans) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2).

Plans: the resident fields of a 64-plan and a 7 168-plan Dijkstra batch planned with offset 1e9 (every wave runs out, so
every robot is inside its field), robot i on plan i mod plans at a random vertex; mnav_fleet_plans for 1, 14 336 and
131 072 robots: kernels (HIP events, mnav_fleet_stats) and the whole C call (wall clock: per-robot outputs and the dense
pose copy included; buffers exist before the clock starts), beside what a caller does without it: mnav_fleet_paths, then
the host pose loop of mnav_planner_host.hpp (vertex_path_poses with calculatePoseFromPosition) on ONE host thread over
host copies of xyz and the vertex normals.  The two are alternated; medians with min and max after 2 warm-ups; the poses
and costs of the two ways are compared bit for bit.
The pose kernel alone is not timed here (the library reports its kernels together): run this tool under
`rocprofv3 --kernel-trace --stats` in a run of its own and read k_plan_poses there; `--copy` times a plain
device-to-device hipMemcpy of the pose bytes of every size in the same run, the rate to hold the kernel against.
Walk plans: 128 CVP plans, 16 robots per plan, mnav_fleet_walk_plans beside mnav_fleet_walks + face_path_poses.

    python tools/fleet_plans_perf.py [--reps K] [--out FILE] [--mesh N] [--big-plans N] [--sizes a,b,c] [--skip small,big,walks]"""
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

from mesh_navigation_amd import capi, meshgen, planner  # noqa: E402
from oracle import oracle as O  # noqa: E402

BIG_OFFSET = 1e9


def spread(x):
    x = [float(v) for v in x]
    return dict(median=float(np.median(x)), min=min(x), max=max(x), runs=len(x))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b, chunk=1 << 24):
    """bit for bit, a NaN matching any NaN; in chunks (the largest case holds 4 GB of poses twice)"""
    a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
    if a.shape != b.shape:
        return False
    for lo in range(0, a.size, chunk):
        x, y = a[lo: lo + chunk], b[lo: lo + chunk]
        nan = np.isnan(y)
        if not (np.array_equal(np.isnan(x), nan) and np.array_equal(x.view(np.uint64)[~nan], y.view(np.uint64)[~nan])):
            return False
    return True


def adapter_lib():
    L = planner._load()
    u64 = C.c_uint64
    L.mnav_adapter_host_vertex_path_poses.restype = u64
    L.mnav_adapter_host_vertex_path_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    L.mnav_adapter_host_face_path_poses.restype = u64
    L.mnav_adapter_host_face_path_poses.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    return L


class Hip:
    """a plain device-to-device hipMemcpy of `nbytes`, timed with the host clock around copy + synchronise"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipFree.argtypes = [C.c_void_p]

    def copy_ms(self, nbytes, reps):
        a, b = C.c_void_p(), C.c_void_p()
        assert self.L.hipMalloc(C.byref(a), nbytes) == 0 and self.L.hipMalloc(C.byref(b), nbytes) == 0
        ms = []
        for k in range(reps + 2):
            self.L.hipDeviceSynchronize()
            t0 = time.perf_counter()
            assert self.L.hipMemcpy(b, a, nbytes, 3) == 0                     # hipMemcpyDeviceToDevice
            self.L.hipDeviceSynchronize()
            if k >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        self.L.hipFree(a); self.L.hipFree(b)
        return ms


class RawPlans:
    """mnav_fleet_plans through the C ABI into buffers that exist before the clock starts"""

    def __init__(self, ctx, slots, vtx, start, goal, cap):
        n = len(slots)
        self.ctx, self.n, self.slots, self.vtx, self.start, self.goal = ctx, n, slots, vtx, start, goal
        self.codes, self.lens = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.off, self.cost, self.poses = np.zeros(n + 1, np.uint64), np.zeros(n, np.float64), np.zeros((max(int(cap), 1), 7), np.float64)
        self.total = C.c_uint64(0)

    def __call__(self, sizing=False):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_plans(c._h, self.n, vp(self.slots), vp(self.vtx), vp(self.start), self.goal.shape[0], vp(self.goal), vp(self.codes), None, None,
                                   vp(self.lens), vp(self.off), vp(self.cost), None if sizing else vp(self.poses), 0 if sizing else self.poses.shape[0], C.byref(self.total))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == (1 if sizing else 0), (rc, c._err())
        return ms, c.fleet_stats()


class PathsThenHost:
    """the parent's way: mnav_fleet_paths (ids over PCIe), then the host pose loop on one thread"""

    def __init__(self, ctx, A, xyz, vn, slots, vtx, start, goal, ids_cap, poses_cap):
        n = len(slots)
        self.ctx, self.A, self.xyz, self.vn, self.n, self.slots, self.vtx, self.start, self.goal = ctx, A, xyz, vn, n, slots, vtx, start, goal
        self.codes, self.lens, self.off = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
        self.ids, self.total = np.zeros(max(int(ids_cap), 1), np.uint32), C.c_uint64(0)
        self.poses, self.cost = np.zeros((max(int(poses_cap), 1), 7), np.float64), np.zeros(n, np.float64)

    def __call__(self):
        c = self.ctx
        t0 = time.perf_counter()
        rc = c._L.mnav_fleet_paths(c._h, self.n, vp(self.slots), vp(self.vtx), None, vp(self.codes), None, None, vp(self.lens), vp(self.off), vp(self.ids), self.ids.size,
                                   C.byref(self.total))
        t1 = time.perf_counter()
        assert rc == 0, (rc, c._err())
        self.n_poses = self.A.mnav_adapter_host_vertex_path_poses(vp(self.xyz), vp(self.vn), self.n, vp(self.ids), vp(self.off), vp(self.slots), vp(self.start), vp(self.goal),
                                                                  vp(self.poses), vp(self.cost))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def plans_case(ctx, A, hip, mesh, vn, plans, sizes, reps, res):
    rng = np.random.default_rng(plans)
    seeds = rng.integers(0, mesh.V, plans).astype(np.uint32)
    targets = rng.integers(0, mesh.V, plans).astype(np.uint32)
    t0 = time.perf_counter()
    r = ctx.plan_dijkstra_batch(seeds, targets, BIG_OFFSET, path_cap=4096, want_stats=False)
    out = dict(ms_plan_batch=(time.perf_counter() - t0) * 1e3, engine=ctx.last_engine(), codes=sorted(set(int(c) for c in r["codes"])), sizes={})
    del r
    goal = (mesh.xyz[seeds] + np.array([0.023, 0.011, 0.004], np.float32)).astype(np.float32)
    for n in sizes:
        slots = (np.arange(n) % plans).astype(np.uint32)
        vtx = rng.integers(0, mesh.V, n).astype(np.uint32)
        start = (mesh.xyz[vtx] + np.array([0.031, 0.017, 0.02], np.float32)).astype(np.float32)
        sizing = RawPlans(ctx, slots, vtx, start, goal, 0)
        ms_size, _ = sizing(sizing=True)
        total = int(sizing.total.value)
        new = RawPlans(ctx, slots, vtx, start, goal, total)
        old = PathsThenHost(ctx, A, mesh.xyz, vn, slots, vtx, start, goal, total, total)
        k = reps if n <= 20000 else max(8, reps // 2) if total < 50_000_000 else 8
        for _ in range(2):
            new(); old()
        wn, kn, wp, wh = [], [], [], []
        for _ in range(k):                                                   # alternated
            ms, st = new(); wn.append(ms); kn.append(st["ms_kernels"])
            a, b = old(); wp.append(a); wh.append(b)
        same = old.n_poses == total and same_bits(new.poses, old.poses) and same_bits(new.cost, old.cost) and np.array_equal(new.lens, np.where(old.lens > 0, old.lens + 1, 0))
        e = dict(robots=n, poses=total, mean_poses=total / n, nan_poses=int(sum(np.isnan(new.poses[lo: lo + (1 << 22)]).any(axis=1).sum() for lo in range(0, total, 1 << 22))), bytes_down=int(56 * total + 28 * n), ms_sizing_call=ms_size,
                 fleet_plans_ms_kernels=spread(kn), fleet_plans_ms_call_wall=spread(wn), fleet_paths_ms_call_wall=spread(wp), host_pose_loop_ms=spread(wh),
                 paths_then_host_ms=spread([a + b for a, b in zip(wp, wh)]), same_poses_and_costs=bool(same))
        if hip is not None and total:
            ms = hip.copy_ms(56 * total, 8)
            e["d2d_hipMemcpy_of_the_pose_bytes"] = dict(bytes=56 * total, ms=spread(ms), gb_per_s_copied=56 * total / np.median(ms) / 1e6)
        out["sizes"][str(n)] = e
        del new, old, sizing
        print("plans", plans, n, json.dumps(e), flush=True)
    res["plans_%d_plans" % plans] = out


def walks_case(ctx, A, mesh, fn, reps, res, plans=128, per_plan=16, step=0.2, cap=4096):
    rng = np.random.default_rng(7)
    a = rng.uniform(0.1, 0.9, (plans, 2))
    ang = rng.uniform(0, 2 * np.pi, plans)
    b = np.clip(a + 0.12 * np.stack([np.cos(ang), np.sin(ang)], axis=1), 0.02, 0.98)
    off = np.array([0.023, 0.011, 0.0], np.float32)
    goal = np.array([mesh.xyz[mesh.vertex_at(*p)] for p in a], np.float32) + off
    t = np.linspace(1.0, 0.35, per_plan)
    start = np.array([[mesh.xyz[mesh.vertex_at(*(a[p] + t[k] * (b[p] - a[p])))] for k in range(per_plan)] for p in range(plans)], np.float32) + off
    gf = ctx.locate(goal)["face"]
    sf = ctx.locate(start.reshape(-1, 3))["face"].reshape(plans, per_plan)
    r = ctx.plan_cvp_batch(goal, gf, sf[:, 0], 0.3)
    goal_pose = np.concatenate([goal.astype(np.float64), np.tile([0.0, 0.0, 0.0, 1.0], (plans, 1))], axis=1)
    pos = np.ascontiguousarray(start.transpose(1, 0, 2).reshape(-1, 3))
    face = np.ascontiguousarray(sf.T.reshape(-1))
    slots = np.tile(np.arange(plans, dtype=np.uint32), per_plan)
    n = len(slots)
    total = ctx.fleet_walk_plans(slots, goal, gf, goal_pose, pos, face, step_width=step, walk_cap=cap)["total"]
    poses_h, cost_h = np.zeros((max(total, 1), 7), np.float64), np.zeros(n, np.float64)

    def new():
        t0 = time.perf_counter()
        o = ctx.fleet_walk_plans(slots, goal, gf, goal_pose, pos, face, step_width=step, walk_cap=cap, poses_cap=max(total, 1))
        return (time.perf_counter() - t0) * 1e3, o

    def old():
        t0 = time.perf_counter()
        w = ctx.fleet_walks(slots, goal, gf, pos, face, step_width=step, walk_cap=cap, entries_cap=max(total, 1))
        t1 = time.perf_counter()
        A.mnav_adapter_host_face_path_poses(vp(fn), n, vp(w["positions"]), vp(w["faces"]), vp(w["offsets"]), vp(slots), vp(goal_pose), vp(poses_h), vp(cost_h))
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    for _ in range(2):
        _ms, o = new(); old()
    same = same_bits(o["poses"], poses_h[:total]) and same_bits(o["cost"], cost_h)
    wn, kn, ww, wh = [], [], [], []
    for _ in range(reps):
        ms, o = new(); wn.append(ms); kn.append(ctx.fleet_stats()["ms_kernels"])
        x, y = old(); ww.append(x); wh.append(y)
    res["walk_plans"] = dict(plans=plans, robots=n, poses=total, codes=sorted(set(int(c) for c in r["codes"])), reached=int((o["status"] == 1).sum()), step_width=step, walk_cap=cap,
                             fleet_walk_plans_ms_kernels=spread(kn), fleet_walk_plans_ms_call_wall=spread(wn), fleet_walks_ms_call_wall=spread(ww),
                             host_pose_loop_ms=spread(wh), walks_then_host_ms=spread([x + y for x, y in zip(ww, wh)]), same_poses_and_costs=bool(same))
    print("walk plans", json.dumps(res["walk_plans"]), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--small-plans", type=int, default=64)
    ap.add_argument("--big-plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,131072")
    ap.add_argument("--skip", default="", help="comma list of: small, big, walks")
    ap.add_argument("--copy", action="store_true", help="time a device-to-device hipMemcpy of the pose bytes of every size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_plans_perf.json"))
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    sizes = [int(s) for s in args.sizes.split(",")]
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    fn = om.face_normals()
    vn = om.vertex_normals(fn)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), reps=args.reps, warmup=2, offset_of_the_fields=BIG_OFFSET)
    A = adapter_lib()
    with capi.MnavContext(0) as ctx:
        hip = Hip() if args.copy else None
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, vn)
        ctx.upload_face_normals(fn)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        if "walks" not in skip:
            walks_case(ctx, A, mesh, fn, args.reps, res)
        if "small" not in skip:
            plans_case(ctx, A, hip, mesh, vn, args.small_plans, sizes, args.reps, res)
        if "big" not in skip:
            plans_case(ctx, A, hip, mesh, vn, args.big_plans, sizes, args.reps, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
