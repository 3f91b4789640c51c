"""Timing of the obstacle layer (mnav_layer_obstacle) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2):
BVH build (HIP events, first call after each upload), ray cast per frame (HIP events around the cast kernel, after
warm-up; median), the whole call (events: cloud upload .. change list), wall time per call and rays/s for clouds of
32k / 131k / 1M points; then the chain obstacle -> inflation -> combine_layers_update -> one plan (wall time).

    python tools/gpu_obstacle_perf.py [--frames K] [--out FILE]"""
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


def cloud(rng, n, centre):
    """a lidar-like cloud around the sensor: points within 25 m, a third of them above the ground"""
    p = np.empty((n, 3), np.float32)
    r = np.sqrt(rng.uniform(0, 1, n)) * 24.0
    a = rng.uniform(0, 2 * np.pi, n)
    p[:, 0] = r * np.cos(a)
    p[:, 1] = r * np.sin(a)
    p[:, 2] = rng.uniform(-3.0, 1.5, n)
    return p, np.concatenate([np.eye(3, dtype=np.float32), centre.reshape(3, 1)], 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--builds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mesh = meshgen.terrain(1000, 0.1, 2)
    rng = np.random.default_rng(0)
    centre = np.array([50.0, 50.0, 1.0], np.float32)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), frames=args.frames, build_ms=[], clouds={})
    with capi.MnavContext(0) as ctx:
        from oracle import oracle as O
        om = O.OracleMesh(mesh.xyz, mesh.faces)
        vn = om.vertex_normals()
        p, m = cloud(rng, 32768, centre)
        for _ in range(args.builds):                         # the BVH is built by the first obstacle call after an upload
            ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, vn)
            st = ctx.layer_obstacle(0, p, sensor_to_map=m, robot_height=2.0, max_obstacle_dist=25.0)["stats"]
            res["build_ms"].append(st["ms_bvh_build"])
        for n in (32768, 131072, 1048576):
            p, m = cloud(rng, n, centre)
            for _ in range(3):
                ctx.layer_obstacle(1, p, sensor_to_map=m, robot_height=2.0, max_obstacle_dist=25.0)
            cast, total, wall = [], [], []
            for _ in range(args.frames):
                t0 = time.perf_counter()
                r = ctx.layer_obstacle(1, p, sensor_to_map=m, robot_height=2.0, max_obstacle_dist=25.0)
                wall.append((time.perf_counter() - t0) * 1e3)
                cast.append(r["stats"]["ms_cast"]); total.append(r["stats"]["ms_total"])
            mc = float(np.median(cast))
            res["clouds"][str(n)] = dict(ms_cast_median=mc, ms_cast_min=float(np.min(cast)), ms_call_device_median=float(np.median(total)),
                                         ms_call_wall_median=float(np.median(wall)), rays_per_s=n / (mc * 1e-3),
                                         rays_kept=r["stats"]["rays_kept"], hits=r["stats"]["hits"], n_lethal=r["n_lethal"])
            print(n, json.dumps(res["clouds"][str(n)]), flush=True)
        # the update chain of one frame: obstacle -> inflation -> combine_layers_update -> one plan.  The vertices handed to
        # the incremental combination are those whose inflation cost differs from the last frame's (what the reference's
        # InflationLayer reports); finding them here costs a download of both layers, which is NOT in the timed chain.
        ctx.layer_steepness(2, 0.6)
        p, m = cloud(rng, 131072, centre)
        ctx.layer_obstacle(0, p, sensor_to_map=m, robot_height=2.0, max_obstacle_dist=25.0)
        ctx.layer_inflation(3, 0)
        ctx.combine_layers([3, 2], [1.0, 1.0], mode="max", edge_cost_factor=1.0)
        prev = ctx.layer_download(3)[0]
        seed, target = mesh.vertex_at(0.1, 0.1), mesh.vertex_at(0.9, 0.9)
        chain, parts = [], []
        for k in range(max(4, args.frames // 3)):
            p, m = cloud(rng, 131072, centre + np.array([0.05 * k, 0.0, 0.0], np.float32))
            t0 = time.perf_counter()
            ctx.layer_obstacle(0, p, sensor_to_map=m, robot_height=2.0, max_obstacle_dist=25.0)
            t1 = time.perf_counter()
            ctx.layer_inflation(3, 0)
            t2 = time.perf_counter()
            cur = ctx.layer_download(3)[0]
            ids = np.nonzero(cur.view(np.uint32) != prev.view(np.uint32))[0].astype(np.uint32)
            prev = cur
            t3 = time.perf_counter()
            ctx.combine_layers_update([3, 2], ids, [1.0, 1.0], mode="max")
            t4 = time.perf_counter()
            out = ctx.plan_dijkstra(seed, target)
            t5 = time.perf_counter()
            if k >= 2:
                chain.append(((t1 - t0) + (t2 - t1) + (t4 - t3) + (t5 - t4)) * 1e3)
                parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3, int(ids.size), int(out.code)])
        pa = np.array(parts, np.float64)
        res["chain_131k"] = dict(ms_median=float(np.median(chain)), ms_obstacle=float(np.median(pa[:, 0])), ms_inflation=float(np.median(pa[:, 1])),
                                 ms_combine_update=float(np.median(pa[:, 2])), ms_plan=float(np.median(pa[:, 3])),
                                 changed_inflation_median=int(np.median(pa[:, 4])), plan_codes=sorted(set(int(c) for c in pa[:, 5])))
        print("chain", json.dumps(res["chain_131k"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
