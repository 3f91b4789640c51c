"""Timing of the pose lookup (mnav_locate) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2):
index build (HIP events, first lookup after each upload), the query kernel (HIP events) and the whole call (wall clock:
positions up, kernel, four result arrays down) for n = 2, 14 336 and 1 048 576 surface positions, median of `--reps`
after 3 warm-up calls; for context the same positions through the adapter's host MeshMap (its x/y grid, one thread,
finalize() not timed); and what plan_dijkstra_batch_at adds to plan_dijkstra_batch at 7 168 plans (wall clock, the two
alternating).

    python tools/gpu_locate_perf.py [--reps K] [--out FILE] [--build-only]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402

ADAPTER = os.path.join(ROOT, "mesh_navigation_amd", "csrc", "adapter")
HOST_LIB = os.path.join(ROOT, "tools", "_variants", "liblocate_hostgrid.so")
HOST_SRC = r'''
#include <chrono>
#include "mesh_map_host.h"
// n lookups (nearest vertex + containing face) through the adapter's MeshMap; returns the milliseconds of the queries alone
extern "C" double host_grid_locate(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, uint32_t n, const float* p,
                                   uint32_t* vtx, uint32_t* face)
{
  mesh_map::MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F);
  m.finalize();
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n; ++i) {
    const mesh_map::Vector q(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]);
    vtx[i] = m.getNearestVertexHandle(q);
    face[i] = m.getContainingFace(q, 0.4f);
  }
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
'''


def host_lib():
    src = os.path.join(os.path.dirname(HOST_LIB), "locate_hostgrid.cpp")
    os.makedirs(os.path.dirname(HOST_LIB), exist_ok=True)
    if not os.path.exists(src) or open(src).read() != HOST_SRC:
        with open(src, "w") as f:
            f.write(HOST_SRC)
    deps = [src, os.path.join(ADAPTER, "mesh_map_host.cpp"), os.path.join(ADAPTER, "mesh_map_host.h")]
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", ADAPTER, "-I", os.path.join(ROOT, "include"),
                               "-o", HOST_LIB, src, os.path.join(ADAPTER, "mesh_map_host.cpp")])
    L = C.CDLL(HOST_LIB)
    L.host_grid_locate.restype = C.c_double
    L.host_grid_locate.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def surface_points(mesh, n, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, mesh.F, n)
    w = rng.dirichlet(np.ones(3), n)
    p = (mesh.xyz[mesh.faces[f]].astype(np.float64) * w[:, :, None]).sum(axis=1)
    p[:, 2] += rng.normal(0.0, 0.05, n)
    return p.astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_perf.json"))
    ap.add_argument("--build-only", action="store_true", help="compile the host-grid helper and exit")
    args = ap.parse_args()
    H = host_lib()
    if args.build_only:
        return
    mesh = meshgen.terrain(1000, 0.1, 2)
    xyz, faces = np.ascontiguousarray(mesh.xyz, np.float32), np.ascontiguousarray(mesh.faces, np.uint32)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), reps=args.reps, warmup=3, build_ms=[], queries={})
    with capi.MnavContext(0) as ctx:
        from oracle import oracle as O
        om = O.OracleMesh(mesh.xyz, mesh.faces)
        vn = om.vertex_normals()
        two = surface_points(mesh, 2, 1)
        for _ in range(args.builds):                          # the index is built by the first lookup after an upload
            ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, vn)
            ctx.locate(two)
            st = ctx.locate_stats()
            assert st["built"] == 1
            res["build_ms"].append(st["ms_build"])
        res["index_bytes_per_vertex"] = 24
        for n in (2, 14336, 1048576):
            p = surface_points(mesh, n, 10 + n)
            for _ in range(3):
                ctx.locate(p)
            kern, wall, cand = [], [], 0
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = ctx.locate(p)
                wall.append((time.perf_counter() - t0) * 1e3)
                st = ctx.locate_stats()
                kern.append(st["ms_query"]); cand = st["candidates"]
            hv, hf = np.empty(n, np.uint32), np.empty(n, np.uint32)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            host_ms = H.host_grid_locate(mesh.V, mesh.F, vp(xyz), vp(faces), n, vp(p), vp(hv), vp(hf))
            mk = float(np.median(kern))
            res["queries"][str(n)] = dict(ms_kernel_median=mk, ms_kernel_min=float(np.min(kern)), ms_call_wall_median=float(np.median(wall)),
                                          ms_call_wall_min=float(np.min(wall)), queries_per_s_kernel=n / (mk * 1e-3) if mk > 0 else None,
                                          candidates_per_query=cand / n, faces_found=float((got["face"] != 0xFFFFFFFF).mean()),
                                          ms_host_grid_single_thread=host_ms, host_grid_same_vertex=float((hv == got["vertex"]).mean()),
                                          host_grid_same_face=float((hf == got["face"]).mean()))
            print(n, json.dumps(res["queries"][str(n)]), flush=True)
        # plans from positions against plans from ids, alternating, paths only
        n = args.plans
        steep, _ = om.steepness(vn, 0.3)
        costs = np.minimum(steep, np.float32(0.9)).astype(np.float32)
        ctx.upload_costs(costs, om.edge_weights(om.edge_distances(), costs, 1.0))
        goal, start = surface_points(mesh, n, 5), surface_points(mesh, n, 6)
        ids = ctx.locate(np.concatenate([goal, start]))["vertex"]
        seeds, targets = ids[:n].copy(), ids[n:].copy()
        t_ids, t_at = [], []
        for k in range(3 + max(5, args.reps // 2)):
            t0 = time.perf_counter()
            a = ctx.plan_dijkstra_batch(seeds, targets, path_cap=4096, want_stats=False)
            t1 = time.perf_counter()
            b = ctx.plan_dijkstra_batch_at(goal, start, path_cap=4096, want_stats=False)
            t2 = time.perf_counter()
            assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["path_len"], b["path_len"])
            if k >= 3:
                t_ids.append((t1 - t0) * 1e3); t_at.append((t2 - t1) * 1e3)
            codes = sorted(set(int(c) for c in b["codes"]))
            del a, b
        hv, hf = np.empty(2 * n, np.uint32), np.empty(2 * n, np.uint32)
        both = np.ascontiguousarray(np.concatenate([goal, start]))
        host_ms = H.host_grid_locate(mesh.V, mesh.F, xyz.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p), 2 * n,
                                     both.ctypes.data_as(C.c_void_p), hv.ctypes.data_as(C.c_void_p), hf.ctypes.data_as(C.c_void_p))
        res["plans_at"] = dict(plans=n, ms_batch_ids_median=float(np.median(t_ids)), ms_batch_at_median=float(np.median(t_at)),
                               ms_added_median=float(np.median(np.array(t_at) - np.array(t_ids))), ms_lookup_kernel=ctx.locate_stats()["ms_query"],
                               ms_host_grid_single_thread=host_ms, codes=codes)
        print("plans_at", json.dumps(res["plans_at"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
