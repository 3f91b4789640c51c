"""Timing of the vector-field follower (mnav_follow_batch) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the
resident vector maps of a 7 168-plan Dijkstra batch (about 86 GB of fields that never leave HBM):

  * device: kernel time (HIP events around the passes) and whole call (wall clock: 44 B per robot up, the passes, every
    output down) for 1, 14 336 and 1 048 576 robots, median of `--reps` calls after 3 warm-up calls, in two mixes -- every
    robot still on its face, and 90 % stay / 9 % neighbour search / 1 % global search -- with robot i on plan i mod 7 168;
  * the same with all robots on plan 0, beside the same ticks through the adapter's host MeshMap on one thread (the
    reference's controller follows one field; median of the same number of runs after one warm-up run, 5 runs for the
    million robots): that field is downloaded once, the download timed separately;
  * mnav_vector_at called once per robot for the 14 336 robots: the sampling path the batch call replaces.

    python tools/follow_perf.py [--reps K] [--plans N] [--out FILE] [--build-only]"""
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
HOST_LIB = os.path.join(ROOT, "tools", "_variants", "libfollow_host.so")
HOST_SRC = r'''
#include <chrono>
#include <cmath>
#include "mesh_map_host.h"
using namespace mesh_map;
// n ticks of mesh_controller.cpp:67-170 / :225-242 through the adapter's MeshMap over ONE vector map; returns the
// milliseconds of the ticks alone (finalize() and setVectorMap are not timed).  cfg: mesh_controller.h:193-200
extern "C" double host_follow(uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const float* costs, const float* vecmap, uint32_t n,
                              const float* pos, const float* dir, const float* up, const uint32_t* face_in, const double* cfg, int32_t* code,
                              uint32_t* face_out, double* cmd)
{
  MeshMap m;
  m.positions.assign(xyz, xyz + 3 * (size_t)V); m.faces.assign(faces, faces + 3 * (size_t)F); m.vertex_costs.assign(costs, costs + V);
  m.finalize();
  std::vector<uint8_t> set(V);
  for (uint32_t v = 0; v < V; ++v) set[v] = vecmap[3 * (size_t)v] != 0.f || vecmap[3 * (size_t)v + 1] != 0.f || vecmap[3 * (size_t)v + 2] != 0.f;
  m.setVectorMap(std::vector<float>(vecmap, vecmap + 3 * (size_t)V), set);
  const double max_lin = cfg[0], max_ang = cfg[1], ang_f = cfg[3], lin_f = cfg[4], max_angle_deg = cfg[5], radius = cfg[6], max_dist = cfg[7];
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n; ++i) {
    Vector p(pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
    const Vector d(dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2]), u(up[3 * (size_t)i], up[3 * (size_t)i + 1], up[3 * (size_t)i + 2]);
    uint32_t f = face_in[i];
    std::array<float, 3> b; float dist;
    code[i] = 1; face_out[i] = kNoHandle; cmd[2 * (size_t)i] = cmd[2 * (size_t)i + 1] = 0.0;
    bool project = true;
    if (f != kNoHandle && projectedBarycentricCoords(p, m.facePositions(f), b, dist) && dist < max_dist) project = false;
    else if (f != kNoHandle && m.findNeighbourFace(p, f, (float)radius, (float)max_dist, f, b)) {}
    else {
      f = m.getContainingFace(p, (float)max_dist);
      if (f == kNoHandle) continue;
      projectedBarycentricCoords(p, m.facePositions(f), b, dist);
    }
    if (project) { const auto t = m.facePositions(f); p = t[0] * b[0] + t[1] * b[1] + t[2] * b[2]; }
    face_out[i] = f;
    const uint32_t* vs = &m.faces[3 * (size_t)f];                     // directionAtPosition, mesh_map.cpp:625-650
    if (!(set[vs[0]] || set[vs[1]] || set[vs[2]])) { code[i] = 2; continue; }
    Vector v(0, 0, 0);
    for (int k = 0; k < 3; ++k)
      if (set[vs[k]]) v = v + Vector(vecmap[3 * (size_t)vs[k]], vecmap[3 * (size_t)vs[k] + 1], vecmap[3 * (size_t)vs[k] + 2]) * b[k];
    if (!(std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z))) { code[i] = 2; continue; }
    const Vector mesh_dir = v.normalized();
    const float phi = std::acos(mesh_dir.dot(d)), sign_phi = mesh_dir.cross(d).dot(u);
    const float ang = copysignf((float)(phi * max_ang / M_PI), -sign_phi);
    const float max_angle = (float)(max_angle_deg * M_PI / 180.0), max_linear = (float)max_lin;
    const float lin = phi <= max_angle ? max_linear - (phi * max_linear / max_angle) : 0.f;
    cmd[2 * (size_t)i] = std::min(max_lin, lin * lin_f); cmd[2 * (size_t)i + 1] = std::min(max_ang, ang * ang_f);
    code[i] = 0;
  }
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
'''


def host_lib():
    src = os.path.join(os.path.dirname(HOST_LIB), "follow_host.cpp")
    os.makedirs(os.path.dirname(HOST_LIB), exist_ok=True)
    if not os.path.exists(src) or open(src).read() != HOST_SRC:
        with open(src, "w") as f:
            f.write(HOST_SRC)
    deps = [src, os.path.join(ADAPTER, "mesh_map_host.cpp"), os.path.join(ADAPTER, "mesh_map_host.h")]
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", ADAPTER, "-I", os.path.join(ROOT, "include"),
                               "-o", HOST_LIB, src, os.path.join(ADAPTER, "mesh_map_host.cpp")])
    L = C.CDLL(HOST_LIB)
    L.host_follow.restype = C.c_double
    L.host_follow.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 8
    return L


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def make_robots(mesh, targets, n, n_slots, mix, seed, field_vertices=None):
    """robot i follows plan i % n_slots and stands on a face at that plan's robot vertex (inside the field) -- or, with
    `field_vertices`, at a random one of those vertices; mix "stay": on the face it was on; "mixed": 9 % on another face at
    that vertex (neighbour search), 1 % were on a face far away (global search)"""
    rng = np.random.default_rng(seed)
    first = np.zeros(mesh.V, np.int64)
    last = np.zeros(mesh.V, np.int64)
    ids = np.arange(mesh.F)
    for k in range(3):
        last[mesh.faces[:, k]] = ids
        first[mesh.faces[::-1, k]] = ids[::-1]
    slot = (np.arange(n) % n_slots).astype(np.uint32)
    v = targets[slot] if field_vertices is None else field_vertices[rng.integers(0, field_vertices.shape[0], n)]
    f = first[v]
    w = rng.dirichlet(np.ones(3), n) * 0.7 + 0.1
    pos = (mesh.xyz[mesh.faces[f]].astype(np.float64) * w[:, :, None]).sum(axis=1).astype(np.float32)
    face_in = f.copy()
    if mix == "mixed":
        r = rng.uniform(size=n)
        nb = (r < 0.09) & (last[v] != f)
        face_in[nb] = last[v][nb]
        gl = (r >= 0.09) & (r < 0.10)
        face_in[gl] = (f[gl] + mesh.F // 2) % mesh.F
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1).astype(np.float32)
    up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    return dict(pos=pos, dir=d, up=up, face_in=face_in.astype(np.uint32), slot=slot)


def time_device(ctx, r, reps):
    for _ in range(3):
        ctx.follow(r["pos"], r["dir"], r["up"], r["face_in"], r["slot"])
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ctx.follow(r["pos"], r["dir"], r["up"], r["face_in"], r["slot"])
        wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.follow_stats()
        kern.append(st["ms_kernels"])
    n = r["pos"].shape[0]
    res = dict(ms_kernels_median=float(np.median(kern)), ms_kernels_min=float(np.min(kern)), ms_call_wall_median=float(np.median(wall)),
               ms_call_wall_min=float(np.min(wall)), robots_per_s_wall=n / (float(np.median(wall)) * 1e-3),
               stayed=st["stayed"], neighbour=st["neighbour"], global_search=st["global"], lost=st["lost"], no_field=st["no_field"],
               bytes_up_per_robot=sum(r[k].nbytes for k in ("pos", "dir", "up", "face_in", "slot")) // n,
               bytes_down_per_robot=sum(getattr(out, k).nbytes for k in ("code", "face", "bary", "pos", "mesh_dir", "cost", "cmd", "how")) // n)
    return res, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--sizes", default="1,14336,1048576")
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_perf.json"))
    ap.add_argument("--build-only", action="store_true", help="compile the host helper and exit")
    args = ap.parse_args()
    H = host_lib()
    if args.build_only:
        return
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    xyz, faces = np.ascontiguousarray(mesh.xyz, np.float32), np.ascontiguousarray(mesh.faces, np.uint32)
    costs = np.zeros(mesh.V, np.float32)
    weights = meshgen.edge_lengths(mesh)
    sizes = [int(s) for s in args.sizes.split(",")]
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=args.plans, reps=args.reps, warmup=3, device_spread={}, device_one_plan={}, host_one_plan={})
    cfg = capi.FollowConfig()
    cfg8 = np.array([getattr(cfg, k) for k, _ in capi.FollowConfig._fields_], np.float64)
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.upload_costs(costs, weights)
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(5)
        seeds = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        targets = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        t0 = time.perf_counter()
        r = ctx.plan_dijkstra_batch(seeds, targets, path_cap=4096, want_stats=False)
        res["ms_plan_batch"] = (time.perf_counter() - t0) * 1e3
        res["plan_codes"] = sorted(set(int(c) for c in r["codes"]))
        res["resident_field_bytes"] = 12 * mesh.V * args.plans
        res["engine"] = ctx.last_engine()
        del r
        ctx.follow(*[make_robots(mesh, targets, 64, args.plans, "mixed", 1)[k] for k in ("pos", "dir", "up", "face_in", "slot")])   # builds the index
        res["index_built_by_first_mixed_call"] = ctx.follow_stats()["built_index"]
        t0 = time.perf_counter()
        field0 = ctx.download_output("vecmap", 0)
        res["ms_download_one_field"] = (time.perf_counter() - t0) * 1e3
        field_vertices = np.nonzero(field0.any(axis=1))[0]                # plan 0's field: where its one-plan robots stand
        res["field_vertices_plan0"] = int(field_vertices.shape[0])
        for n in sizes:
            for mix in ("stay", "mixed"):
                key = "%d_%s" % (n, mix)
                res["device_spread"][key], _ = time_device(ctx, make_robots(mesh, targets, n, args.plans, mix, 10 + n), args.reps)
                one = make_robots(mesh, targets, n, 1, mix, 20 + n, field_vertices)
                res["device_one_plan"][key], out = time_device(ctx, one, args.reps)
                code, face, cmd = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros((n, 2), np.float64)
                host_reps = args.reps if n <= 100000 else 5              # (a million mixed ticks take most of a second each)
                ms = [H.host_follow(mesh.V, mesh.F, vp(xyz), vp(faces), vp(costs), vp(field0), n, vp(one["pos"]), vp(one["dir"]), vp(one["up"]),
                                    vp(one["face_in"]), vp(cfg8), vp(code), vp(face), vp(cmd)) for _ in range(1 + host_reps)][1:]   # first run: warm-up
                dev = res["device_one_plan"][key]
                res["host_one_plan"][key] = dict(ms_ticks_single_thread_median=float(np.median(ms)), ms_ticks_single_thread_min=float(np.min(ms)), runs=host_reps,
                                                 speedup_wall_same_robots=float(np.median(ms)) / dev["ms_call_wall_median"], same_code=float((code == out.code).mean()), same_face=float((face == out.face).mean()),
                                                 same_cmd_bits=float((cmd.view(np.uint64) == out.cmd.view(np.uint64)).all(axis=1).mean()))
                print(key, json.dumps(dict(spread=res["device_spread"][key], one_plan=res["device_one_plan"][key], host=res["host_one_plan"][key])), flush=True)
        # the path this replaces: one mnav_vector_at per robot (face and barycentrics from the batch call's outputs)
        n = 14336 if 14336 in sizes else sizes[-1]
        rb = make_robots(mesh, targets, n, args.plans, "stay", 10 + n)
        out = ctx.follow(rb["pos"], rb["dir"], rb["up"], rb["face_in"], rb["slot"])
        t0 = time.perf_counter()
        hits = 0
        for i in range(n):
            hits += ctx.vector_at(faces[out.face[i]], out.bary[i], int(rb["slot"][i])) is not None
        res["vector_at_per_robot"] = dict(robots=n, ms_total=(time.perf_counter() - t0) * 1e3, with_vector=hits, ok_in_batch=int((out.code == 0).sum()))
        print("vector_at", json.dumps(res["vector_at_per_robot"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
