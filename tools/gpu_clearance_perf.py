"""Timing of the clearance and border layers (mnav_layer_clearance, mnav_layer_border) on terrain(1000, 0.1, 2), the 1M-vertex
C2 mesh, under a flat ceiling sheet (z = 1.0, spacing 0.2) over half of its area: medians of the BVH build (HIP events,
built by the first clearance call after each upload), of that first call (cast kernel alone, and the whole call: events
from the call's start to the end of the cost pass), of a reconfigure-only call (cached clearance, cost pass + change
list) and of a border call (wall time of the C call, which includes its counter download and synchronisation).

    python tools/gpu_clearance_perf.py [--builds K] [--calls K] [--out FILE (default profiles/clearance_perf.json)]"""
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
from tests import clearance_model as CM  # noqa: E402


def mesh_with_ceiling():
    ground = meshgen.terrain(1000, 0.1, 2)
    g = meshgen.flat_grid(250, 0.2)
    top = g.xyz.copy()
    top[:, 0] *= 0.5                                                  # x in 0 .. 24.9 of 0 .. 99.9: half the area
    top[:, 2] = 1.0
    xyz = np.concatenate([ground.xyz, top]).astype(np.float32)
    faces = np.concatenate([ground.faces, g.faces[:, ::-1] + ground.V]).astype(np.uint32)
    return meshgen.from_faces(xyz, faces)


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_perf.json"))
    args = ap.parse_args()
    mesh = mesh_with_ceiling()
    nrm = CM.vertex_normals(mesh.xyz, mesh.faces)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F, ceiling="flat sheet z=1.0 over x<25 (half the area)"), builds=args.builds, calls=args.calls)
    first = dict(bvh=[], cast=[], total=[], wall=[])
    with capi.MnavContext(0) as ctx:
        for _ in range(args.builds):                                 # the first clearance call after an upload builds + casts
            ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
            t0 = time.perf_counter()
            st = ctx.layer_clearance(0, 0.5, 0.3)["stats"]
            first["wall"].append((time.perf_counter() - t0) * 1e3)
            assert st["cast"] == 1
            first["bvh"].append(st["ms_bvh_build"]); first["cast"].append(st["ms_cast"]); first["total"].append(st["ms_total"])
        res["first_call"] = dict(ms_bvh_build_median=med(first["bvh"]), ms_cast_median=med(first["cast"]),
                                 ms_cast_plus_costs_median=med([t - b for t, b in zip(first["total"], first["bvh"])]),
                                 ms_call_device_median=med(first["total"]), ms_call_wall_median=med(first["wall"]),
                                 rays=st["rays"], hits=st["hits"], samples=first)
        print("first", json.dumps({k: v for k, v in res["first_call"].items() if k != "samples"}), flush=True)
        dev, wall, nch = [], [], []
        for k in range(args.calls + 3):                              # reconfigure: alternate two height pairs, cache reused
            rh, hi = (0.5, 0.3) if k % 2 else (0.6, 0.25)
            t0 = time.perf_counter()
            r = ctx.layer_clearance(0, rh, hi)
            w = (time.perf_counter() - t0) * 1e3
            assert r["stats"]["cast"] == 0
            if k >= 3:
                dev.append(r["stats"]["ms_total"]); wall.append(w); nch.append(r["changed"].size)
        res["reconfigure"] = dict(ms_call_device_median=med(dev), ms_call_wall_median=med(wall), changed_median=int(np.median(nch)))
        print("reconfigure", json.dumps(res["reconfigure"]), flush=True)
        wall, nch = [], []
        for k in range(args.calls + 3):
            bc = 1.0 if k % 2 else 0.75                              # every border vertex changes cost bits each call
            r = ctx.layer_border(1, bc, 0.5)
            if k >= 3:
                wall.append(r["stats"]["ms_wall"]); nch.append(r["changed"].size)
        res["border"] = dict(ms_call_wall_median=med(wall), changed_median=int(np.median(nch)), n_lethal=r["n_lethal"])
        print("border", json.dumps(res["border"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
