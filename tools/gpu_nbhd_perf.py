"""Timing of the local-neighbourhood layers (mnav_layer_height_diff / _roughness / _ridge) on the 1M-vertex C2 mesh,
terrain(1000, 0.1, 2): device milliseconds of each layer at radius 0.3 and 1.0 (HIP events around the whole call, after a
warm-up call; median), wall time per call, Σ|N(v)|, max |N(v)| and the centres that left the LDS path.  Then the same
header's single-threaded host routine (mnav_nbhd.h nb_centre_host, built here with g++ -O2) over a fixed sample of
centres, scaled to all V centres and labelled as such.

    python tools/gpu_nbhd_perf.py [--reps K] [--host-sample N] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402

OPS = ("height_diff", "roughness", "ridge")

SHIM = r'''
#include "mnav_nbhd.h"
extern "C" void layer(int op, const unsigned* row_ptr, const unsigned* nbr, const float* xyz, const float* nrm, double r2,
                      unsigned n, const unsigned* centres, float* out, unsigned* stamp, unsigned* queue) {
  for (unsigned i = 0; i < n; ++i) out[i] = mnav_nb::nb_centre_host(op, centres[i], row_ptr, nbr, xyz, nrm, r2, stamp, i + 1, queue, nullptr);
}
'''


def host_routine(tmp):
    gxx = shutil.which("g++")
    if not gxx:
        return None
    src = os.path.join(tmp, "shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    lib = os.path.join(tmp, "libshim.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "mesh_navigation_amd", "csrc"), "-o", lib, src])
    L = C.CDLL(lib)
    vp = C.c_void_p
    L.layer.argtypes = [C.c_int, vp, vp, vp, vp, C.c_double, C.c_uint, vp, vp, vp, vp]
    return L


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mesh = meshgen.terrain(1000, 0.1, 2)
    from oracle import oracle as O
    nrm = O.OracleMesh(mesh.xyz, mesh.faces).vertex_normals()
    res = dict(mesh=dict(V=mesh.V, E=mesh.E), reps=args.reps, device={}, host={})
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
        for radius in (0.3, 1.0):
            for op in OPS:
                f = getattr(ctx, "layer_" + op)
                f(0, radius=radius)                                  # warm-up (code objects, scratch allocation)
                ms, wall = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    st = f(0, radius=radius)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(st["ms"])
                key = f"{op}_r{radius}"
                res["device"][key] = dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_wall_median=float(np.median(wall)),
                                          visits=st["visits"], mean_size=st["visits"] / mesh.V, max_size=st["max_size"], spilled=st["spilled"])
                print(key, json.dumps(res["device"][key]), flush=True)
    from tests import nbhd_model as M
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    rp, nb = row_ptr.astype(np.uint32), nbr.astype(np.uint32)
    xyz = np.ascontiguousarray(mesh.xyz, np.float32)
    n3 = np.ascontiguousarray(nrm, np.float32)
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        L = host_routine(tmp)
        if L is None:
            res["host"] = "not measured (no g++)"
        else:
            for radius, n in ((0.3, args.host_sample), (1.0, max(1, args.host_sample // 10))):
                c = np.sort(rng.choice(mesh.V, n, replace=False)).astype(np.uint32)
                out = np.zeros(n, np.float32)
                stamp = np.zeros(mesh.V, np.uint32)
                queue = np.zeros(mesh.V, np.uint32)
                for k, op in enumerate(OPS):
                    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
                    t0 = time.perf_counter()
                    L.layer(k, p(rp), p(nb), p(xyz), p(n3), radius * radius, n, p(c), p(out), p(stamp), p(queue))
                    s = time.perf_counter() - t0
                    stamp[:] = 0
                    key = f"{op}_r{radius}"
                    res["host"][key] = dict(sample_centres=n, sample_ms=s * 1e3, scaled_ms_all_centres=s * 1e3 * mesh.V / n,
                                            label="one host thread, sampled centres, scaled linearly to V")
                    print("host", key, json.dumps(res["host"][key]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
