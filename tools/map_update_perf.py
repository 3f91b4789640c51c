"""One obstacle frame through the resident layer graph (mnav_map_obstacle) against the same event through the separate
entry points (mnav_layer_obstacle, mnav_layer_download, mnav_layer_inflation, mnav_layer_download + a host diff,
mnav_combine_layers_update), on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), with 131 072-point frames as in
tools/gpu_obstacle_perf.py.  Graph: obstacle (slot 0) -> inflation (1); combined (3, the default layer) = max or avg of
(obstacle, inflation, steepness (2)); edge_cost_factor 1.  Both paths see the same frames, each on its own context; wall
time per event, its spread, the bytes each path moves over PCIe, and a check that both leave the same costs and weights.

The graph's default layer is the combination, and nothing reads the combination's lethal set here, so the baseline
needs no host-combined layer uploaded for it (with an inflation over a combination it would).

One process; every step runs under an alarm of its own and a step that overruns it ends the process.

    python tools/map_update_perf.py [--frames K] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import time
from contextlib import contextmanager

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mesh_navigation_amd import capi, meshgen  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_obstacle_perf import cloud  # noqa: E402  (the lidar-like cloud of the obstacle layer's timing)

N_POINTS = 131072
KW = dict(robot_height=2.0, max_obstacle_dist=25.0)


@contextmanager
def step(name: str, seconds: int):
    def overrun(*_):
        print(f"step '{name}' overran its {seconds} s", flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, overrun)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def spread(ms):
    a = np.asarray(ms, np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()), p10=float(np.percentile(a, 10)), p90=float(np.percentile(a, 90)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    with step("mesh", 120):
        from oracle import oracle as O
        mesh = meshgen.terrain(1000, 0.1, 2)
        vn = O.OracleMesh(mesh.xyz, mesh.faces).vertex_normals()
    V = mesh.V
    centre = np.array([50.0, 50.0, 1.0], np.float32)
    res = dict(mesh=dict(V=V, F=mesh.F), points=N_POINTS, frames=args.frames, modes={})
    for mode in ("max", "avg"):
        rng = np.random.default_rng(0)
        nodes = [dict(layer=0, kind="input"), dict(layer=2, kind="input"), dict(layer=1, kind="inflation", inputs=[0]),
                 dict(layer=3, kind=mode, inputs=[0, 1, 2], weights=[1.0, 1.0, 1.0])]
        with capi.MnavContext(0) as g, capi.MnavContext(0) as b:
            p, m = cloud(rng, N_POINTS, centre)
            with step("setup", 120):
                for ctx in (g, b):
                    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, vn)
                    ctx.layer_steepness(2, 0.6)
                    ctx.layer_obstacle(0, p, sensor_to_map=m, **KW)
                g.map_configure(nodes, 3, 1.0)
                g.map_compute()
                b.layer_inflation(1, 0)
                b.combine_layers([0, 1, 2], [1.0, 1.0, 1.0], mode=mode, edge_cost_factor=1.0)
            t_graph, t_base, parts, n_d, n_obst, waves, dev_ms = [], [], [], [], [], [], []
            bytes_graph, bytes_base = [], []
            for k in range(args.warmup + args.frames):
                p, m = cloud(rng, N_POINTS, centre + np.array([0.05 * (k + 1), 0.0, 0.0], np.float32))
                with step("graph frame", 60):
                    t0 = time.perf_counter()
                    out = g.map_obstacle(0, p, sensor_to_map=m, **KW)
                    tg = (time.perf_counter() - t0) * 1e3
                with step("baseline frame", 60):
                    t0 = time.perf_counter()
                    ob = b.layer_obstacle(0, p, sensor_to_map=m, **KW)
                    t1 = time.perf_counter()
                    before = b.layer_download(1)[0]
                    t2 = time.perf_counter()
                    b.layer_inflation(1, 0)
                    t3 = time.perf_counter()
                    after = b.layer_download(1)[0]
                    ids = np.union1d(np.nonzero(before.view(np.uint32) != after.view(np.uint32))[0].astype(np.uint32), ob["changed"])
                    t4 = time.perf_counter()
                    b.combine_layers_update([0, 1, 2], ids, [1.0, 1.0, 1.0], mode=mode)
                    t5 = time.perf_counter()
                if k < args.warmup:
                    continue
                st = out["stats"]
                t_graph.append(tg); t_base.append((t5 - t0) * 1e3)
                parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3])
                n_d.append(int(out["changed"].size)); n_obst.append(int(ob["changed"].size)); waves.append(st["waves"]); dev_ms.append(st["ms_total"])
                # the frame up; down: the obstacle pass's 24 B of counters, 16 B per diffing stage (the wave, the combination)
                # and the wave's own control words are not counted in either path; |D| (id, value) pairs
                bytes_graph.append(p.nbytes + 24 + 16 * 2 + 8 * int(out["changed"].size))
                # the frame up; down: counters, the obstacle's ids, the inflation layer twice (costs + flags); up: the ids;
                # down: their combined values
                bytes_base.append(p.nbytes + 24 + 4 * int(ob["changed"].size) + 2 * 5 * V + 4 * int(ids.size) + 4 * int(ids.size))
            with step("compare", 60):
                vg, wg = g.download_costs()
                vb, wb = b.download_costs()
                same = bool(np.array_equal(vg.view(np.uint32), vb.view(np.uint32)) and np.array_equal(wg.view(np.uint32), wb.view(np.uint32)))
            pa = np.asarray(parts, np.float64)
            res["modes"][mode] = dict(
                graph_ms=spread(t_graph), baseline_ms=spread(t_base), graph_device_ms_median=float(np.median(dev_ms)),
                baseline_parts_ms_median=dict(zip(("obstacle", "download_before", "inflation", "download_and_diff", "combine_update"),
                                                  (float(x) for x in np.median(pa, axis=0)))),
                default_changed_median=int(np.median(n_d)), obstacle_changed_median=int(np.median(n_obst)), waves=sorted(set(waves)),
                pcie_bytes_graph_median=int(np.median(bytes_graph)), pcie_bytes_baseline_median=int(np.median(bytes_base)),
                frame_bytes=int(p.nbytes), same_costs_and_weights=same)
            print(mode, json.dumps(res["modes"][mode]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
