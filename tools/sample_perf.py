"""Timing of the sampled rollout (mnav_follow_sample) on the 1M-vertex C2 mesh, terrain(1000, 0.1, 2), over the resident
fields of the 7 168-plan Dijkstra batch the other fleet tools use (set up as tools/rollout_perf.py does; robot i on plan
i mod 7 168, follow_perf's "mixed" mix): `--ticks` ticks of K in {16, 64, 256} candidates for n in {1, 14 336, the largest n
with n * K <= 2^20} robots, against two comparisons:

  (a) mnav_follow_rollout over n * K robots (every robot K times) for the same ticks: what the same row count cost before,
      with no candidates, no score and no pick -- and with n * K rows uploaded where the sampled call uploads n.  The
      rollout's kernels are this library's k_rollout_*, whose source is the parent commit's but for rol_after_tick being
      written in two pieces;
  (b) for n = 1: the compiled host mirror (smp_run + smp_score + smp_pick of mnav_sample.h, g++ -O2, one thread) over one
      field and potential downloaded from the device, the download timed apart.

The sampled call and (a) alternate; medians with (min .. max) of `--reps` repetitions after `--warmup`.  Per shape: the
whole call (host clock around the synchronised call, picks downloaded only), its kernels (device events), the share of the
expand and of the score + pick kernels, row-ticks per second.

    python tools/sample_perf.py [--reps R] [--ticks T] [--plans N] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from follow_perf import make_robots  # noqa: E402
from mesh_navigation_amd import capi, meshgen  # noqa: E402


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def candidates(K, seed=1):
    """the follower, then arcs and biased followers: gains 0 / 0.5 / 1, biases within the follower's limits"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.choice([0.0, 0.5, 1.0], K), rng.uniform(0.0, 0.5, K), rng.choice([0.0, 1.0], K), rng.uniform(-0.3, 0.3, K)], axis=1)
    t[0] = [1, 0, 1, 0]
    return np.ascontiguousarray(t, np.float64)


def sample_once(ctx, r, tab, cfg, ro, sa):
    t0 = time.perf_counter()
    out = ctx.follow_sample(r["pos"], r["dir"], r["up"], r["face_in"], r["slot"], tab, config=cfg, rollout=ro, sample=sa, outputs=capi.SAMPLE_PICKS)
    return (time.perf_counter() - t0) * 1e3, ctx.sample_stats(), out


def rollout_once(ctx, r, cfg, ro):
    t0 = time.perf_counter()
    ctx.rollout(r["pos"], r["dir"], r["up"], r["face_in"], r["slot"], config=cfg, rollout=ro, outputs=("status",))
    return (time.perf_counter() - t0) * 1e3, ctx.rollout_stats()


def host_mirror(ctx, mesh, r, tab, ro, sa, reps):
    """comparison (b): one robot on the host.  The shim (mnav_sample.h for the host, g++ -O2) and its wrapper are the CPU
    test's own; anything missing raises"""
    import pathlib
    import tempfile

    from oracle import oracle as O
    from tests import follow_model as FM
    from tests.test_sample_model import Mirror, build_shim

    class Tmp:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))

    L = build_shim(Tmp())
    s = int(r["slot"][0])
    t0 = time.perf_counter()
    field, pot = ctx.download_output("vecmap", s), ctx.download_output("dist", s)
    ms_download = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    model = FM.Model(mesh, O.OracleMesh(mesh.xyz, mesh.faces), np.zeros(mesh.V, np.float32))
    mirror = Mirror(L, model)
    ms_setup = (time.perf_counter() - t0) * 1e3
    one = dict(r, slot=np.zeros(1, np.uint32), seed_face=None)
    smp = dict(w_potential=sa.w_potential, w_cost=sa.w_cost, w_time=sa.w_time, lethal_cost=sa.lethal_cost)
    cfg = FM.config()
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = mirror.sample(cfg, [field], [pot], one, None, tab, ro.dt, ro.ticks, sample=smp)
        ms.append((time.perf_counter() - t0) * 1e3)
    mirror.close()
    return dict(ms_call=stats(ms[1:]), ms_field_download=ms_download, ms_mesh_tables_and_index_once=ms_setup, best_k=int(out["best_k"][0]),
                row_ticks=int(out["ticks"].sum()))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--plans", type=int, default=7168)
    ap.add_argument("--candidates", default="16,64,256")
    ap.add_argument("--mesh", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_perf.json"))
    args = ap.parse_args()
    mesh = meshgen.terrain(args.mesh, 0.1, 2)
    res = dict(mesh=dict(V=mesh.V, F=mesh.F), plans=args.plans, reps=args.reps, warmup=args.warmup, ticks=args.ticks, dt=args.dt, shapes={})
    cfg = capi.FollowConfig()
    ro = capi.RolloutConfig(dt=args.dt, ticks=args.ticks)
    sa = capi.SampleConfig(w_potential=1.0, w_cost=0.5, w_time=0.1, lethal_cost=1.0)
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
        ctx.upload_costs(np.zeros(mesh.V, np.float32), meshgen.edge_lengths(mesh))
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(5)
        seeds = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        targets = rng.integers(0, mesh.V, args.plans).astype(np.uint32)
        t0 = time.perf_counter()
        r = ctx.plan_dijkstra_batch(seeds, targets, path_cap=4096, want_stats=False)
        res["plan_batch_s"] = time.perf_counter() - t0
        res["plan_codes"] = sorted(set(int(c) for c in r["codes"]))
        res["engine"] = ctx.last_engine()
        del r
        ctx.locate(mesh.xyz[:8])                                          # the lookup index exists before anything is timed
        for K in [int(k) for k in args.candidates.split(",")]:
            tab = candidates(K)
            for n in (1, 14336, (1 << 20) // K):
                rb = make_robots(mesh, targets, n, args.plans, "mixed", 10 + n)
                rep_rows = {k: np.repeat(v, K, axis=0) for k, v in rb.items()}       # comparison (a): every robot K times
                wall, kern, expand, pick, r_wall, r_kern = [], [], [], [], [], []
                for rep in range(args.warmup + args.reps):
                    w, st, out = sample_once(ctx, rb, tab, cfg, ro, sa)
                    rw, rst = rollout_once(ctx, rep_rows, cfg, ro)
                    if rep >= args.warmup:
                        wall.append(w); kern.append(st["ms_kernels"]); expand.append(st["ms_expand"]); pick.append(st["ms_pick"])
                        r_wall.append(rw); r_kern.append(rst["ms_kernels"])
                a, b = stats(wall), stats(r_wall)
                shape = dict(rows=n * K, fields_used=int(np.unique(rb["slot"]).size), sample_ms_call_wall=a, sample_ms_kernels=stats(kern), sample_ms_expand=stats(expand),
                             sample_ms_score_pick=stats(pick), expand_share_of_kernels=float(np.median(expand) / np.median(kern)),
                             score_pick_share_of_kernels=float(np.median(pick) / np.median(kern)), row_ticks=st["row_ticks"],
                             row_ticks_per_s_kernels=st["row_ticks"] / (np.median(kern) * 1e-3), row_ticks_per_s_wall=st["row_ticks"] / (a["median"] * 1e-3),
                             rollout_ms_call_wall=b, rollout_ms_kernels=stats(r_kern), rollout_robot_ticks=rst["robot_ticks"],
                             rollout_robot_ticks_per_s_kernels=rst["robot_ticks"] / (np.median(r_kern) * 1e-3),
                             rollout_robot_ticks_per_s_wall=rst["robot_ticks"] / (b["median"] * 1e-3),
                             wall_ratio_rollout_over_sample=b["median"] / a["median"], kernels_ratio_rollout_over_sample=float(np.median(r_kern) / np.median(kern)),
                             final_status=dict(running=st["running"], reached=st["reached"], out_of_map=st["out_of_map"], no_field=st["no_field"]),
                             feasible_rows=st["feasible_rows"], lethal_rows=st["lethal_rows"], robots_without_pick=st["robots_without_pick"],
                             stayed=st["stayed"], neighbour=st["neighbour"], global_search=st["global"])
                if n == 1:
                    shape["host_mirror_one_thread"] = host_mirror(ctx, mesh, rb, tab, ro, sa, args.reps)
                res["shapes"]["n%d_K%d" % (n, K)] = shape
                print("n%d_K%d" % (n, K), json.dumps(shape), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
