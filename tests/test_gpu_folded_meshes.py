"""GPU: every planner on meshes that are no height field -- the helicoidal ramp (eight storeys over the same ground), the torus,
the vertical tube and the ramp far from the origin of tests/folded_meshes.py -- against the oracle, bit for bit.

The tile-batch engine cuts its tiles by coordinates, so a tile of the ramp is a column through every storey: up to 186 ghosts (199
on the moved ramp) where the terrain tilings of the other GPU tests have 54 at most.  That reaches what they never ran: the fall
back from k_tbv_solve to k_tb_solve_q above 64 ghosts, slices beyond 256 slots in k_tb_finalize, k_tb_warm and the paths-only
walk, and a finalize pass whose only finite values of a slice sit in its late ghost slots (tests/test_folded_meshes.py pins the
tilings and that such plans exist).  Shapes: V = 3840 / 2048 / 1920, batches of at most 192 plans."""
import functools
import re

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import folded_meshes as FM
from tests import replan_each_model as E
from tests.replan_model import bits
from tests.test_gpu_replan_each import oracle_all
from tests.test_gpu_replan_warm import OFF, each_step, ran_warm, recorded_by_tile_batch

pytestmark = pytest.mark.gpu
NAMES = sorted(FM.MAKERS)
ENGINES = {"tiled": "k_tile_round", "band": "k_step", "tile_batch": "k_tb_solve_q", "async": "k_plan_async"}
INF = float("inf")


@functools.lru_cache(maxsize=None)
def oracle(name, s, t, offset):
    """(the oracle's plan, its vector map)"""
    c = FM.case(name)
    r = c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=offset)
    return r, c.om.dijkstra_vector_map(r.pred)


def context(factory, name, engine=None, resident=True):
    ctx = factory()
    FM.case(name).upload(ctx)
    if engine:
        ctx.set_dijkstra_engine(engine)
    ctx.set_resident_outputs(resident)
    return ctx


def assert_batch_equals_oracle(ctx, name, out, seeds, targets, offset, tag, vecmaps=True):
    for k, (s, t) in enumerate(zip(seeds, targets)):
        r, vm = oracle(name, int(s), int(t), offset)
        at = (tag, k, int(s), int(t), offset)
        assert out["codes"][k] == r.code, at
        assert np.array_equal(out["paths"][k], r.path), at
        if out["dist"] is not None:
            bad = np.flatnonzero(bits(out["dist"][k]) != bits(r.dist))
            assert bad.size == 0, (at, "dist differs at", bad[:6].tolist(), out["dist"][k][bad[:6]].tolist(), r.dist[bad[:6]].tolist())
            assert np.array_equal(out["pred"][k], r.pred), at
            if vecmaps:
                assert np.array_equal(bits(ctx.download_output("vecmap", k)), bits(vm)), at


# ---- 1. Dijkstra on the four engines ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("name", NAMES)
def test_dijkstra_on_every_engine(gpu_ctx_factory, name, engine):
    """single plans (another storey, the whole lane, across the lane; opposite sides of the torus; the tube end to end) and a batch
    of 24, at the offsets 0.3, 0, -0.2 and +inf: code, path, dist, pred and vector map"""
    ctx = context(gpu_ctx_factory, name, engine)
    seeds, targets = FM.plan_pairs(name, 24)
    ran = set()
    for offset in (0.3, 0.0, -0.2, INF):
        # every call names its kernel: the engine's own, except that the band steps hand a negative offset to the tile rounds
        kernel = ENGINES["tiled"] if engine == "band" and offset < 0 else ENGINES[engine]
        for k in range(3):
            r, vm = oracle(name, int(seeds[k]), int(targets[k]), offset)
            out = ctx.plan_dijkstra(int(seeds[k]), int(targets[k]), offset, want_vecmap=True)
            at = (name, engine, offset, k)
            assert out.code == r.code == 0, at
            assert np.array_equal(out.path, r.path), at
            assert np.array_equal(bits(out.dist), bits(r.dist)) and np.array_equal(out.pred, r.pred), at
            assert np.array_equal(bits(out.vecmap), bits(vm)), at
            assert kernel in ctx.last_engine(), (at, ctx.last_engine())
            ran.add(ctx.last_engine())
        b = ctx.plan_dijkstra_batch(seeds, targets, offset, want_fields=True)
        assert kernel in ctx.last_engine(), (name, engine, offset, "batch", ctx.last_engine())
        ran.add(ctx.last_engine())
        assert_batch_equals_oracle(ctx, name, b, seeds, targets, offset, (name, engine))
    print("kernels", name, engine, sorted(ran))
    if name in ("ramp", "moved_ramp"):                                # the other storey is reached along the lane, not through the floor
        r, _ = oracle(name, int(seeds[0]), int(targets[0]), 0.3)
        assert len(r.path) >= 30 and r.dist[targets[0]] > 6.0
    ctx.close()


# ---- 2. which solve kernel ------------------------------------------------------------------------------------------------------

def test_a_tile_with_more_than_64_ghosts_keeps_the_batch_off_the_register_kernel(gpu_ctx_factory):
    assert FM.TILINGS["ramp"][1] > 64 >= FM.TILINGS["tube"][1]
    seeds, targets = FM.plan_pairs("ramp", 192, seed=9)
    ctx = context(gpu_ctx_factory, "ramp", "auto")
    auto = ctx.plan_dijkstra_batch(seeds, targets, 0.3, want_fields=True)   # 192 plans on 36 tiles: 32 per tile, k_tbv_solve's share
    assert "k_tb_solve_q" in ctx.last_engine(), ctx.last_engine()
    assert_batch_equals_oracle(ctx, "ramp", auto, seeds, targets, 0.3, "auto", vecmaps=False)
    ctx.set_dijkstra_engine("tile_batch")
    ctx.set_option("tb_kernel", 1)                                     # asked for, overridden
    asked = ctx.plan_dijkstra_batch(seeds, targets, 0.3, want_fields=True)
    assert "k_tb_solve_q" in ctx.last_engine(), ctx.last_engine()
    assert np.array_equal(bits(asked["dist"]), bits(auto["dist"])) and np.array_equal(asked["pred"], auto["pred"])
    ctx.close()
    ts, tt = FM.plan_pairs("tube", 64, seed=9)                         # the control: a mesh that fits
    ctl = context(gpu_ctx_factory, "tube", "tile_batch")
    ctl.set_option("tb_kernel", 1)
    out = ctl.plan_dijkstra_batch(ts, tt, 0.3, want_fields=True)
    assert "k_tbv_solve" in ctl.last_engine(), ctl.last_engine()
    assert_batch_equals_oracle(ctl, "tube", out, ts, tt, 0.3, "tube on k_tbv_solve")
    ctl.close()


# ---- 3. the finalize pass where a slice's only finite values are late ghosts ----------------------------------------------------

def late_batch(offset, n_late=64):
    """n_late of the late-ghost plans at this offset, dealt round the tiles, and as many random plans: (seeds, targets, the late ones)"""
    P = [p for p in FM.late_ghost_plans("ramp") if p["offset"] == offset]
    by_tile = {}
    for p in P:
        by_tile.setdefault(p["tile"], []).append(p)
    late = []
    while len(late) < n_late and any(by_tile.values()):
        for t in sorted(by_tile):
            if by_tile[t] and len(late) < n_late:
                late.append(by_tile[t].pop(len(by_tile[t]) // 2))
    rs, rt = FM.plan_pairs("ramp", len(late), seed=33)
    seeds = np.concatenate([np.array([p["seed"] for p in late], np.uint32), rs])
    targets = np.concatenate([np.array([p["target"] for p in late], np.uint32), rt])
    return seeds, targets, late


def resident_fields(ctx, n):
    return {w: np.stack([ctx.download_output(w, k) for k in range(n)]) for w in ("dist", "pred", "vecmap")}


def assert_fields_equal_oracle(got, seeds, targets, offset, tag):
    for k, (s, t) in enumerate(zip(seeds, targets)):
        r, vm = oracle("ramp", int(s), int(t), offset)
        bad = np.flatnonzero(bits(got["dist"][k]) != bits(r.dist))
        assert bad.size == 0, (tag, "plan", k, int(s), int(t), "dist differs at", bad[:6].tolist(), "device", got["dist"][k][bad[:6]].tolist(),
                               "oracle", r.dist[bad[:6]].tolist())
        assert np.array_equal(got["pred"][k], r.pred), (tag, k)
        assert np.array_equal(bits(got["vecmap"][k]), bits(vm)), (tag, k)


@pytest.mark.parametrize("offset", [0.02, 0.0, -1e-9])
def test_plans_that_end_on_the_late_ghosts_of_a_long_slice(gpu_ctx_factory, offset):
    """The front stops at the goal bound with its only popped vertices near a tile in that tile's ghost slots from 256 on: the tile
    was never activated, its owned slots and its first 136 ghosts are +inf, and the reference still gave the owned neighbours of
    those ghosts tentative values.  Then what the pass keeps for the next call on such pairs: the skipped
    stores of a second run, the reset of the distance buffer, a paths-only batch on what the reset left, and a batch that reaches
    the pairs that were unreached."""
    seeds, targets, late = late_batch(offset)
    n = len(seeds)
    assert len(late) >= 32 and len({p["tile"] for p in late}) >= 4 and n <= 512
    ctx = context(gpu_ctx_factory, "ramp", "tile_batch")
    out = ctx.plan_dijkstra_batch(seeds, targets, offset, want_fields=True)
    assert "k_tb_solve_q" in ctx.last_engine(), ctx.last_engine()
    first = ctx.tb_finalize_stats()
    for k, p in enumerate(late):                                       # the tentative values of the reference, on owned vertices of the silent tile
        assert np.isfinite(oracle("ramp", p["seed"], p["target"], offset)[0].dist[p["owned"]]).all()
        assert np.isfinite(out["dist"][k][p["owned"]]).all(), ("late-ghost plan", k, p["seed"], p["target"], "tile", p["tile"], "owned vertices left at +inf",
                                                                 p["owned"][~np.isfinite(out["dist"][k][p["owned"]])].tolist())
    assert_batch_equals_oracle(ctx, "ramp", out, seeds, targets, offset, "first run")
    # the same batch again: the map of the first pass vouches for the unreached pairs, their stores are skipped
    ctx.plan_dijkstra_batch(seeds, targets, offset)
    second = ctx.tb_finalize_stats()
    print("finalize counters", first, second)
    assert first["skipped_pairs"] == 0 and second["skipped_pairs"] > 0, (first, second)
    assert_fields_equal_oracle(resident_fields(ctx, n), seeds, targets, offset, "second run")
    # with the reset of the distance buffer by the pass, then a paths-only batch on what it left
    ctx.set_option("tb_fin_keep", 3)
    ctx.plan_dijkstra_batch(seeds, targets, offset)
    third = ctx.tb_finalize_stats()
    assert third["reset_pairs"] > 0, third
    assert_fields_equal_oracle(resident_fields(ctx, n), seeds, targets, offset, "with the reset")
    ctx.set_resident_outputs(False)
    ps, pt = FM.plan_pairs("ramp", n, seed=34)
    lazy = ctx.plan_dijkstra_batch(ps, pt, 0.3, want_fields=False)
    s4 = ctx.tb_finalize_stats()
    assert not s4["filled_at_start"] and s4["reset_pairs"] == 0 and s4["skipped_pairs"] == 0, s4     # it ran on what the pass left
    assert not ctx.device_output(0, 0)
    for k in range(n):
        r, _ = oracle("ramp", int(ps[k]), int(pt[k]), 0.3)
        assert lazy["codes"][k] == r.code and np.array_equal(lazy["paths"][k], r.path), k
    for k in (0, 1, n // 2, n - 1):                                    # exact up to goal_dist, +inf beyond
        r, _ = oracle("ramp", int(ps[k]), int(pt[k]), 0.3)
        cut = np.float32(np.float64(r.dist[pt[k]]) + 0.3)
        assert np.array_equal(bits(ctx.download_output("popped", k)), bits(np.where(r.dist <= cut, r.dist, np.float32(np.inf)))), k
    ctx.set_resident_outputs(True)
    ctx.set_option("tb_fin_keep", None)
    # the late batch once more (a new claim), then the same wave sources with robots far away: the waves now sweep the tiles they stopped
    # short of -- pairs that were unreached are reached, a bit that should have been 0 would hide their stores
    ctx.plan_dijkstra_batch(seeds, targets, offset)
    far = np.array([FM.ramp_vertex(0.98, 0.5) if s % FM.RAMP_NU < FM.RAMP_NU // 2 else FM.ramp_vertex(0.02, 0.5) for s in seeds], np.uint32)
    ctx.plan_dijkstra_batch(seeds, far, offset)
    last = ctx.tb_finalize_stats()
    print("after the far batch", last)
    assert_fields_equal_oracle(resident_fields(ctx, n), seeds, far, offset, "far robots after the late batch")
    ctx.close()


# ---- 4. the warm repair on long slices ------------------------------------------------------------------------------------------

def test_warm_repair_on_the_ramp(gpu_ctx_factory):
    """72 plans recorded by the tile-batch engine, a blocked patch on the fourth storey, the per-plan replan with the warm start:
    k_tb_warm reloads the slices beyond 256 words.  Every output equals a fresh plan's on a second context, and the oracle's."""
    seeds, targets, patch = FM.ramp_warm_batch()
    W = FM.FoldedWorld("ramp")
    A, B = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (A, B):
        W.upload(c)
        c.set_resident_outputs(True)
        c.set_option("replan_each_fresh_share", 1)
    A.set_option("replan_repair_engine", 5)
    A.set_option("replan_fresh_below", 0)
    recorded_by_tile_batch(A, seeds, targets, 0)
    old = oracle_all(W, seeds, targets)
    a, m, new = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), 0.0, "ramp warm")
    nr = int((m[0] == E.REPAIRED).sum())
    assert len(seeds) >= 70 and nr >= 20
    ran_warm(A, a, nr, "k_tb_solve_q")
    for p, r in enumerate(new):                                        # every plan against the oracle, not the first alone
        assert a["codes"][p] == r.code and np.array_equal(a["paths"][p], r.path), p
        assert np.array_equal(bits(a["dist"][p]), bits(r.dist)) and np.array_equal(a["pred"][p], r.pred), p
    A.close(); B.close()


# ---- 5. paths only --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ramp", "torus"])
def test_paths_only_batches(gpu_ctx_factory, name):
    ctx = context(gpu_ctx_factory, name, "tile_batch", resident=False)
    seeds, targets = FM.plan_pairs(name, 96, seed=21)
    for offset in (0.3, 0.0, INF):
        out = ctx.plan_dijkstra_batch(seeds, targets, offset, want_fields=False)
        assert "k_tb_solve_q" in ctx.last_engine() and not ctx.device_output(0, 0) and not ctx.device_output(0, 1)
        for k in range(96):
            r, _ = oracle(name, int(seeds[k]), int(targets[k]), offset)
            assert out["codes"][k] == r.code and np.array_equal(out["paths"][k], r.path), (name, offset, k)
    ctx.close()


# ---- 6. CVP ---------------------------------------------------------------------------------------------------------------------

def cvp_ends(name, n, seed=5):
    c = FM.case(name)
    s, t = FM.plan_pairs(name, n, seed)
    sf = np.array([FM.face_of(c, int(v)) for v in s], np.uint32)
    tf = np.array([FM.face_of(c, int(v)) for v in t], np.uint32)
    sp = np.stack([FM.face_point(c, int(f)) for f in sf])
    tp = np.stack([FM.face_point(c, int(f)) for f in tf])
    return sp, sf, tp, tf


def assert_cvp_equals(out_dist, out_pred, ref, at, cutface=None, direction=None, vecmap=None):
    assert np.array_equal(bits(out_dist), bits(ref.dist)) and np.array_equal(out_pred, ref.pred), at
    upd = ref.pred != np.arange(ref.pred.shape[0])
    if cutface is not None:
        assert np.array_equal(cutface[upd], ref.cutface[upd]), at
        assert np.array_equal(bits(direction[upd]), bits(ref.direction[upd])), at
        has = ref.has_vec.astype(bool)
        assert np.array_equal(bits(vecmap[has]), bits(ref.vecmap[has])), at


@pytest.mark.parametrize("name", NAMES)
def test_cvp_single_plans_a_wide_batch_and_walks(gpu_ctx_factory, name):
    """single plans on both step kernels (k_step's 8-lane replay, k_step_wide), a batch of 32 on the wide kernel, and the walks back
    over the batch's resident fields at two step widths -- the first pair of the ramps has the robot one storey above the goal"""
    c = FM.case(name)
    sp, sf, tp, tf = cvp_ends(name, 32)
    ctx = context(gpu_ctx_factory, name)
    refs = [c.om.cvp(c.weights, c.costs, c.vn, sp[k], int(sf[k]), int(tf[k])) for k in range(32)]
    for k, off in ((0, 0.3), (1, -0.2), (2, INF)):
        ref = refs[k] if off == 0.3 else c.om.cvp(c.weights, c.costs, c.vn, sp[k], int(sf[k]), int(tf[k]), goal_dist_offset=off)
        for wide in (0, 1):
            ctx.set_option("cvp_wide", wide)
            out = ctx.plan_cvp(sp[k], int(sf[k]), int(tf[k]), goal_dist_offset=off, want_vecmap=True)
            assert out.code == ref.code == 0, (name, k, wide)
            assert_cvp_equals(out.dist, out.pred, ref, (name, k, off, wide), out.cutface, out.direction, out.vecmap)
    ctx.set_option("cvp_wide", None)
    # The batch on both step kernels.  No counter names the kernel of a CVP call: the host takes k_step_wide from cvp_wide_min_batch =
    # 32 plans on (option unset), the option forces either; as in tests/test_gpu_cvp_wide.py the three runs must agree bit for bit.
    runs = {}
    for wide in (None, 1, 0):
        ctx.set_option("cvp_wide", wide)
        b = ctx.plan_cvp_batch(sp, sf, tf, want_fields=True, want_vecmap=True)
        assert b["stats"]["steps"] > 10, b["stats"]
        for k in range(32):
            assert b["codes"][k] == refs[k].code, (name, wide, k)
            assert_cvp_equals(b["dist"][k], b["pred"][k], refs[k], (name, "batch", wide, k))
            has = refs[k].has_vec.astype(bool)
            assert np.array_equal(bits(b["vecmap"][k][has]), bits(refs[k].vecmap[has])), (name, "batch vector map", wide, k)
        runs[wide] = b
    ctx.set_option("cvp_wide", None)
    for wide in (1, 0):
        assert np.array_equal(bits(runs[wide]["dist"]), bits(runs[None]["dist"])) and np.array_equal(runs[wide]["pred"], runs[None]["pred"])
        assert np.array_equal(bits(runs[wide]["vecmap"]), bits(runs[None]["vecmap"]))
    ctx.plan_cvp_batch(sp, sf, tf)                                     # (the walks below: over the fields of the default kernel)
    # The walks.  On the ramps most of the reference's walks end as "no path": a step of meshAhead leaves the lane or lands on the
    # storey 0.05 below or above, whatever the step width -- the device must stop at the same face and position.
    assert all(r.code == 0 for r in refs)
    for sw in (0.15, 0.04):
        walks = ctx.backtrack_cvp_batch(sp, sf, tp, tf, step_width=sw)
        assert len(walks) == 32
        done = steps = 0
        for k, (st, pos, face) in enumerate(walks):
            rc, ppos, pface = c.om.cvp_backtrack(refs[k].vecmap, refs[k].has_vec, sp[k], int(sf[k]), tp[k], int(tf[k]), step_width=sw)
            assert (st == 1) == (rc == 0), (name, sw, k)
            assert np.array_equal(face, pface) and np.array_equal(bits(pos), bits(ppos)), (name, sw, k)
            done += rc == 0
            steps += len(pface)
        print("walks", name, sw, "reached", done, "of 32, positions compared", steps)
        assert done >= 1 and steps >= 200, (name, sw, done, steps)
    ctx.close()


# ---- 7. what the upload reports -------------------------------------------------------------------------------------------------

TILES_LINE = re.compile(r"\[mnav\] tiles: size (\d+), (\d+) tiles, max owned (\d+), halo (\d+), edges (\d+) -> LDS (\d+) B \(solve\), (\d+) B \(finalize\)")


def pad(x, m):
    return (x + m - 1) // m * m


@pytest.mark.parametrize("tile_size", [None, 1024, 2048])
def test_upload_diagnostics_and_tiles_beyond_64_kb_of_lds(gpu_ctx_factory, capfd, tile_size):
    """the "tiles:" line of a verbose upload: the tile size asked for (no shrink: no tile of these meshes comes near 150 KB, see
    below), and the LDS of the finalize pass as mnav_finalize.h adds it up.  Tiles of 2048 vertices push the solve and the finalize
    kernels beyond the 64 KB a kernel gets without the dynamic-LDS attribute; the tile rounds and the asynchronous engine plan on them."""
    c = FM.case("ramp")
    ctx = gpu_ctx_factory()
    ctx.set_option("verbose", 1)
    if tile_size:
        ctx.set_option("tile_size", tile_size)
    capfd.readouterr()
    c.upload(ctx)
    err = capfd.readouterr().err
    ctx.set_option("verbose", None)
    m = TILES_LINE.search(err)
    assert m, err
    size, ntiles, nv, nh, ne, solve, fin = (int(x) for x in m.groups())
    print("tiles line:", m.group(0))
    assert size == (tile_size or 512) and nv <= size and ntiles >= -(-c.mesh.V // size)
    assert fin == solve + 4 * pad(nv, 4) + 4 * pad(nv + nh, 4) + 8 * nv
    if tile_size == 2048:                                             # both kernels need the attribute
        assert 64 * 1024 < solve < fin <= 150 * 1024, (solve, fin)
    elif tile_size == 1024:                                           # the finalize kernel alone
        assert solve <= 64 * 1024 < fin <= 150 * 1024, (solve, fin)
    else:
        assert fin <= 64 * 1024
    seeds, targets = FM.plan_pairs("ramp", 8)
    for engine in ("tiled", "async"):
        ctx.set_dijkstra_engine(engine)
        out = ctx.plan_dijkstra_batch(seeds, targets, 0.3, want_fields=True)
        assert ENGINES[engine] in ctx.last_engine()
        assert_batch_equals_oracle(ctx, "ramp", out, seeds, targets, 0.3, (engine, tile_size), vecmaps=False)
    ctx.close()
