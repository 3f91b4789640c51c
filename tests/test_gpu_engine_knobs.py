"""The per-plan engines under every band width and launch shape: "the schedule changes, never the result" (mnav_options.h),
held on the device for the band steps (k_step; k_cvp_ctl + k_step_wide: CVP, band Dijkstra, the inflation wave), the
tile rounds (k_tile_round) and the asynchronous tiles (k_plan_async), the way tests/test_gpu_tbv_parity.py and its neighbours hold
the tile-batch engine.  What real concurrency adds to the serial CPU model (tests/test_schedule_model.py): 8 lanes per vertex, the wide
kernel's face / vertex phases, work-list appends, provisional pop keys -- at the band extremes where the scheme's safety nets live: a
band of 0.05 mean edge weights has hundreds of near-empty bands (band advance, arming), a band wider than the whole field settles
everything in one band with maximal cascades below the front (band shrink, "still moving" cuts, the post-arming repair).

Every comparison is with the oracle, bit for bit, with no tolerance and no "skip if refused": tests/test_engine_knobs_model.py shows on
the CPU model that each input listed in tests/engine_knob_cases.py ends with code 0 and the oracle's bits, so INTERNAL_ERROR (a
RuntimeError here) in any of them is the device's own.  Every test restores what it changed."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import engine_knob_cases as K

pytestmark = pytest.mark.gpu
INF = K.INF
CASES = ("L", "A", "H", "X", "P")
OPTIONS_TOUCHED = ("cvp_wide", "cvp_groups", "blocks_per_plan", "wide_waves", "no_graph", "debug_chunk", "tile_band", "rounds_band_mult",
                   "tile_blocks", "async_band_mult", "async_wg_per_cu", "async_wg_per_plan", "async_max_s")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def contexts(gpu_ctx_factory):
    made = {}
    for name in CASES:                                                 # (built here, so that no test's time is a context's)
        made[name] = gpu_ctx_factory()
        K.case(name).upload(made[name])
    yield made.__getitem__
    for ctx in made.values():
        ctx.close()


@contextlib.contextmanager
def knobs(ctx, band=None, engine=None, **options):
    """options, band width and engine for the block; the defaults again afterwards, whatever happened inside"""
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        if band is not None:
            ctx.set_band_width(band)
        if engine is not None:
            ctx.set_dijkstra_engine(engine)
        yield ctx
    finally:
        for name in options:
            ctx.set_option(name, None)
        ctx.set_band_width(0)
        ctx.set_dijkstra_engine("auto")


# ---- the oracle's answers, computed once per process and never written to
@functools.lru_cache(maxsize=None)
def ref_cvp(name, sp, sf, tf, offset):
    c = K.case(name)
    return c.om.cvp(c.weights, c.costs, c.vn, np.array(sp, np.float32), sf, tf, goal_dist_offset=offset, invalid=c.invalid)


@functools.lru_cache(maxsize=None)
def ref_dijkstra(name, s, t, offset, limit=1.0):
    c = K.case(name)
    r = c.om.dijkstra(c.weights, c.costs, s, t, goal_dist_offset=offset, cost_limit=limit, invalid=c.invalid)
    return r, c.om.dijkstra_vector_map(r.pred)


def batch_refs(name, offset):
    sps, sfs, tfs = K.cvp_batch(name)
    return [ref_cvp(name, tuple(float(x) for x in sps[k]), int(sfs[k]), int(tfs[k]), offset) for k in range(len(sfs))]


def assert_cvp_fields(at, ref, code, dist, pred, cutface, direction, vecmap):
    """code; potential; predecessors; cutting faces and directions where the reference set them; the vector map where it has an entry"""
    assert code == ref.code, (at, code, ref.code)
    if ref.code == O.INVALID_START or ref.code == O.INVALID_GOAL:      # answered before any field exists
        return
    d = bits(dist) != bits(ref.dist)
    assert not d.any(), (at, "potential", int(d.sum()), int(np.argmax(d)))
    d = pred != ref.pred
    assert not d.any(), (at, "predecessors", int(d.sum()), int(np.argmax(d)))
    upd = ref.pred != np.arange(len(ref.pred))
    d = upd & (cutface != ref.cutface)
    assert not d.any(), (at, "cutting faces", int(d.sum()), int(np.argmax(d)))
    d = upd & (bits(direction) != bits(ref.direction))
    assert not d.any(), (at, "directions", int(d.sum()), int(np.argmax(d)))
    has = ref.has_vec.astype(bool)
    d = has & (bits(vecmap) != bits(ref.vecmap)).any(axis=1)
    assert not d.any(), (at, "vector map", int(d.sum()), int(np.argmax(d)))


def assert_cvp_single(at, out, ref):
    assert_cvp_fields(at, ref, out.code, out.dist, out.pred, out.cutface, out.direction, out.vecmap)


def assert_cvp_batch(at, ctx, b, refs):
    """EVERY plan of the batch, every field the call returns, and the cutting faces / directions out of the resident outputs"""
    assert len(b["codes"]) == len(refs)
    for k, ref in enumerate(refs):
        if ref.code == O.INVALID_START:
            assert b["codes"][k] == ref.code, (at, k)
            continue
        assert_cvp_fields(at + (k,), ref, int(b["codes"][k]), b["dist"][k], b["pred"][k], ctx.download_output("cutface", k),
                          ctx.download_output("direction", k), b["vecmap"][k])


def assert_dijkstra_single(at, out, ref, vm):
    assert out.code == ref.code, (at, out.code, ref.code)
    d = bits(out.dist) != bits(ref.dist)
    assert not d.any(), (at, "potential", int(d.sum()), int(np.argmax(d)))
    d = out.pred != ref.pred
    assert not d.any(), (at, "predecessors", int(d.sum()), int(np.argmax(d)))
    assert np.array_equal(out.path, ref.path), (at, "path", len(out.path), len(ref.path))
    assert bits(out.stats["goal_dist"]) == bits(ref.stats["goal_dist"]), (at, "goal_dist", out.stats["goal_dist"], ref.stats["goal_dist"])
    d = (bits(out.vecmap) != bits(vm)).any(axis=1)
    assert not d.any(), (at, "vector map", int(d.sum()), int(np.argmax(d)))


def assert_dijkstra_batch(at, name, b, seeds, targets, offset):
    for k in range(len(seeds)):
        ref, _ = ref_dijkstra(name, int(seeds[k]), int(targets[k]), offset)
        assert b["codes"][k] == ref.code, (at, k)
        d = bits(b["dist"][k]) != bits(ref.dist)
        assert not d.any(), (at, k, "potential", int(d.sum()), int(np.argmax(d)))
        assert np.array_equal(b["pred"][k], ref.pred), (at, k, "predecessors")
        assert np.array_equal(b["paths"][k], ref.path), (at, k, "path")


# ---- a. CVP band width: the 8-lane replay and the wide kernel
@pytest.mark.parametrize("combo", K.CVP_SINGLE, ids=K.ident)
def test_cvp_band_width_on_both_step_kernels(contexts, combo):
    name, k, mult, offset = combo
    c, ctx, p = K.case(name), contexts(name), K.cvp_plans(name)[k]
    ref = ref_cvp(name, p.sp, p.sf, p.tf, offset)
    for wide in (0, 1):
        with knobs(ctx, band=K.band_width(c, mult), cvp_wide=wide):
            out = ctx.plan_cvp(p.seed_pos, p.sf, p.tf, goal_dist_offset=offset)
        assert_cvp_single(combo + ("cvp_wide", wide), out, ref)
        assert out.stats["steps"] > 0 and out.stats["bands"] > 0
        if mult == 0.05:                                               # the field spans over a thousand of these widths
            assert out.stats["bands"] > 100, out.stats


# ---- b. a CVP batch of 34 on the wide kernel, one, default and two stream branches
@pytest.mark.parametrize("combo", K.CVP_BATCH, ids=K.ident)
def test_cvp_batch_band_width_and_groups_on_the_wide_kernel(contexts, combo):
    """Every plan of the batch and every field, per stream-branch count, on the forced wide kernel (the two seeds beside the mesh never
    reach the device: 32 plans step, in two branches of 16 under cvp_groups = 2).  k_step_repair, the third kernel of a wide step, has
    no plan to work on here or anywhere: k_cvp_ctl lists a plan for it in a step with ctl.repair above 2 or with a seed mask, and
    controller_core sets repair 3 / 5 only for plans with a seed mask -- the inflation wave, which steps on k_step.  No test of this
    file depends on its launch."""
    name, mult, offset = combo
    c, ctx = K.case(name), contexts(name)
    sps, sfs, tfs = K.cvp_batch(name)
    refs = batch_refs(name, offset)
    assert sum(r.code == O.INVALID_START for r in refs) >= 1 and sum(r.code == O.SUCCESS for r in refs) >= 24
    for groups in (None, 1, 2):                                        # 2: two stream branches in the captured graph
        with knobs(ctx, band=K.band_width(c, mult), cvp_groups=groups, cvp_wide=1):
            b = ctx.plan_cvp_batch(sps, sfs, tfs, goal_dist_offset=offset, want_fields=True, want_vecmap=True)
            assert_cvp_batch(combo + ("cvp_groups", groups), ctx, b, refs)
        assert b["stats"]["steps"] > 0


# ---- c. launch shape of the band steps
def test_blocks_per_plan_on_both_step_kernels(contexts):
    name, mult, offset = K.SHAPE_CASE, K.SHAPE_MULT, K.SHAPE_OFFSET
    assert (name, 0, mult, offset) in K.CVP_SINGLE and mult is None
    ctx, p = contexts(name), K.cvp_plans(name)[0]
    ref = ref_cvp(name, p.sp, p.sf, p.tf, offset)
    for wide in (0, 1):
        launches = {}
        for blocks in (1, 4, 4096):                                    # (the launcher clamps to 4 .. 4096)
            with knobs(ctx, cvp_wide=wide, blocks_per_plan=blocks):
                out = ctx.plan_cvp(p.seed_pos, p.sf, p.tf, goal_dist_offset=offset)
            assert_cvp_single(("blocks_per_plan", blocks, "cvp_wide", wide), out, ref)
            launches[blocks] = out.stats["launches"]
        assert launches[1] == launches[4], launches


@pytest.mark.parametrize("waves,plans", [(1, 12), (2, 20), (4096, K.BATCH_N)])
def test_wide_waves_on_the_batch(contexts, waves, plans):
    """One wave walks every plan's work list round by round: the serial extreme.  The two serial runs take the first 12 and 20 plans of
    the batch (the one beside the mesh among them), to stay as quick as the rest of the file; all of them on the forced wide kernel."""
    (name, mult, offset), = K.CVP_BATCH_SHAPE
    c, ctx = K.case(name), contexts(name)
    sps, sfs, tfs = (a[:plans] for a in K.cvp_batch(name))
    with knobs(ctx, band=K.band_width(c, mult), wide_waves=waves, cvp_wide=1):
        b = ctx.plan_cvp_batch(sps, sfs, tfs, goal_dist_offset=offset, want_fields=True, want_vecmap=True)
        assert_cvp_batch(("wide_waves", waves), ctx, b, batch_refs(name, offset)[:plans])


def test_no_graph_and_debug_chunk_equal_the_graph_run(contexts):
    """The kernels rotate their control and counter blocks by launch % 6 and every chunk starts its launches at 0: debug_chunk is
    rounded UP to a multiple of 6, and a value below 1 is the default chunk (run_chunk / steps_per_chunk in mnav.hip).  Launch by
    launch, whatever the chunk, the outputs are those of the replayed graph."""
    (name, mult, offset), = K.CVP_BATCH_SHAPE                         # (the single plans at this width and offset: K.CVP_SINGLE, K.DIJKSTRA_BAND)
    assert (name, 0, mult, offset) in K.CVP_SINGLE and (name, 0, mult, offset) in K.DIJKSTRA_BAND and mult is None
    ctx, p = contexts(name), K.cvp_plans(name)[0]
    ref = ref_cvp(name, p.sp, p.sf, p.tf, offset)
    sps, sfs, tfs = K.cvp_batch(name)
    refs = batch_refs(name, offset)
    s, t, lim = K.dijkstra_plans(name)[0]
    dref, dvm = ref_dijkstra(name, s, t, offset, lim)
    for wide in (0, 1):
        with knobs(ctx, cvp_wide=wide):
            graph = ctx.plan_cvp(p.seed_pos, p.sf, p.tf, goal_dist_offset=offset)
        assert_cvp_single(("graph", wide), graph, ref)
        assert graph.stats["launches"] % 96 == 0
        launches = {}
        for chunk in (None, 6, 12, 1, 7, 0):
            with knobs(ctx, cvp_wide=wide, no_graph=1, debug_chunk=chunk):
                out = ctx.plan_cvp(p.seed_pos, p.sf, p.tf, goal_dist_offset=offset)
            at = ("no_graph", "debug_chunk", chunk, "cvp_wide", wide)
            assert_cvp_single(at, out, ref)
            for f in ("dist", "direction", "vecmap"):
                assert np.array_equal(bits(getattr(out, f)), bits(getattr(graph, f))), at + (f,)
            assert np.array_equal(out.pred, graph.pred) and np.array_equal(out.cutface, graph.cutface), at
            assert out.stats["launches"] > 0 and out.stats["launches"] % 6 == 0, (at, out.stats["launches"])
            launches[chunk] = out.stats["launches"]
        assert launches[None] % 96 == 0 and launches[0] % 96 == 0, launches     # unset and 0: the default chunk
        assert launches[7] % 12 == 0 and launches[12] % 12 == 0, launches       # 7 is rounded up to 12, not down to 6
    for chunk in (None, 7):                                            # the batch on the wide kernel, launch by launch
        with knobs(ctx, no_graph=1, debug_chunk=chunk, cvp_wide=1):
            b = ctx.plan_cvp_batch(sps, sfs, tfs, goal_dist_offset=offset, want_fields=True, want_vecmap=True)
            assert_cvp_batch(("no_graph batch", chunk), ctx, b, refs)
        assert b["stats"]["launches"] % 6 == 0
    for chunk in (None, 7, 0):                                         # and k_step on a Dijkstra plan
        with knobs(ctx, engine="band", no_graph=1, debug_chunk=chunk):
            out = ctx.plan_dijkstra(s, t, offset, lim, want_fields=True, want_vecmap=True)
            assert "k_step" in ctx.last_engine(), ctx.last_engine()
        assert_dijkstra_single(("no_graph dijkstra", chunk), out, dref, dvm)
        assert out.stats["launches"] % 6 == 0


# ---- d. band Dijkstra
@pytest.mark.parametrize("combo", K.DIJKSTRA_BAND, ids=K.ident)
def test_band_dijkstra_band_width(contexts, combo):
    """k_step by name; a negative offset goes to the tile rounds (tests/test_gpu_folded_meshes.py), by name too"""
    name, k, mult, offset = combo
    c, ctx = K.case(name), contexts(name)
    s, t, lim = K.dijkstra_plans(name)[k]
    ref, vm = ref_dijkstra(name, s, t, offset, lim)
    assert ref.code == (O.NO_PATH_FOUND if K.unreachable(name, k) else O.SUCCESS)
    with knobs(ctx, band=K.band_width(c, mult), engine="band"):
        out = ctx.plan_dijkstra(s, t, offset, lim, want_fields=True, want_vecmap=True)
        engine = ctx.last_engine()
    assert ("k_tile_round" if offset < 0 else "k_step") in engine, (combo, engine)
    assert_dijkstra_single(combo, out, ref, vm)


# ---- e. tile rounds
TILE_KNOBS = [("tile_band", m) for m in (0.25, 60, 1e6)] + [("rounds_band_mult", m) for m in (0.25, 64)]


@pytest.mark.parametrize("name", K.DIJKSTRA_CASES)
@pytest.mark.parametrize("knob", TILE_KNOBS, ids=K.ident)
def test_tile_rounds_band_and_blocks(contexts, name, knob):
    c, ctx = K.case(name), contexts(name)
    option, value = knob
    if option == "tile_band":
        value = value * K.mean_weight(c)
    offset = 0.3
    seeds, targets = K.dijkstra_batch(name, 9)
    for blocks in (1, 2, 10 ** 6):                                     # (the last: clamped to the tile count)
        with knobs(ctx, engine="tiled", tile_blocks=blocks, **{option: value}):
            for s, t, lim in K.dijkstra_plans(name):
                out = ctx.plan_dijkstra(s, t, offset, lim, want_fields=True, want_vecmap=True)
                assert "k_tile_round" in ctx.last_engine(), ctx.last_engine()
                assert_dijkstra_single((name, knob, blocks, s, t), out, *ref_dijkstra(name, s, t, offset, lim))
            b = ctx.plan_dijkstra_batch(seeds, targets, offset, want_fields=True)
            assert "k_tile_round" in ctx.last_engine(), ctx.last_engine()
        assert_dijkstra_batch((name, knob, blocks), name, b, seeds, targets, offset)


# ---- f. asynchronous tiles
@pytest.mark.parametrize("name", K.DIJKSTRA_CASES)
@pytest.mark.parametrize("band_mult", [0, 0.25, 16])
@pytest.mark.parametrize("wg_per_plan", [1, 4])
def test_async_tiles_band_and_workgroups(contexts, name, band_mult, wg_per_plan):
    """k_plan_async is persistent and its workgroups wait for tickets (mnav_async.h, the loop around `e = aq::ld(ring_p + i)`), so
    these runs stay at or below the built-in workgroup counts (1 per CU instead of 4; 1 or 4 per plan instead of up to 128), and
    async_max_s = 5 makes a stuck kernel give up by itself: abort 2 surfaces as a RuntimeError and the test fails.

    Why one workgroup alone (async_wg_per_plan = 1: block p serves plan p) always finds its next ticket filed: work[p] counts the
    tickets filed and not yet retired, and a solver gives its own count back only AFTER its wake-ups have filed theirs (route / push,
    drained).  Alone, every ticket below head is retired, so work[p] after the give-back is tail - head.  If that is above zero, slot
    `head` was stored by this very workgroup before it came back to pop: the first look finds it.  If it is zero, the same workgroup
    advances the band before it pops again -- it either files the next band's tickets (same argument) or finds nothing parked, finishes
    the plan (done = 1) and, at its next pop, leaves the poll loop through the `done` / done_plans looks at every 8th spin.  It never
    waits for a ticket that only another workgroup could file.  With 4 per plan a popper may wait for a ticket a busy neighbour has
    yet to file; that neighbour never waits for the popper, so the wait ends.

    A silent re-run on the tile rounds (ring overflow, abort 5) would name k_tile_round: the engine is asserted by name."""
    ctx = contexts(name)
    offset = 0.3
    with knobs(ctx, engine="async", async_max_s=5, async_wg_per_cu=1, async_wg_per_plan=wg_per_plan, async_band_mult=band_mult):
        for s, t, lim in K.dijkstra_plans(name):                       # batches of 1
            out = ctx.plan_dijkstra(s, t, offset, lim, want_fields=True, want_vecmap=True)
            assert "k_plan_async" in ctx.last_engine(), ctx.last_engine()
            assert out.stats["launches"] == 1
            assert_dijkstra_single((name, band_mult, wg_per_plan, s, t), out, *ref_dijkstra(name, s, t, offset, lim))
        for n in (8, 33):                                              # (from 32 plans on the default band changes)
            seeds, targets = K.dijkstra_batch(name, n)
            b = ctx.plan_dijkstra_batch(seeds, targets, offset, want_fields=True)
            assert "k_plan_async" in ctx.last_engine(), ctx.last_engine()
            assert_dijkstra_batch((name, band_mult, wg_per_plan, n), name, b, seeds, targets, offset)


# ---- g. the inflation wave: its band is the inflation radius
@pytest.mark.parametrize("radius", K.RADII)
def test_inflation_wave_radius_and_launch_shape(contexts, radius):
    name = "L"
    c, ctx = K.case(name), contexts(name)
    lethal = K.lethal_of(name)
    cfg = O.InflationCfg.defaults()
    cfg.inflation_radius = radius
    cost, dist, vec = c.om.inflation(lethal, c.edge_dist, cfg)
    vec = np.ascontiguousarray(vec, np.float32)
    ref_has = ~(vec == 0).all(axis=1)                                  # (the oracle's map writes the zero vector where it has no entry)
    assert ref_has.sum() > lethal.sum() // 2
    ctx.layer_upload(0, np.zeros(c.mesh.V, np.float32), lethal)
    for options in (dict(blocks_per_plan=4), dict(blocks_per_plan=4096), dict(no_graph=1), dict(no_graph=1, debug_chunk=7)):
        at = (radius, tuple(options.items()))
        with knobs(ctx, **options):                                    # the wave launches 12 x blocks_per_plan workgroups, at most 8192
            st = ctx.layer_inflation(1, 0, inflation_radius=radius)
            co, le, d = ctx.layer_download(1, distances=True)
            dv, has = ctx.layer_vectors(1)
        assert st["steps"] > 0
        bad = bits(d) != bits(dist)
        assert not bad.any(), (at, "distances", int(bad.sum()), int(np.argmax(bad)))
        assert np.array_equal(bits(co), bits(cost)), (at, "costs")
        assert np.array_equal(le, lethal), (at, "lethal flags")
        same = (bits(dv) == bits(vec)).all(axis=1) | (np.isnan(dv).any(axis=1) & np.isnan(vec).any(axis=1))
        bad = ref_has & ~(same & (has == 1))
        assert not bad.any(), (at, "vectors", int(bad.sum()), int(np.argmax(bad)))
        bad = ~ref_has & (has == 1) & (bits(dv) != 0).any(axis=1)      # an entry the reference does not have
        assert not bad.any(), (at, "has-entry flags", int(bad.sum()), int(np.argmax(bad)))
    # the wave worked in plan slot 0: a plan afterwards is untouched by it
    p = K.cvp_plans(name)[0]
    assert_cvp_single(("after the wave", radius), ctx.plan_cvp(p.seed_pos, p.sf, p.tf), ref_cvp(name, p.sp, p.sf, p.tf, 0.3))


def test_no_knob_leaked(contexts):
    """(runs last) the module's contexts are back at their defaults"""
    for name in CASES:
        ctx = contexts(name)
        assert all(ctx.get_option(o) is None for o in OPTIONS_TOUCHED), name
        assert ctx.get_option("dijkstra_engine") == 3.0
