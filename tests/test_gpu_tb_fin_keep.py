"""What the tile-batch finalize pass keeps from one call to the next (option tb_fin_keep): it stores
nothing for a (tile, plan) whose wave stays away again when the slot's arrays hold the unreached pattern from the pass before
(bit 0, the default), and it can reset the distance buffer itself so that the next call starts without a fill and without a second
buffer (bit 1; off by default, it gains no time).  Neither may change a bit of any output.

Shapes: terrain(96) = 9 216 vertices (about 80 tiles of 120 rows), 130 plans = two full blocks of 64 plans + 2, resident outputs
with vector maps.  Two batches A and B with different goals (the wave sources):

  A: 122 small waves in the upper left corner, 8 wide ones that start on the right and sweep most of the mesh
  B: 130 small waves in the upper right corner

The engine puts the plans into slots by the tile of their source, so which plan of A shares a slot with which plan of B is not
known here; the layout makes the four transitions of a (tile, slot) pair occur under EVERY pairing (transitions_hold):
  reached -> reached      a slot that held a wide wave of A: that wave reached something every wave of B reaches
  reached -> unreached    a slot with two small waves (there are 114 at least): tiles on the left, around a vertex every small wave of A reaches
  unreached -> reached    the same slot: tiles on the right
  unreached -> unreached  the same slot: tiles at the bottom of the mesh
"Unreached" is the engine's word, not the oracle's: its distance slice of the tile, ghosts included, is all +inf, and the engine
may run up to a band (two tile widths) beyond the oracle's finite potentials.  So the CPU check keeps kMargin = 40 grid cells
between a region it calls unreached and every finite potential of the waves concerned: 24 for the band, 16 for a tile (11 x 11
vertices) with its ghost ring around the vertex in question.  What the engine really did is then read from the counters.

Every comparison is exact: bits of dist and vecmap, ids of pred.  The expected values come from the oracle and from a fresh
context that ran the last batch alone; both are computed once per module."""
import functools
import threading
import time

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests.common import terrain_case

OFFSET = 0.3
N = 130
N_WIDE = 8
kMargin = 40


class World:
    def __init__(self):
        self.case = c = terrain_case(96, 1)
        m = c.mesh
        G = m.N

        def vid(i, j):
            return (np.asarray(j) * G + np.asarray(i)).astype(np.uint32)

        def window(ci, cj, n):                                          # n distinct sources in a 13-wide window around (ci, cj)
            k = np.arange(n)
            return ci - 6 + k % 13, cj - 5 + k // 13

        # A: small waves top left (the robot 8 rows below the source: a disc of about 11 cells), 8 wide ones from the right
        ai, aj = window(14, 80, N - N_WIDE)
        wi, wj = 70 + 2 * np.arange(N_WIDE), np.full(N_WIDE, 70)
        self.seeds_a = np.concatenate([vid(ai, aj), vid(wi, wj)])
        self.targets_a = np.concatenate([vid(ai, aj - 8), vid(wi - 45, wj - 30)])
        self.small_a = np.arange(N) < N - N_WIDE
        # B: small waves top right
        bi, bj = window(81, 80, N)
        self.seeds_b, self.targets_b = vid(bi, bj), vid(bi, bj - 8)
        # other robot vertices for the replans: two rows further down
        self.targets_a2 = np.concatenate([vid(ai, aj - 10), vid(wi - 45, wj - 32)])
        self.grid = G

    @functools.cached_property
    def ref_a(self):
        return self.oracle(self.seeds_a, self.targets_a)

    @functools.cached_property
    def ref_b(self):
        return self.oracle(self.seeds_b, self.targets_b)

    def oracle(self, seeds, targets):
        c = self.case
        out = []
        for s, t in zip(seeds, targets):
            r = c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=OFFSET)
            out.append((r, c.om.dijkstra_vector_map(r.pred)))
        return out

    def context(self, resident=True, keep=None):
        """keep: option tb_fin_keep (None: the default, 1 = the skipped stores alone; 3 adds the reset of the distance buffer)"""
        ctx = capi.MnavContext(0)
        self.case.upload(ctx)
        ctx.set_dijkstra_engine("tile_batch")
        ctx.set_resident_outputs(resident)
        if keep is not None:
            ctx.set_option("tb_fin_keep", keep)
        return ctx


@functools.lru_cache(maxsize=1)
def world():
    return World()


def dilate(mask, r):
    """L-infinity dilation of a boolean grid by r cells"""
    out = mask.copy()
    for axis in (0, 1):
        acc = out.copy()
        for s in range(1, r + 1):
            lo = [slice(None)] * 2
            hi = [slice(None)] * 2
            lo[axis], hi[axis] = slice(s, None), slice(None, -s)
            acc[tuple(lo)] |= out[tuple(hi)]
            acc[tuple(hi)] |= out[tuple(lo)]
        out = acc
    return out


def transitions_hold(W):
    """the four transitions among (tile, slot) pairs, under every pairing of A's plans with B's, from the oracle's potentials"""
    G = W.grid
    fin_a = np.array([np.isfinite(r.dist).reshape(G, G) for r, _ in W.ref_a])
    fin_b = np.array([np.isfinite(r.dist).reshape(G, G) for r, _ in W.ref_b])
    small_a, wide_a = fin_a[W.small_a], fin_a[~W.small_a]
    far_from_a = ~dilate(small_a.any(axis=0), kMargin)
    far_from_b = ~dilate(fin_b.any(axis=0), kMargin)
    every_a, every_b = small_a.all(axis=0), fin_b.all(axis=0)
    got = dict(
        slots_with_two_small_waves=bool(W.small_a.sum() + N > N),          # (pigeonhole: B's waves are all small)
        reached_reached=bool(all((w & b).any() for w in wide_a for b in fin_b)),
        reached_unreached=bool((every_a & far_from_b).any()),
        unreached_reached=bool((every_b & far_from_a).any()),
        unreached_unreached=bool((far_from_a & far_from_b).any()),
    )
    print("transitions", got, "finite vertices per plan: A small %.0f, A wide %.0f, B %.0f"
          % (small_a.sum(axis=(1, 2)).mean(), wide_a.sum(axis=(1, 2)).mean(), fin_b.sum(axis=(1, 2)).mean()))
    return got


def test_the_two_batches_show_all_four_transitions_on_the_cpu():
    W = world()
    assert (W.seeds_a != W.targets_a).all() and (W.seeds_b != W.targets_b).all() and (W.seeds_a != W.targets_a2).all()
    assert len(set(W.seeds_a)) == N and len(set(W.seeds_b)) == N
    assert all(r.code == 0 for r, _ in W.ref_a) and all(r.code == 0 for r, _ in W.ref_b)
    assert all(transitions_hold(W).values())


# ---- the device -----------------------------------------------------------------------------------------------------------------

def batch(ctx, seeds, targets, fields=False):
    out = ctx.plan_dijkstra_batch(seeds, targets, OFFSET, want_fields=fields)
    assert out["rc"] == 0 and (out["codes"] == 0).all(), (out["rc"], out["codes"])
    return out


def fields(ctx, n=N, vecmaps=True):
    """dist, pred (and vector map) of every plan, as left on the device"""
    whats = ("dist", "pred") + (("vecmap",) if vecmaps else ())
    return {w: np.stack([ctx.download_output(w, k) for k in range(n)]) for w in whats}


def assert_same_fields(got, want, tag):
    for w in want:
        a, b = got[w], want[w]
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32))
        if not same:
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError((tag, w, "first differences (plan, vertex[, component])", bad[:5].tolist(), "of", len(bad)))


def assert_same_paths(a, b, tag):
    assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["path_len"], b["path_len"]), tag
    assert all(np.array_equal(a["paths"][k], b["paths"][k]) for k in range(len(a["codes"]))), tag


@functools.lru_cache(maxsize=1)
def fresh_b():
    """a fresh context that ran only batch B: outputs, paths and counters"""
    W = world()
    with W.context() as ctx:
        out = batch(ctx, W.seeds_b, W.targets_b)
        st = ctx.tb_finalize_stats()
        return dict(out=out, fields=fields(ctx), stats=st)


@pytest.mark.gpu
def test_two_fresh_batches_in_a_row():
    W = world()
    assert all(transitions_hold(W).values())                             # on the CPU, before the device runs
    want = fresh_b()
    assert want["stats"]["skipped_pairs"] == 0 and want["stats"]["filled_at_start"], want["stats"]   # a first call keeps nothing
    with W.context() as ctx:
        a = batch(ctx, W.seeds_a, W.targets_a)
        sa = ctx.tb_finalize_stats()
        assert "k_tb" in ctx.last_engine(), ctx.last_engine()
        b = batch(ctx, W.seeds_b, W.targets_b)
        sb = ctx.tb_finalize_stats()
        print("counters", sa, sb, "engine", ctx.last_engine())
        got = fields(ctx)
        for k, (r, vm) in enumerate(W.ref_b):                            # the oracle
            at = (k, int(W.seeds_b[k]), int(W.targets_b[k]))
            assert np.array_equal(got["dist"][k].view(np.uint32), r.dist.view(np.uint32)), at
            assert np.array_equal(got["pred"][k], r.pred), at
            assert np.array_equal(got["vecmap"][k].view(np.uint32), vm.view(np.uint32)), at
            assert np.array_equal(b["paths"][k], r.path), at
        assert_same_fields(got, want["fields"], "B after A")             # the fresh context
        assert_same_paths(b, want["out"], "B after A")
        assert all(np.array_equal(a["paths"][k], W.ref_a[k][0].path) for k in range(N))
        assert sa["skipped_pairs"] == 0 and sa["filled_at_start"] and sa["reset_pairs"] == 0, sa     # (the default: stores skipped, no reset)
        assert sb["skipped_pairs"] > 0 and not sb["filled_at_start"] and sb["reset_pairs"] == 0, sb
        # the same pair of batches with each half on and off: the same bits, and the counters say which half ran
        # (no fill at the start either way: without the reset the second buffer is filled behind every call, as before)
        reached = set()
        for keep in (0, 1, 2, 3):
            ctx.set_option("tb_fin_keep", keep)
            batch(ctx, W.seeds_a, W.targets_a)
            batch(ctx, W.seeds_b, W.targets_b)
            s = ctx.tb_finalize_stats()
            print("tb_fin_keep", keep, s)
            assert s["skipped_pairs"] == (sb["skipped_pairs"] if keep & 1 else 0) and not s["filled_at_start"], (keep, s)
            assert (s["reset_pairs"] > 0) == bool(keep & 2), (keep, s)
            if keep & 2:
                reached.add(s["reset_pairs"])
            assert_same_fields(fields(ctx), want["fields"], "tb_fin_keep %d" % keep)
        assert len(reached) == 1, reached                                # the same pairs were reached, whatever was skipped


def single_async_plan(ctx, W):
    ctx.set_dijkstra_engine("async")
    out = ctx.plan_dijkstra(int(W.seeds_a[3]), int(W.targets_a[3]), OFFSET)
    ctx.set_dijkstra_engine("tile_batch")
    assert out.code == 0


def cvp_call(ctx, W):
    m, om = W.case.mesh, W.case.om
    pos = (m.xyz[W.seeds_b[:2]] + np.array([0.02, 0.03, 0.0], np.float32)).astype(np.float32)
    sf = np.array([om.containing_face(p)[0] for p in pos], np.uint32)
    tf = np.array([om.containing_face((m.xyz[t] + np.array([0.02, 0.03, 0.0], np.float32)).astype(np.float32))[0] for t in W.targets_b[:2]], np.uint32)
    assert (sf < m.F).all() and (tf < m.F).all()
    c = ctx.plan_cvp_batch(pos, sf, tf, OFFSET)
    assert list(c["codes"]) == [0, 0]


def repairing_replan(ctx, W):
    ctx.set_option("replan_fresh_below", 0)
    a = ctx.replan_dijkstra(W.targets_a2, OFFSET)
    assert a["rc"] == 0 and a["replan"]["reason"] == 0, a["replan"]


def per_plan_replan(ctx, W):
    ctx.set_option("replan_fresh_below", 0)
    ctx.set_option("replan_each_fresh_share", 1)
    a = ctx.replan_dijkstra_each(W.targets_a2, OFFSET)
    assert a["rc"] == 0 and a["each"]["reason"] == 0, a["each"]


def inflation_wave(ctx, W):
    lethal = np.zeros(W.case.mesh.V, np.uint8)
    lethal[W.case.mesh.vertex_at(0.5, 0.5)] = 1
    ctx.layer_upload(0, W.case.costs, lethal)
    ctx.layer_inflation(1, 0)                                            # the wave works in plan slot 0


def paths_only_batch(ctx, W):
    ctx.set_resident_outputs(False)
    out = batch(ctx, W.seeds_a, W.targets_a)
    assert not ctx.device_output(0, 0)                                   # nothing V-sized was written
    ctx.set_resident_outputs(True)
    assert all(np.array_equal(out["paths"][k], W.ref_a[k][0].path) for k in range(N))


def cancelled_call(ctx, W):
    """mnav_cancel while a batch runs: the host looks at the flag between two chunks of iterations, so the batch is given a
    narrow band (more iterations than one chunk holds) and the flag is set over and over from a second thread"""
    ctx.set_option("tb_band_mult", 0.125)
    stop = threading.Event()

    def keep_cancelling():
        while not stop.is_set():
            ctx.cancel()
            time.sleep(0.0002)

    th = threading.Thread(target=keep_cancelling)
    th.start()
    try:
        out = ctx.plan_dijkstra_batch(W.seeds_a, W.targets_a, OFFSET)
    finally:
        stop.set()
        th.join(timeout=60)
    ctx.set_option("tb_band_mult", None)
    assert out["rc"] == capi.CANCELED and (out["codes"] == capi.CANCELED).all(), out["rc"]


def vector_maps_off(ctx, W):
    ctx.set_resident_outputs(False)
    out = batch(ctx, W.seeds_a, W.targets_a, fields=True)                # finalized, without vector maps
    ctx.set_resident_outputs(True)
    assert np.array_equal(out["dist"][5].view(np.uint32), W.ref_a[5][0].dist.view(np.uint32))


def new_mesh(ctx, W):
    W.case.upload(ctx)


def smaller_then_larger(ctx, W):
    batch(ctx, W.seeds_a[:70], W.targets_a[:70])
    s = ctx.tb_finalize_stats()
    assert not s["filled_at_start"], s                                   # fewer plans than were left clean
    big_s = np.concatenate([W.seeds_a, W.seeds_b[:70]])
    big_t = np.concatenate([W.targets_a, W.targets_b[:70]])
    batch(ctx, big_s, big_t)                                             # 200 plans: new buffers, nothing to keep
    s = ctx.tb_finalize_stats()
    assert s["skipped_pairs"] == 0 and s["filled_at_start"], s


# what happens between A and B, and whether the claim had to fall (then B may skip nothing); None: it may stand
BETWEEN = [
    ("a single plan on the asynchronous engine", single_async_plan, True),
    ("a CVP call", cvp_call, True),
    ("a replan that repairs", repairing_replan, True),
    ("a per-plan replan", per_plan_replan, True),
    ("an inflation layer", inflation_wave, True),
    ("a paths-only batch", paths_only_batch, True),
    ("a cancelled call", cancelled_call, True),
    ("a smaller batch and then a larger one", smaller_then_larger, None),
    ("vector maps off and on again", vector_maps_off, True),
    ("a new mesh", new_mesh, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [None, 3], ids=["default", "with_reset"])
@pytest.mark.parametrize("what,between,falls", BETWEEN, ids=[b[0].replace(" ", "_") for b in BETWEEN])
def test_something_else_between_the_two_batches(what, between, falls, keep):
    W = world()
    want = fresh_b()
    with W.context(keep=keep) as ctx:
        batch(ctx, W.seeds_a, W.targets_a)
        between(ctx, W)
        b = batch(ctx, W.seeds_b, W.targets_b)
        s = ctx.tb_finalize_stats()
        print(what, s)
        assert_same_fields(fields(ctx), want["fields"], what)
        assert_same_paths(b, want["out"], what)
        if falls:
            assert s["skipped_pairs"] == 0, (what, s)
        assert (s["reset_pairs"] > 0) == (keep == 3), (what, s)


@pytest.mark.gpu
def test_a_paths_only_batch_after_a_finalized_one_finds_clean_distances():
    W = world()
    with W.context(resident=False) as F:                                 # the fresh context: the paths-only batch alone
        want = batch(F, W.seeds_b, W.targets_b)
        want_popped = np.stack([F.download_output("popped", k) for k in range(N)])
    with W.context(keep=3) as ctx:
        batch(ctx, W.seeds_a, W.targets_a)
        assert ctx.tb_finalize_stats()["reset_pairs"] > 0
        ctx.set_resident_outputs(False)
        got = batch(ctx, W.seeds_b, W.targets_b)
        s = ctx.tb_finalize_stats()
        assert not s["filled_at_start"] and s["reset_pairs"] == 0 and s["skipped_pairs"] == 0, s   # it ran on what the pass left
        assert not ctx.device_output(0, 0)
        assert_same_paths(got, want, "paths-only after finalized")
        popped = np.stack([ctx.download_output("popped", k) for k in range(N)])
        assert np.array_equal(popped.view(np.uint32), want_popped.view(np.uint32))
        for k in (0, 64, 129):                                           # and the oracle: exact up to goal_dist, +inf beyond
            r = W.ref_b[k][0]
            cut = np.float32(np.float64(r.dist[W.targets_b[k]]) + OFFSET)
            assert np.array_equal(popped[k].view(np.uint32), np.where(r.dist <= cut, r.dist, np.float32(np.inf)).view(np.uint32)), k


@pytest.mark.gpu
def test_a_warm_repair_after_a_finalized_batch_and_a_fresh_batch_after_it():
    W = world()
    with W.context() as F:                                               # the fresh context: the plans towards the new robot vertices
        want_out = batch(F, W.seeds_a, W.targets_a2)
        want = fields(F)
    with W.context(keep=3) as ctx:
        ctx.set_option("replan_fresh_below", 0)
        ctx.set_option("replan_repair_engine", 5)
        batch(ctx, W.seeds_a, W.targets_a)
        a = ctx.replan_dijkstra(W.targets_a2, OFFSET)
        assert a["rc"] == 0 and a["replan"]["reason"] == 0 and a["warm"]["plans"] == N, (a["replan"], a["warm"], ctx.last_engine())
        assert_same_fields(fields(ctx), want, "warm repair")
        assert_same_paths(a, want_out, "warm repair")
        # the repair's finalize pass left the distances clean as well, and no claim: the next fresh batch fills nothing, skips nothing
        b = batch(ctx, W.seeds_b, W.targets_b)
        s = ctx.tb_finalize_stats()
        assert not s["filled_at_start"] and s["skipped_pairs"] == 0, s
        assert_same_fields(fields(ctx), fresh_b()["fields"], "fresh after warm")
        assert_same_paths(b, fresh_b()["out"], "fresh after warm")
