"""The resident layer graph (mnav_map_*, include/mnav.h): LayerManager + MeshMap::layerChanged on the
device.  Every comparison is bit for bit against tests/map_model.py, which recomputes the whole graph after every update
from the oracle's layers; tests/test_map_model.py pins that model to the reference's own incremental chain.

Sizes: the change-list passes work in blocks of 1024 vertices and scan 256 blocks per turn -- 33 x 31 (1 023: under one
block), 32 x 33 (1 056: a ragged second block), 513 x 513 (263 169: 258 blocks, a second turn of the scan), 96 x 96."""
import functools

import numpy as np
import pytest

from tests import map_model as M
from tests import obstacle_model as OM
from tests.common import Case
from tests.map_model import bits

pytestmark = pytest.mark.gpu

SIZES = [(33, 31), (32, 33), (513, 513), (96, 96)]


@functools.lru_cache(maxsize=None)
def grid_case(nx, ny):
    return Case(M.rect_terrain(nx, ny))


def start(ctx, case, name, nx, ny, mode="avg", factor=1.0, invalid=None):
    """graph `name` with the scenario's inputs on the device and in the model, both computed"""
    nodes, default, slots = M.graph(name, mode)
    sc = M.scenario_for(name, nx, ny)
    model = M.MapModel(case.om, case.edge_dist, nodes, default, factor, invalid)
    m = case.mesh
    ctx.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
    for slot, (c, le) in zip(slots, sc.inputs):
        ctx.layer_upload(slot, c, le)
        model.set_input(slot, c, le)
    ctx.map_configure(nodes, default, factor, invalid)
    ctx.map_compute()
    model.compute()
    return model, sc, slots


def same_state(ctx, model, where):
    """every layer slot, the inflation distances and vector fields, the resident vertex costs and edge weights"""
    for slot in model.order:
        infl = model.nodes[slot]["kind"] == "inflation"
        got = ctx.layer_download(slot, distances=infl)
        assert np.array_equal(bits(got[0]), bits(model.cost[slot])), (where, slot, int((bits(got[0]) != bits(model.cost[slot])).sum()))
        assert np.array_equal(got[1] != 0, model.lethal[slot] != 0), (where, slot)
        if infl:
            assert np.array_equal(bits(got[2]), bits(model.dist[slot])), (where, slot)
            dv, has = ctx.layer_vectors(slot)
            vec = model.vec[slot]
            same = (bits(dv).reshape(-1, 3) == bits(vec).reshape(-1, 3)).all(axis=1) | (np.isnan(dv).any(axis=1) & np.isnan(vec).any(axis=1))
            same |= (has == 0) & (vec == 0).all(axis=1)                # no entry in the reference's map
            assert same.all(), (where, slot, int((~same).sum()))
    vc, w = ctx.download_costs()
    assert np.array_equal(bits(vc), bits(model.vertex_costs)), where
    assert np.array_equal(bits(w), bits(model.edge_weights)), where


PARITY = [(name, nx, ny, "avg", 1.0) for nx, ny in SIZES for name in "abc"] + [("b", 96, 96, "max", 0.0), ("b", 32, 33, "max", 1.0)]


@pytest.mark.parametrize("name,nx,ny,mode,factor", PARITY)
def test_state_parity_over_an_update_sequence(gpu_ctx_factory, name, nx, ny, mode, factor):
    """After map_compute and after each update -- lethals added, lethals removed, a cost-only change, the same update again
    (nothing changes), duplicate ids -- every layer, the wave state, the vertex costs, the edge weights and changed_out are
    the model's.  The state-changing updates change some but not all vertices (0 < n_changed < V) and the first two flip
    lethal flags; tests/test_map_model.py shows the model alone satisfies that.  Graph (a)'s default layer is the
    inflation of `costs`, a function of its lethal set only: a cost-only change cannot reach it, so there n_changed is 0."""
    case = grid_case(nx, ny)
    V = case.mesh.V
    ctx = gpu_ctx_factory()
    model, sc, slots = start(ctx, case, name, nx, ny, mode, factor)
    same_state(ctx, model, "compute")
    for tag, k, ids, costs, lethal in sc.updates:
        flags_before = ctx.layer_download(slots[k])[1]
        D = model.update_layer(slots[k], ids, costs, lethal)
        out = ctx.map_update_layer(slots[k], ids, costs, lethal)
        n_changed, st = out["changed"].size, out["stats"]
        print(name, nx, ny, tag, "n_changed", n_changed, "stats", st)
        assert np.array_equal(out["changed"], D), (tag, n_changed, D.size)
        same_state(ctx, model, tag)
        assert st["waves"] == model.waves and st["default_changed"] == n_changed
        flipped = int((flags_before != ctx.layer_download(slots[k])[1]).sum())
        if tag in ("add", "remove"):
            assert 0 < n_changed < V and flipped > 0 and st["waves"] == 1
        elif tag == "cost":
            assert st["waves"] == 0 and flipped == 0
            assert n_changed == 0 if name == "a" else 0 < n_changed < V
        elif tag == "nothing":
            assert n_changed == 0 and st["waves"] == 0
        if factor == 0.0:
            assert st["edges_reweighted"] == 0
    ctx.close()


def test_invalid_vertices_reach_the_waves_and_the_planner_tables(gpu_ctx_factory):
    """the map's non-manifold flags given at configure: the inflation waves of compute and of an update never fix them"""
    nx = ny = 96
    case = grid_case(nx, ny)
    invalid = np.zeros(case.mesh.V, np.uint8)
    invalid[np.random.default_rng(1).choice(case.mesh.V, case.mesh.V // 40, replace=False)] = 1
    ctx = gpu_ctx_factory()
    model, sc, slots = start(ctx, case, "b", nx, ny, "avg", 1.0, invalid)
    same_state(ctx, model, "compute")
    tag, k, ids, costs, lethal = sc.updates[0]
    D = model.update_layer(slots[k], ids, costs, lethal)
    assert np.array_equal(ctx.map_update_layer(slots[k], ids, costs, lethal)["changed"], D)
    same_state(ctx, model, tag)
    ctx.close()


def hovering_cloud(mesh, lo, hi, n=60):
    """n x n points one unit above the terrain over the square [lo, hi]^2 (grid units of 0.1)"""
    g = np.linspace(lo * 0.1, hi * 0.1, n, dtype=np.float32)
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, 1.5, np.float32)], axis=1).astype(np.float32)


def test_map_obstacle_is_the_obstacle_pass_plus_the_chain(gpu_ctx_factory):
    """A cloud hovering over a patch, down_axis (0, 0, -1): mnav_map_obstacle leaves the state of a second context that ran
    mnav_layer_obstacle and handed the returned ids to mnav_map_layer_changed, and the state of the model fed with the
    obstacle layer's downloaded costs and flags.  The second, shifted frame clears and sets vertices in one call."""
    nx = ny = 96
    case = grid_case(nx, ny)
    m = case.mesh
    nodes, default, slots = M.graph("b", "avg")
    second = M.scenario_for("b", nx, ny).inputs[1]
    model = M.MapModel(case.om, case.edge_dist, nodes, default, 1.0)
    ctxs = [gpu_ctx_factory(), gpu_ctx_factory()]
    empty = np.zeros((0, 3), np.float32)
    for ctx in ctxs:
        ctx.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
        ctx.layer_obstacle(0, empty)                                 # an empty cloud: the obstacle layer, cleared
        ctx.layer_upload(2, *second)
        ctx.map_configure(nodes, default, 1.0)
        ctx.map_compute()
    model.set_input(0, np.zeros(m.V, np.float32), np.zeros(m.V, np.uint8))
    model.set_input(2, *second)
    model.compute()
    same_state(ctxs[0], model, "compute")
    old = np.zeros(m.V, np.uint8)
    for frame, (lo, hi) in enumerate(((30, 40), (36, 46))):
        pts = hovering_cloud(m, lo, hi)
        a = ctxs[0].map_obstacle(0, pts, down_axis=(0.0, 0.0, -1.0))
        b0 = ctxs[1].layer_obstacle(0, pts, down_axis=(0.0, 0.0, -1.0))
        b = ctxs[1].map_layer_changed(0, b0["changed"])
        want = OM.obstacle_layer(m.xyz, m.faces, pts, old_lethal=old)
        assert np.array_equal(b0["changed"], want["changed"])
        c, le = ctxs[0].layer_download(0)
        assert np.array_equal(le, want["lethal"]) and np.array_equal(bits(c), bits(want["cost"]))
        D = model.replace_layer(0, c, le, b0["changed"])
        assert np.array_equal(a["changed"], D) and np.array_equal(b["changed"], D) and 0 < D.size < m.V
        same_state(ctxs[0], model, frame)
        same_state(ctxs[1], model, frame)
        assert a["stats"]["waves"] == 1 and b["stats"]["waves"] == 1
        gone, came = old & ~want["lethal"] & 1, want["lethal"] & ~old & 1
        assert came.sum() > 0 and (frame == 0 or gone.sum() > 0)    # the shifted frame clears and sets in one call
        old = want["lethal"]
    for ctx in ctxs:
        ctx.close()


def test_planners_see_an_update(gpu_ctx_factory):
    """plan_dijkstra and plan_cvp after an update == a fresh context that got the final costs and weights through
    mnav_upload_costs, with a seed / target on a vertex the update made lethal and on one it freed: the host's cost mirror
    (seed cut-offs) and the cost-limit folded tables (built by a plan before the update) follow."""
    nx = ny = 96
    case = grid_case(nx, ny)
    m = case.mesh
    ctx = gpu_ctx_factory()
    model, sc, slots = start(ctx, case, "b", nx, ny, "avg", 1.0)
    far = 5 * nx + 5

    def face_of(v):                                                  # a face with v as a corner (v is the v00 of its cell)
        return 2 * ((v // nx) * (nx - 1) + v % nx)

    freed = int(sc.updates[1][2][-1])                                # a wall vertex the second update frees
    made = int(sc.updates[0][2][-1])                                 # a patch vertex the first update makes lethal and the second keeps
    ctx.plan_dijkstra(far, freed)                                    # builds the folded tables on the old costs
    ctx.plan_cvp(m.xyz[far], face_of(far), face_of(freed))
    for tag, k, ids, costs, lethal in sc.updates[:2]:
        model.update_layer(slots[k], ids, costs, lethal)
        ctx.map_update_layer(slots[k], ids, costs, lethal)
    assert model.lethal[model.default_layer][made] == 1 and model.lethal[model.default_layer][freed] == 0
    assert model.vertex_costs[made] >= 1.0 > model.vertex_costs[freed]
    fresh = gpu_ctx_factory()
    fresh.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
    fresh.upload_costs(model.vertex_costs, model.edge_weights)
    for s, t in ((far, freed), (freed, far), (far, made), (made, far)):
        a, b = ctx.plan_dijkstra(s, t), fresh.plan_dijkstra(s, t)
        assert a.code == b.code, (s, t, a.code, b.code)
        assert np.array_equal(bits(a.dist), bits(b.dist)) and np.array_equal(a.pred, b.pred) and np.array_equal(a.path, b.path), (s, t)
        a, b = ctx.plan_cvp(m.xyz[s], face_of(s), face_of(t)), fresh.plan_cvp(m.xyz[s], face_of(s), face_of(t))
        assert a.code == b.code, (s, t, a.code, b.code)
        assert np.array_equal(bits(a.dist), bits(b.dist)) and np.array_equal(a.pred, b.pred), (s, t)
        assert np.array_equal(bits(a.direction), bits(b.direction)) and np.array_equal(a.cutface, b.cutface), (s, t)
    assert ctx.plan_dijkstra(far, freed).code == 0                   # the freed vertex can be reached
    ctx.close()
    fresh.close()


REFUSED = [
    ([dict(layer=64, kind="input")], 64, "slot out of range"),
    ([dict(layer=1, kind="input"), dict(layer=1, kind="input")], 1, "listed twice"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="max", inputs=[0, 5])], 1, "not a node"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="inflation", inputs=[0, 0])], 1, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="avg")], 1, "number of inputs"),
    ([dict(layer=0, kind="input", inputs=[0])], 0, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="max", inputs=[0, 2]), dict(layer=2, kind="inflation", inputs=[1])], 1, "cycle"),
    ([dict(layer=0, kind="input")], 3, "default layer is not a node"),
]


def test_errors(gpu_ctx_factory):
    nx, ny = 32, 33
    case = grid_case(nx, ny)
    m = case.mesh
    ctx = gpu_ctx_factory()
    nodes, default, slots = M.graph("b", "avg")
    ctx.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
    ids, vals = np.array([3], np.uint32), np.array([0.5], np.float32)
    # before configure / compute
    with pytest.raises(RuntimeError, match="mnav_map_configure first"):
        ctx.map_compute()
    with pytest.raises(RuntimeError, match="mnav_map_configure first"):
        ctx.map_update_layer(0, ids, vals)
    ctx.map_configure(nodes, default, 1.0)
    with pytest.raises(RuntimeError, match="input layer is not resident"):
        ctx.map_compute()
    with pytest.raises(RuntimeError, match="mnav_map_compute first"):
        ctx.map_update_layer(0, ids, vals)
    with pytest.raises(RuntimeError, match="mnav_map_compute first"):
        ctx.map_layer_changed(0, ids)
    with pytest.raises(RuntimeError, match="mnav_map_compute first"):
        ctx.map_obstacle(0, np.zeros((0, 3), np.float32))
    ctx.close()
    # a working configuration survives every refused one
    ctx = gpu_ctx_factory()
    model, sc, slots = start(ctx, case, "b", nx, ny)
    for bad, d, what in REFUSED:
        with pytest.raises(RuntimeError, match=what):
            ctx.map_configure(bad, d, 1.0)
        with pytest.raises(ValueError):
            M.dependency_order(bad, d)
    tag, k, ids, costs, lethal = sc.updates[0]
    D = model.update_layer(slots[k], ids, costs, lethal)
    assert np.array_equal(ctx.map_update_layer(slots[k], ids, costs, lethal)["changed"], D)
    same_state(ctx, model, "after the refused configurations")
    # an id >= V: nothing is written
    with pytest.raises(RuntimeError, match="out of range"):
        ctx.map_update_layer(0, np.array([5, m.V], np.uint32), np.array([9.0, 9.0], np.float32), np.array([1, 1], np.uint8))
    with pytest.raises(RuntimeError, match="out of range"):
        ctx.map_layer_changed(0, np.array([m.V + 7], np.uint32))
    same_state(ctx, model, "after an id out of range")
    # derived nodes are the graph's
    for call in (lambda: ctx.map_update_layer(1, ids, costs, lethal), lambda: ctx.map_update_layer(3, ids, costs),
                 lambda: ctx.map_layer_changed(3, ids), lambda: ctx.map_obstacle(1, np.zeros((0, 3), np.float32))):
        with pytest.raises(RuntimeError, match="derived node"):
            call()
    with pytest.raises(RuntimeError, match="not a node"):
        ctx.map_update_layer(7, ids, costs)
    with pytest.raises(RuntimeError, match="down_axis must be finite and non-zero"):   # an argument error of the obstacle pass
        ctx.map_obstacle(0, np.zeros((4, 3), np.float32), down_axis=(0.0, 0.0, 0.0))
    same_state(ctx, model, "after the refused updates")
    tag, k, ids, costs, lethal = sc.updates[1]                       # ... and the graph is not stale
    D = model.update_layer(slots[k], ids, costs, lethal)
    assert np.array_equal(ctx.map_update_layer(slots[k], ids, costs, lethal)["changed"], D)
    same_state(ctx, model, "an update after the refused ones")
    # a new mesh drops the graph
    ctx.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
    with pytest.raises(RuntimeError, match="mnav_map_configure first"):
        ctx.map_compute()
    with pytest.raises(RuntimeError, match="mnav_map_configure first"):
        ctx.map_update_layer(0, ids, costs)
    ctx.close()
