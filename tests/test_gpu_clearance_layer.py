"""The clearance and border layers on the device (mnav_layer_clearance, mnav_layer_border; ClearanceLayer,
clearance_layer.cpp:67-99 / :122-164, BorderLayer, border_layer.cpp:66-80 / :104-110).  Every comparison is exact
against tests/clearance_model.py: raw clearance, costs, lethal flags and the change list."""
import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import clearance_model as M
from tests import nbhd_model
from tests import obstacle_model as OM
from tests.common import Case
from tests.clearance_model import up, with_ceiling

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_layer(ctx, layer, got, want):
    c, le = ctx.layer_download(layer)
    assert np.array_equal(bits(c), bits(want["cost"])), int((bits(c) != bits(want["cost"])).sum())
    assert np.array_equal(le, want["lethal"])
    assert np.array_equal(got["changed"], want["changed"])
    assert got["n_lethal"] == int(want["lethal"].sum())


def clearance_case(ctx, mesh, nrm, layer=0, rh=0.5, hi=0.3, old=None, verts=None):
    """one clearance call against the model (all vertices, or raw clearance on `verts` only); returns the model's layer"""
    got = ctx.layer_clearance(layer, rh, hi)
    c = ctx.clearance()
    if verts is None:
        want_c = M.clearance(mesh.xyz, mesh.faces, nrm)
        assert np.array_equal(bits(c), bits(want_c)), int((bits(c) != bits(want_c)).sum())
    else:
        want_c = M.clearance(mesh.xyz, mesh.faces, nrm, verts)
        assert np.array_equal(bits(c[verts]), bits(want_c))
    want = M.clearance_layer(c, rh, hi, *(old or (None, None)))
    check_layer(ctx, layer, got, want)
    return c, want


@pytest.mark.parametrize("tilt", [False, True])
def test_flat_grid_never_hits_its_own_fan(gpu_ctx_factory, tilt):
    g = meshgen.flat_grid(48, 0.1)
    xyz, nrm = g.xyz, up(g.V)
    if tilt:
        a, b = 0.05, -0.03
        R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]) @ \
            np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        xyz = (g.xyz.astype(np.float64) @ R.T).astype(np.float32)
        nrm = np.tile((R @ np.array([0.0, 0.0, 1.0])).astype(np.float32), (g.V, 1))
    mesh = meshgen.from_faces(xyz, g.faces)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    c, want = clearance_case(ctx, mesh, nrm)
    assert np.isinf(c).all() and (want["cost"] == 0).all()          # a self-hit would show as c == 0
    st = ctx.clearance_stats()
    assert st["cast"] == 1 and st["rays"] == g.V and st["hits"] == 0 and st["ms_bvh_build"] > 0


def test_terrain_48_every_vertex(gpu_ctx_factory):
    mesh = meshgen.terrain(48, 0.1, 4, amplitude=3.0, base_freq=0.25)   # steep valleys: many rays hit the opposite slope
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    nrm[::41] = 0.0
    nrm[5] = np.nan
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    c, want = clearance_case(ctx, mesh, nrm, rh=0.2, hi=0.3)
    st = ctx.clearance_stats()
    assert st["hits"] == int(np.isfinite(c).sum()) > 0 and st["rays"] == mesh.V - len(range(0, mesh.V, 41)) - 1
    assert want["lethal"].sum() > 0 and ((want["cost"] > 0) & (want["cost"] < 1)).any()


def test_two_sheets_and_a_holed_ceiling(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    sheets = nbhd_model.two_sheets(24, 0.1, 0.2)
    nrm = M.vertex_normals(sheets.xyz, sheets.faces)
    ctx.upload_mesh(sheets.xyz, sheets.faces, sheets.edges, nrm)
    c, _ = clearance_case(ctx, sheets, nrm, rh=0.15, hi=0.1)
    assert np.isfinite(c).sum() > 24 * 24
    ground = meshgen.terrain(40, 0.1, 9, amplitude=0.4)
    mesh = with_ceiling(ground, 0.6, step=2, drop=0.25, seed=3)
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    c, want = clearance_case(ctx, mesh, nrm, layer=3)
    hit_ground = np.isfinite(c[:ground.V])
    assert 0.3 * ground.V < hit_ground.sum() < ground.V                # the holes let some rays through


def test_c2_mesh_under_a_ceiling(gpu_ctx_factory):
    ground = meshgen.terrain(1000, 0.1, 2)
    n = 250                                                           # ceiling over half the area, spacing 0.2, at z = 1.0
    g = meshgen.flat_grid(n, 0.2)
    top = g.xyz.copy()
    top[:, 0] *= 0.5                                                  # 0 .. 24.9 in x, 0 .. 49.8 in y
    top[:, 2] = 1.0
    xyz = np.concatenate([ground.xyz, top]).astype(np.float32)
    faces = np.concatenate([ground.faces, g.faces[:, ::-1] + ground.V]).astype(np.uint32)
    mesh = meshgen.from_faces(xyz, faces)
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    got = ctx.layer_clearance(0, 0.5, 0.3)
    c = ctx.clearance()
    cost, le = ctx.layer_download(0)
    # the whole array: no NaN, t >= 0, and the cost pass of the model over every vertex
    assert not np.isnan(c).any() and (c >= 0).all()
    want = M.clearance_layer(c, 0.5, 0.3)
    assert np.array_equal(bits(cost), bits(want["cost"])) and np.array_equal(le, want["lethal"])
    assert got["changed"].size == mesh.V and got["n_lethal"] == int(want["lethal"].sum())
    assert np.isfinite(c[ground.V:]).sum() > 0.9 * g.V                # the ceiling's normals point down, at the ground
    assert got["stats"]["rays"] == mesh.V and got["stats"]["hits"] == int(np.isfinite(c).sum())
    # a sample against the brute-force model: lethal, in the band, free under the ceiling, open sky, the ceiling
    rng = np.random.default_rng(0)
    covered = np.nonzero(np.isfinite(c[:ground.V]))[0]
    groups = [np.nonzero(want["lethal"])[0], np.nonzero((want["cost"] > 0) & (want["cost"] < 1))[0],
              covered[want["cost"][covered] == 0], np.nonzero(np.isinf(c[:ground.V]))[0], np.arange(ground.V, mesh.V)]
    sample = np.concatenate([rng.choice(x, min(16, x.size), replace=False) for x in groups if x.size])
    assert sample.size >= 64
    fc = M.Faces(mesh.xyz, mesh.faces)
    want_c, _ = M.clearance_of(mesh.xyz, mesh.faces, nrm, sample, fc)
    assert np.array_equal(bits(c[sample]), bits(want_c))


def test_reconfigure_reuses_the_cache(gpu_ctx_factory):
    ground = meshgen.terrain(40, 0.1, 5, amplitude=0.6)
    mesh = with_ceiling(ground, 0.55, step=1)
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    c, a = clearance_case(ctx, mesh, nrm, layer=2, rh=0.5, hi=0.3)
    assert ctx.clearance_stats()["cast"] == 1
    for rh, hi in ((0.4, 0.5), (0.4, 0.5), (0.6, 0.0)):
        got = ctx.layer_clearance(2, rh, hi)
        st = got["stats"]
        assert st["cast"] == 0 and st["rays"] == 0 and st["ms_bvh_build"] == 0 and st["ms_cast"] == 0
        want = M.clearance_layer(c, rh, hi, a["cost"], a["lethal"])
        check_layer(ctx, 2, got, want)
        a = want
    assert got["changed"].size > 0
    assert np.array_equal(bits(ctx.clearance()), bits(c))


def test_chain_clearance_inflation_combination_plan(gpu_ctx_factory):
    ground = meshgen.terrain(96, 0.1, 6, amplitude=0.6)
    mesh = with_ceiling(ground, 0.9, step=2, drop=0.3, seed=2)
    case = Case(mesh)
    m = case.mesh
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(m.xyz, m.faces, m.edges, case.vn)
    ctx.layer_clearance(0, 0.5, 0.3)
    c = ctx.clearance()
    ctx.layer_steepness(2, 0.6)
    steep_d, _ = ctx.layer_download(2)
    want_vc = None
    old_infl = None
    for rh, hi in ((0.5, 0.3), (0.7, 0.2)):
        got = ctx.layer_clearance(0, rh, hi)
        clr = M.clearance_layer(c, rh, hi)
        ctx.layer_inflation(1, 0)
        infl_d, _, dist_d = ctx.layer_download(1, distances=True)
        infl, dist, _ = case.om.inflation(clr["lethal"], case.edge_dist)
        assert np.array_equal(bits(dist_d), bits(dist)) and np.array_equal(bits(infl_d), bits(infl))
        want_vc = O.combine([clr["cost"], infl, steep_d], [1.0, 1.0, 1.0], "max")
        if old_infl is None:
            ctx.combine_layers([0, 1, 2], [1.0, 1.0, 1.0], mode="max", edge_cost_factor=1.0)
        else:
            ids = np.union1d(got["changed"], np.nonzero(bits(infl) != bits(old_infl))[0]).astype(np.uint32)
            assert 0 < got["changed"].size and ids.size < m.V
            ctx.combine_layers_update([0, 1, 2], ids, [1.0, 1.0, 1.0], mode="max")
        old_infl = infl
        vc, w = ctx.download_costs()
        want_w = case.om.edge_weights(case.edge_dist, want_vc, 1.0)
        assert np.array_equal(bits(vc), bits(want_vc)) and np.array_equal(bits(w), bits(want_w))
        free = np.nonzero(want_vc[:ground.V] < 0.5)[0]
        s, t = int(free[len(free) // 5]), int(free[-len(free) // 6])
        ref = case.om.dijkstra(want_w, want_vc, s, t)
        out = ctx.plan_dijkstra(s, t)
        assert out.code == ref.code and np.array_equal(bits(out.dist), bits(ref.dist)) and np.array_equal(out.pred, ref.pred)


def test_shared_bvh_with_the_obstacle_layer(gpu_ctx_factory):
    ground = meshgen.terrain(64, 0.1, 7, amplitude=0.5)
    mesh = with_ceiling(ground, 0.8, step=2, drop=0.2, seed=4)
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(0, 6.3, (3000, 2)), rng.uniform(1.0, 2.0, (3000, 1))], 1).astype(np.float32)

    def fresh():
        ctx = gpu_ctx_factory()
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
        return ctx

    a, b, c, d = fresh(), fresh(), fresh(), fresh()
    a.layer_clearance(0)
    a.layer_obstacle(1, pts, robot_height=1.5)
    assert a.obstacle_stats()["ms_bvh_build"] == a.clearance_stats()["ms_bvh_build"] > 0   # built by the clearance call
    b.layer_obstacle(1, pts, robot_height=1.5)
    b.layer_clearance(0)
    assert b.clearance_stats()["ms_bvh_build"] == 0 and b.clearance_stats()["cast"] == 1
    c.layer_clearance(0)
    d.layer_obstacle(1, pts, robot_height=1.5)
    want_obs = OM.obstacle_layer(mesh.xyz, mesh.faces, pts, robot_height=1.5)
    for ctx in (a, b, c):
        assert np.array_equal(bits(ctx.clearance()), bits(c.clearance()))
        assert all(np.array_equal(x, y) for x, y in zip(ctx.layer_download(0), c.layer_download(0)))
    for ctx in (a, b, d):
        cost, le = ctx.layer_download(1)
        assert np.array_equal(le, want_obs["lethal"]) and np.array_equal(bits(cost), bits(want_obs["cost"]))


def test_reupload_gives_the_first_round_again(gpu_ctx_factory):
    A = with_ceiling(meshgen.terrain(40, 0.1, 1, amplitude=0.5), 0.7, step=2, drop=0.2)
    B = meshgen.punched(32, 0.1, 2)
    na, nb = M.vertex_normals(A.xyz, A.faces), M.vertex_normals(B.xyz, B.faces)
    ctx = gpu_ctx_factory()

    def round_(mesh, nrm):
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
        c_got = ctx.layer_clearance(0)
        b_got = ctx.layer_border(1)
        assert c_got["stats"]["cast"] == 1 and c_got["changed"].size == mesh.V and b_got["changed"].size == mesh.V
        return ctx.clearance(), ctx.layer_download(0), ctx.layer_download(1), ctx.device_bytes()

    first = round_(A, na)
    round_(B, nb)
    again = round_(A, na)
    assert np.array_equal(bits(first[0]), bits(again[0]))
    for x, y in zip(first[1] + first[2], again[1] + again[2]):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    assert first[3] == again[3]
    want = M.border_layer(A.V, A.edges, A.faces)
    assert np.array_equal(again[2][1], want["lethal"]) and np.array_equal(bits(again[2][0]), bits(want["cost"]))


@pytest.mark.parametrize("kind", ["triangle", "grid", "punched", "sheets"])
def test_border_layer(gpu_ctx_factory, kind):
    if kind == "triangle":
        mesh = meshgen.from_faces(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    elif kind == "grid":
        mesh = meshgen.flat_grid(33, 0.1)
    elif kind == "punched":
        mesh = meshgen.punched(96, 0.1, 5, drop=0.1, cut_column=40)
    else:
        mesh = nbhd_model.two_sheets(24, 0.1, 0.2)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)            # no normals needed
    want = M.border_layer(mesh.V, mesh.edges, mesh.faces)
    got = ctx.layer_border(4)
    check_layer(ctx, 4, got, want)
    assert 0 < want["border"].sum() and (want["border"].all() == (kind == "triangle"))
    # another border_cost keeps every flag but changes the border vertices' cost bits: they are the change list
    nxt = M.border_layer(mesh.V, mesh.edges, mesh.faces, 0.75, 0.5, want["cost"], want["lethal"])
    got = ctx.layer_border(4, 0.75, 0.5)
    check_layer(ctx, 4, got, nxt)
    assert np.array_equal(got["changed"], np.nonzero(want["border"])[0])
    nxt2 = M.border_layer(mesh.V, mesh.edges, mesh.faces, 0.75, -1.0, nxt["cost"], nxt["lethal"])   # every vertex lethal
    check_layer(ctx, 4, ctx.layer_border(4, 0.75, -1.0), nxt2)


def test_errors_leave_the_slot_untouched(gpu_ctx_factory):
    from mesh_navigation_amd import capi
    ctx = gpu_ctx_factory()
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        ctx.layer_clearance(0)
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        ctx.layer_border(0)
    mesh = meshgen.terrain(32, 0.1, 1)
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)
    rng = np.random.default_rng(0)
    cost0 = rng.uniform(0, 1, mesh.V).astype(np.float32)
    leth0 = (rng.uniform(size=mesh.V) < 0.1).astype(np.uint8)
    ctx.layer_upload(0, cost0, leth0)

    def untouched():
        c, le = ctx.layer_download(0)
        assert np.array_equal(bits(c), bits(cost0)) and np.array_equal(le, leth0)

    with pytest.raises(RuntimeError, match="normals"):
        ctx.layer_clearance(0)                                       # no resident normals
    untouched()
    with pytest.raises(RuntimeError, match="no clearance"):
        ctx.clearance()
    nrm = M.vertex_normals(mesh.xyz, mesh.faces)
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    ctx.layer_upload(0, cost0, leth0)
    for rh, hi in ((np.nan, 0.3), (np.inf, 0.3), (0.5, np.nan), (0.5, -np.inf), (-0.1, 0.3), (0.5, -1e-9)):
        with pytest.raises(RuntimeError, match="robot_height"):
            ctx.layer_clearance(0, rh, hi)
        untouched()
    for bc, th in ((np.nan, 0.5), (np.inf, 0.5), (-np.inf, 0.5), (1.0, np.nan)):
        with pytest.raises(RuntimeError, match="border_cost|threshold"):
            ctx.layer_border(0, bc, th)
        untouched()
    with pytest.raises(RuntimeError, match="layer index"):
        ctx.layer_clearance(64)
    assert ctx._L.mnav_clearance_download(ctx._h, None) < 0           # nothing cached yet: every failed call cast nothing
    # the argument checks come before the cast: the first valid call still casts, with NULL outputs
    assert ctx._L.mnav_layer_clearance(ctx._h, 5, 0.5, 0.3, None, None, None) == 0
    assert ctx.clearance_stats()["cast"] == 1
    ok = np.zeros(mesh.V, np.float32)
    assert ctx._L.mnav_clearance_download(ctx._h, capi._p(ok)) == 0 and np.array_equal(bits(ok), bits(ctx.clearance()))
