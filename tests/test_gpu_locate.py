"""The pose lookup on the device (mnav_locate, mnav_locate_stats, mnav_plan_dijkstra_batch_at, mnav_plan_cvp_batch_at)
against the oracle's nearest_vertex / containing_face: every query family of tests/locate_model.py, a million queries on
the C2 mesh, the plans from positions against the plans from oracle-resolved ids, re-uploads and errors.  Every comparison
is exact: ids equal, floats compared as bits."""
import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from oracle import oracle as O
from tests import locate_model as M
from tests.common import Case

pytestmark = pytest.mark.gpu


def upload(ctx, mesh, rows=None):
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None, face_circulation=rows)


@pytest.mark.parametrize("name", M.GRID_NAMES)
def test_every_family_equals_the_oracle(gpu_ctx_factory, name):
    mesh = M.grid_meshes()[name]()
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    ctx = gpu_ctx_factory()
    upload(ctx, mesh)
    for k, (fam, (pts, info)) in enumerate(M.families(mesh, 100 + M.GRID_NAMES.index(name)).items()):
        got = ctx.locate(pts)
        st = ctx.locate_stats()
        assert st["built"] == (1 if k == 0 else 0)
        M.assert_same(got, M.oracle_locate(om, pts), (name, fam))
        if fam == "surface":
            found = (got["face"] != M.NONE).mean()
            print(name, "surface queries with a face:", found, "candidates per query:", st["candidates"] / pts.shape[0])
            assert found >= 0.9
            assert st["candidates"] < pts.shape[0] * mesh.V / 4       # pruned, not a scan
        if fam == "midpoints":
            print(name, "exact ties:", M.check_midpoint_ties(mesh, pts, info, got["vertex"]))
        if fam == "vertices":
            assert (M.d2(pts, mesh.xyz[got["vertex"]]) == 0).all() and (got["vertex"] <= np.arange(mesh.V)).all()
        if fam == "far":
            assert (got["vertex"] != M.NONE).all()
            assert st["candidates"] < pts.shape[0] * mesh.V / 4       # a far query walks no rings of empty space
        if fam == "degenerate":
            assert (got["vertex"] == M.NONE).all() and (got["face"] == M.NONE).all()


def test_coincident_isolated_and_outlier_vertices(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    mesh, pairs = M.coincident_mesh()
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    upload(ctx, mesh)
    pts = np.concatenate([mesh.xyz, M.surface_points(mesh, 300, 5)[0]])
    got = ctx.locate(pts)
    M.assert_same(got, M.oracle_locate(om, pts), "coincident")
    for lo, hi in pairs:
        assert got["vertex"][lo] == lo and got["vertex"][hi] == lo

    mesh, iso = M.isolated_mesh()
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    upload(ctx, mesh)
    pts = np.stack([mesh.xyz[iso], mesh.xyz[iso] + np.float32(0.01), mesh.xyz[iso] - np.array([0, 0, 0.2], np.float32)]).astype(np.float32)
    got = ctx.locate(pts)
    M.assert_same(got, M.oracle_locate(om, pts), "isolated")
    assert (got["vertex"] == iso).all() and (got["face"] == M.NONE).all()

    mesh, v_far = M.outlier_mesh()
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    base = ctx.device_bytes()
    upload(ctx, mesh)
    pts = np.concatenate([M.surface_points(mesh, 500, 6)[0], M.far_points(mesh), mesh.xyz[v_far][None], np.array([[0.0, 0.3, 0.0]], np.float32)])
    before = ctx.device_bytes()
    got = ctx.locate(pts)
    M.assert_same(got, M.oracle_locate(om, pts), "outlier")
    assert got["vertex"][-2] == v_far and (got["vertex"] != v_far + 1).all()      # the NaN vertex is never a candidate
    assert ctx.locate_stats()["candidates"] < pts.shape[0] * mesh.V / 4
    # the index is O(V) whatever the box: 16 B per vertex + 64 B per 8 vertices, + the face rows of the search
    assert ctx.device_bytes() - before <= 24 * mesh.V + 256 + 4 * (6 * mesh.F + mesh.V + 1) + 3 * 64, (base, before, ctx.device_bytes())


def test_rotated_circulation_rows_decide_the_face_on_a_flat_mesh(gpu_ctx_factory):
    mesh = M.grid_meshes()["flat"]()
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    ptr, vf = om.vertex_faces()
    pts = np.concatenate([M.surface_points(mesh, 400, 9, sigma=0.0)[0], M.edge_midpoints(mesh, 200, 10)[0], mesh.xyz[::7]])
    ctx = gpu_ctx_factory()
    faces = []
    for by in (0, 1, 2):
        rows = (ptr, M.rotated_rows(ptr, vf, by))
        upload(ctx, mesh, rows)
        got = ctx.locate(pts)
        M.assert_same(got, M.oracle_locate(om, pts, rows), ("rows", by))
        faces.append(got["face"])
    assert (faces[0] != faces[1]).any() and (faces[1] != faces[2]).any()
    upload(ctx, mesh)                                                  # the library's own replay = the oracle's rows
    M.assert_same(ctx.locate(pts), M.oracle_locate(om, pts), "own rows")


def test_c2_million_queries(gpu_ctx_factory):
    mesh = meshgen.terrain(1000, 0.1, 2)
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    ctx = gpu_ctx_factory()
    upload(ctx, mesh)
    n = 1 << 20
    pts, gen = M.surface_points(mesh, n, 77)
    got = ctx.locate(pts)
    st = ctx.locate_stats()
    print("C2: build ms", st["ms_build"], "query ms", st["ms_query"], "candidates per query", st["candidates"] / n)
    assert st["built"] == 1
    assert st["candidates"] / n < mesh.V / 100                         # keeps a brute-force kernel from passing as the feature
    sample = np.random.default_rng(3).choice(n, 2000, replace=False)
    want = M.oracle_locate(om, pts[sample])
    M.assert_same({k: v[sample] for k, v in got.items()}, want, "C2 sample")
    # all queries: no corner of the generating face is a better (d, id) than the answer ...
    v = got["vertex"]
    assert (v < mesh.V).all()
    best = M.key(M.d2(pts, mesh.xyz[v]), v)
    for c in range(3):
        corner = mesh.faces[gen, c]
        assert (M.key(M.d2(pts, mesh.xyz[corner]), corner) >= best).all()
    # ... and a returned face has the answer as a corner and passes the inside test when recomputed
    f = got["face"]
    has = np.nonzero(f != M.NONE)[0]
    assert has.size >= 0.9 * n
    tri = mesh.faces[f[has]]
    assert (tri == v[has, None]).any(axis=1).all()
    inside, bary, dist = M.projected_barycentric_bulk(pts[has], mesh.xyz[tri[:, 0]], mesh.xyz[tri[:, 1]], mesh.xyz[tri[:, 2]])
    assert inside.all()
    assert np.array_equal(M.bits(bary), M.bits(got["bary"][has])) and np.array_equal(M.bits(dist), M.bits(got["dist"][has]))
    none = np.nonzero(f == M.NONE)[0]
    assert not got["bary"][none].any() and not got["dist"][none].any()


@pytest.fixture(scope="module")
def costed():
    """a 96-terrain whose vertex costs are its steepness (all below the cost limit: every pair of vertices has a path)"""
    mesh = meshgen.terrain(96, 0.1, 6, amplitude=0.6)
    plain = Case(mesh)
    steep, _ = plain.om.steepness(plain.vn, 0.3)
    return Case(mesh, np.minimum(steep, np.float32(0.9)), edge_cost_factor=1.0)


def plan_positions(case, n, seed):
    mesh = case.mesh
    goal, _ = M.surface_points(mesh, n, seed, sigma=0.02)
    start, _ = M.surface_points(mesh, n, seed + 1, sigma=0.02)
    return goal, start


@pytest.mark.parametrize("n", [1, 64, 512])
def test_dijkstra_plans_from_positions_equal_plans_from_oracle_ids(gpu_ctx_factory, costed, n):
    ctx = gpu_ctx_factory()
    costed.upload(ctx)
    goal, start = plan_positions(costed, n, 40 + n)
    if n > 1:
        goal[1] = [np.nan, 0.0, 0.0]                                   # no vertex: INVALID_START
        start[2] = [0.0, np.inf, 0.0]                                  # no vertex: INVALID_GOAL
    seeds = np.array([costed.om.nearest_vertex(p) for p in goal], np.uint32)
    targets = np.array([costed.om.nearest_vertex(p) for p in start], np.uint32)
    a = ctx.plan_dijkstra_batch_at(goal, start, want_fields=True)
    assert ctx.locate_stats()["built"] == 1
    b = ctx.plan_dijkstra_batch(seeds, targets, want_fields=True)
    assert np.array_equal(a["seeds"], seeds) and np.array_equal(a["targets"], targets)
    assert a["rc"] == b["rc"] and np.array_equal(a["codes"], b["codes"])
    if n > 1:
        assert a["codes"][1] == capi.INVALID_START and a["codes"][2] == capi.INVALID_GOAL
    assert (a["codes"] == capi.SUCCESS).sum() == (n - 2 if n > 1 else 1)
    assert np.array_equal(a["path_len"], b["path_len"])
    for k in range(n):
        assert np.array_equal(a["paths"][k], b["paths"][k])
    assert np.array_equal(M.bits(a["dist"]), M.bits(b["dist"])) and np.array_equal(a["pred"], b["pred"])


@pytest.mark.parametrize("n", [1, 64, 512])
def test_cvp_plans_from_positions_equal_plans_from_oracle_ids(gpu_ctx_factory, costed, n):
    ctx = gpu_ctx_factory()
    costed.upload(ctx)
    goal, start = plan_positions(costed, n, 80 + n)
    off_mesh = np.array([-0.5, -0.5, 0.0], np.float32)                 # beside the border: a nearest vertex, no face
    assert costed.om.containing_face(off_mesh)[0] == M.NONE and costed.om.nearest_vertex(off_mesh) != M.NONE
    if n > 1:
        goal[1] = off_mesh                                             # INVALID_START (52)
        start[2] = off_mesh                                            # INVALID_GOAL (53)
    sf = np.array([costed.om.containing_face(p)[0] for p in goal], np.uint32)
    tf = np.array([costed.om.containing_face(p)[0] for p in start], np.uint32)
    a = ctx.plan_cvp_batch_at(goal, start, want_fields=True, want_vecmap=True)
    b = ctx.plan_cvp_batch(goal, sf, tf, want_fields=True, want_vecmap=True)
    assert np.array_equal(a["seed_faces"], sf) and np.array_equal(a["target_faces"], tf)
    assert a["rc"] == b["rc"] and np.array_equal(a["codes"], b["codes"])
    if n > 1:
        assert a["codes"][1] == 52 and a["codes"][2] == 53
    ran = np.nonzero((sf != M.NONE) & (tf != M.NONE))[0]               # rows of rejected plans are never written
    assert ran.size >= 0.9 * n                                         # (a noisy surface point may have no face, as for the oracle)
    assert np.array_equal(M.bits(a["dist"][ran]), M.bits(b["dist"][ran])) and np.array_equal(a["pred"][ran], b["pred"][ran])
    assert np.array_equal(M.bits(a["vecmap"][ran]), M.bits(b["vecmap"][ran]))


def test_reupload_rebuilds_the_index_and_gives_the_first_round_again(gpu_ctx_factory):
    A = M.grid_meshes()["terrain"]()
    B = M.grid_meshes()["ceiling"]()
    omB = O.OracleMesh(B.xyz, B.faces)
    pa = np.concatenate([M.surface_points(A, 1500, 1)[0], M.far_points(A)])
    pb = np.concatenate([M.surface_points(B, 1500, 2)[0], M.far_points(B)])
    ctx = gpu_ctx_factory()
    upload(ctx, A)
    first = ctx.locate(pa)
    assert ctx.locate_stats()["built"] == 1
    again = ctx.locate(pa)
    assert ctx.locate_stats()["built"] == 0
    M.assert_same(again, first, "second call")
    bytes_first = ctx.device_bytes()
    upload(ctx, B)
    gb = ctx.locate(pb)
    assert ctx.locate_stats()["built"] == 1
    M.assert_same(gb, M.oracle_locate(omB, pb), "mesh B")
    ctx.locate(pb[:3])
    assert ctx.locate_stats()["built"] == 0
    upload(ctx, A)
    third = ctx.locate(pa)
    assert ctx.locate_stats()["built"] == 1
    M.assert_same(third, first, "mesh A again")
    assert ctx.device_bytes() == bytes_first


def test_errors_and_null_outputs(gpu_ctx_factory, costed):
    ctx = gpu_ctx_factory()
    pts, _ = M.surface_points(costed.mesh, 64, 3)
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        ctx.locate(pts)
    with pytest.raises(RuntimeError):
        ctx.plan_dijkstra_batch_at(pts, pts)
    assert ctx.locate(np.zeros((0, 3), np.float32))["vertex"].shape == (0,)   # n == 0: a no-op even without a mesh
    costed.upload(ctx)
    want = M.oracle_locate(costed.om, pts)
    none = ctx.locate(pts, want_vertex=False, want_face=False, want_bary=False, want_dist=False)
    assert all(v is None for v in none.values())
    only_face = ctx.locate(pts, want_vertex=False, want_bary=False, want_dist=False)
    assert np.array_equal(only_face["face"], want["face"])
    M.assert_same(ctx.locate(pts), want, "all outputs")
    # a failed call leaves the resident plan outputs and the layers untouched
    ctx.set_resident_outputs(True)
    ctx.layer_upload(0, costed.costs, None)
    s, t = costed.mesh.vertex_at(0.2, 0.2), costed.mesh.vertex_at(0.8, 0.8)
    ctx.plan_dijkstra_batch(np.array([s], np.uint32), np.array([t], np.uint32), goal_dist_offset=float("inf"))
    dist0 = ctx.download_output("dist", 0)
    rc = ctx._L.mnav_locate(ctx._h, 4, None, None, None, None, None)   # a null position array with n > 0
    assert rc < 0 and "null" in ctx._err()
    rc = ctx._L.mnav_plan_cvp_batch_at(ctx._h, 4, None, None, 0.3, 1.0, None, None, None, None, None, None)
    assert rc == capi.INTERNAL_ERROR and "null" in ctx._err()
    assert np.array_equal(M.bits(ctx.download_output("dist", 0)), M.bits(dist0))
    c, le = ctx.layer_download(0)
    assert np.array_equal(M.bits(c), M.bits(costed.costs))
    ctx.locate(pts)                                                    # and a successful lookup does not touch them either
    assert np.array_equal(M.bits(ctx.download_output("dist", 0)), M.bits(dist0))
