"""The local-neighbourhood layers on the device (mnav_layer_height_diff / _roughness / _ridge; HeightDiffLayer,
RoughnessLayer, RidgeLayer of mesh_layers).  Every comparison is exact against tests/nbhd_model.py: float bits, lethal
bytes, Σ|N(v)| and max |N(v)|."""
import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import nbhd_model as M

pytestmark = pytest.mark.gpu

OPS = (M.HEIGHT, M.ROUGH, M.RIDGE)
THRESHOLD = {M.HEIGHT: 0.185, M.ROUGH: 0.3, M.RIDGE: 0.3}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def normals(mesh):
    return O.OracleMesh(mesh.xyz, mesh.faces).vertex_normals()


def run(ctx, op, layer, radius, threshold):
    f = {M.HEIGHT: ctx.layer_height_diff, M.ROUGH: ctx.layer_roughness, M.RIDGE: ctx.layer_ridge}[op]
    return f(layer, radius=radius, threshold=threshold)


def check(ctx, mesh, nrm, radius, centres=None, layer=5, ops=OPS):
    """every op on the device against the model (all centres, or the given sample); returns the stats of the last call"""
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    for op in ops:
        st = run(ctx, op, layer, radius, THRESHOLD[op])
        c, le = ctx.layer_download(layer)
        want, wle, size = M.layer(op, row_ptr, nbr, mesh.xyz, nrm, radius, THRESHOLD[op], centres)
        idx = np.arange(mesh.V) if centres is None else np.asarray(centres)
        assert np.array_equal(bits(c[idx]), bits(want)), (op, radius, int((bits(c[idx]) != bits(want)).sum()))
        assert np.array_equal(le[idx], wle), op
        assert st["centres"] == mesh.V
        if centres is None:
            assert st["visits"] == int(size.sum()) and st["max_size"] == int(size.max()), (op, st, int(size.sum()), int(size.max()))
        else:
            assert st["max_size"] >= int(size.max())
    return st


@pytest.mark.parametrize("radius", [0.3, 1.0])
def test_terrain_96_every_centre(gpu_ctx_factory, radius):
    mesh = meshgen.terrain(96, 0.1, 7)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    st = check(ctx, mesh, nrm, radius)
    if radius == 1.0:
        assert st["spilled"] > 0                                  # ~300 members: beyond the default LDS cap


def test_terrain_300(gpu_ctx_factory):
    mesh = meshgen.terrain(300, 0.1, 3)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    check(ctx, mesh, nrm, 0.3)
    rng = np.random.default_rng(300)
    check(ctx, mesh, nrm, 1.0, centres=np.sort(rng.choice(mesh.V, 3000, replace=False)))


@pytest.mark.parametrize("name", ["punched", "fan_field", "two_sheets"])
def test_irregular_meshes(gpu_ctx_factory, name):
    mesh = {"punched": lambda: meshgen.punched(80, 0.1, 4, drop=0.12),
            "fan_field": lambda: meshgen.fan_field(40, 8, 2),
            "two_sheets": lambda: M.two_sheets(40)}[name]()
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    for radius in (0.15, 0.3, 0.6):
        check(ctx, mesh, nrm, radius)


def test_exact_boundary_zero_radius_and_whole_component(gpu_ctx_factory):
    mesh = M.exact_boundary(12)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    st = check(ctx, mesh, nrm, 0.5)                               # grid neighbours at d2 == r*r exactly: N(v) = {v}
    assert st["visits"] == mesh.V and st["max_size"] == 1
    check(ctx, mesh, nrm, 0.75)
    t = meshgen.terrain(24, 0.1, 9)
    tn = normals(t)
    ctx.upload_mesh(t.xyz, t.faces, t.edges, tn)
    for op in OPS:                                                # r = 0: {v}, height 0, ridge 0
        st = run(ctx, op, 1, 0.0, THRESHOLD[op])
        c, le = ctx.layer_download(1)
        assert st["visits"] == t.V and st["max_size"] == 1
        if op != M.ROUGH:
            assert (c == 0.0).all() and not le.any()
    check(ctx, t, tn, 0.0, ops=(M.ROUGH,))
    st = check(ctx, t, tn, 100.0)                                 # larger than the mesh: the whole component
    assert st["max_size"] == t.V and st["visits"] == t.V * t.V
    g = meshgen.terrain(36, 0.1, 4)                               # a component beyond the first global spill capacity (1024)
    gn = normals(g)
    ctx.upload_mesh(g.xyz, g.faces, g.edges, gn)
    st = check(ctx, g, gn, 100.0, ops=(M.HEIGHT,))
    assert st["max_size"] == g.V > 1024 and st["spilled"] == g.V


def test_c2_mesh_sample(gpu_ctx_factory):
    mesh = meshgen.terrain(1000, 0.1, 2)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    rng = np.random.default_rng(2024)
    N = 1000
    border = np.concatenate([np.arange(N), np.arange(N) * N, np.arange(N) * N + N - 1, (N - 1) * N + np.arange(N)])
    fixed = np.unique(np.concatenate([[0, mesh.V - 1], rng.choice(border, 200, replace=False)]))
    rest = rng.permutation(np.setdiff1d(np.arange(mesh.V), fixed))[:4096 - fixed.size]
    sample = np.sort(np.concatenate([fixed, rest]))
    assert sample.size == 4096
    st = check(ctx, mesh, nrm, 0.3, centres=sample)
    assert st["visits"] > 20 * mesh.V


def test_spill_path_and_repeat_give_the_same_bits(gpu_ctx_factory):
    mesh = meshgen.terrain(96, 0.1, 7)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    for op in OPS:
        base = run(ctx, op, 2, 0.4, THRESHOLD[op])
        c0, l0 = ctx.layer_download(2)
        again = run(ctx, op, 2, 0.4, THRESHOLD[op])
        c1, l1 = ctx.layer_download(2)
        assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(l0, l1) and again == {**base, "ms": again["ms"]}
        ctx.set_option("nbhd_lds_cap", 32)                        # the smallest LDS cap: most centres leave the LDS path
        sp = run(ctx, op, 3, 0.4, THRESHOLD[op])
        ctx.set_option("nbhd_lds_cap", None)
        c2, l2 = ctx.layer_download(3)
        assert sp["spilled"] > 0 and base["spilled"] == 0, (base, sp)
        assert sp["visits"] == base["visits"] and sp["max_size"] == base["max_size"]
        assert np.array_equal(bits(c0), bits(c2)) and np.array_equal(l0, l2)


def test_height_diff_layer_feeds_combination_and_inflation(gpu_ctx_factory):
    mesh = meshgen.terrain(96, 0.1, 7)
    nrm = normals(mesh)
    ctx = gpu_ctx_factory()
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, nrm)
    ctx.layer_steepness(0, 0.6)
    ctx.layer_height_diff(1)
    hc, hl = ctx.layer_download(1)
    assert 0 < hl.sum() < mesh.V
    ctx.layer_upload(2, hc, hl)
    ctx.combine_layers([1, 0], [1.0, 2.0], mode="avg", edge_cost_factor=1.0)
    a = ctx.download_costs()
    ctx.combine_layers([2, 0], [1.0, 2.0], mode="avg", edge_cost_factor=1.0)
    b = ctx.download_costs()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    ctx.layer_inflation(3, 1)
    ia = ctx.layer_download(3, distances=True)
    ctx.layer_inflation(4, 2)
    ib = ctx.layer_download(4, distances=True)
    for x, y in zip(ia, ib):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def test_errors_leave_the_layer_untouched(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        ctx.layer_height_diff(0)
    mesh = meshgen.terrain(24, 0.1, 1)
    ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, None)           # no normals
    ctx.layer_height_diff(0, radius=0.3, threshold=0.05)
    c0, l0 = ctx.layer_download(0)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        for f in (ctx.layer_height_diff, ctx.layer_roughness, ctx.layer_ridge):
            with pytest.raises(RuntimeError, match="radius"):
                f(0, radius=bad)
    with pytest.raises(RuntimeError, match="normals"):
        ctx.layer_roughness(0)
    with pytest.raises(RuntimeError, match="normals"):
        ctx.layer_ridge(0)
    with pytest.raises(RuntimeError, match="layer index"):
        ctx.layer_height_diff(64)
    c1, l1 = ctx.layer_download(0)
    assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(l0, l1)
