import numpy as np

from mesh_navigation_amd import meshgen
from oracle import oracle as O


def test_sizes_of_survey_table():
    m = meshgen.terrain(224, 0.1, 1)           # config "50k"
    assert (m.V, m.F, m.E) == (50176, 99458, 149633)


def test_edge_convention_matches_oracle():
    for mesh in (meshgen.terrain(17, 0.1, 4), meshgen.flat_grid(6)):
        om = O.OracleMesh(mesh.xyz, mesh.faces)
        assert np.array_equal(om.edges(), mesh.edges)
        assert np.array_equal(om.face_edges(), mesh.face_edges)
        assert np.array_equal(om.edge_distances().view(np.uint32), meshgen.edge_lengths(mesh).view(np.uint32))


def test_terrain_is_seeded_and_ccw():
    a, b = meshgen.terrain(20, 0.1, 9), meshgen.terrain(20, 0.1, 9)
    assert np.array_equal(a.xyz, b.xyz)
    assert not np.array_equal(a.xyz, meshgen.terrain(20, 0.1, 10).xyz)
    om = O.OracleMesh(a.xyz, a.faces)
    assert (om.face_normals()[:, 2] > 0).all()


def test_grid_edges_closed_form_matches_first_appearance_order():
    """meshgen.grid_edges (no sort; the 10M-vertex bench mesh) == edges_from_faces(grid_faces) (lvr2/pmp edge ids)"""
    from mesh_navigation_amd import meshgen
    for N in (2, 3, 7, 33):
        e1, fe1 = meshgen.edges_from_faces(meshgen.grid_faces(N))
        e2, fe2 = meshgen.grid_edges(N)
        assert np.array_equal(e1, e2) and np.array_equal(fe1, fe2)


def _valences(mesh):
    deg = np.bincount(mesh.edges.ravel(), minlength=mesh.V)
    return {int(k): int(v) for k, v in zip(*np.unique(deg, return_counts=True))}


def _checked(mesh):
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    assert om.manifold                                               # every edge in at most two faces
    assert np.array_equal(om.edges(), mesh.edges) and np.array_equal(om.face_edges(), mesh.face_edges)
    assert (om.face_normals()[:, 2] > 0).all()                       # counter-clockwise seen from +z
    assert mesh.V - mesh.E + mesh.F == 1 + int((np.bincount(mesh.edges.ravel(), minlength=mesh.V) == 0).sum())   # a disc + its face-less vertices
    return om


def test_union_jack_alternates_valence_4_and_8():
    m = meshgen.union_jack(96, 0.1, 3, 0.5)
    _checked(m)
    assert (m.V, m.F, m.E) == (9216, 18050, 27265)
    assert _valences(m) == {2: 2, 3: 190, 4: 4418, 5: 188, 8: 4418}
    assert np.array_equal(m.xyz, meshgen.terrain(96, 0.1, 3, amplitude=0.5).xyz)
    deg = np.bincount(m.edges.ravel(), minlength=m.V).reshape(96, 96)
    j, i = np.mgrid[1:95, 1:95]
    assert np.array_equal(deg[1:95, 1:95], np.where((i + j) % 2 == 0, 8, 4))
    f = meshgen.union_jack(48, 1.0, flat=True)                       # flat: the vertices of flat_grid, many equal potentials
    _checked(f)
    assert (f.V, f.F, f.E) == (2304, 4418, 6721)
    assert _valences(f) == {2: 2, 3: 94, 4: 1058, 5: 92, 8: 1058}
    assert np.array_equal(f.xyz, meshgen.flat_grid(48, 1.0).xyz)
    om = O.OracleMesh(f.xyz, f.faces)
    w = om.edge_distances()
    d = om.dijkstra(w, np.zeros(f.V, np.float32), f.vertex_at(0.5, 0.5), f.vertex_at(0.9, 0.9), goal_dist_offset=np.inf).dist
    assert np.isfinite(d).all() and len(np.unique(d)) == 325          # 2304 vertices, 325 distinct potentials from the centre


def test_hub_terrain_valences_and_faceless_vertices():
    hubs = [(20, 20, 1), (60, 30, 2), (40, 90, 3), (100, 100, 5), (64, 64, 1), (90, 40, 2)]
    m = meshgen.hub_terrain(128, hubs, 0.1, 3)
    _checked(m)
    assert (m.V, m.F, m.E) == (16384, 32018, 48281)
    assert _valences(m) == {0: 120, 2: 2, 3: 2, 4: 504, 5: 88, 6: 15650, 7: 12, 8: 2, 16: 2, 24: 1, 40: 1}
    deg = np.bincount(m.edges.ravel(), minlength=m.V)
    for ci, cj, k in hubs:
        assert deg[cj * 128 + ci] == 8 * k
        inner = [(cj + dj) * 128 + ci + di for dj in range(-k + 1, k) for di in range(-k + 1, k) if (di, dj) != (0, 0)]
        assert (deg[inner] == 0).all() and len(inner) == (2 * k - 1) ** 2 - 1      # the hub's former interior neighbours
    assert np.array_equal(m.xyz, meshgen.terrain(128, 0.1, 3, amplitude=0.5).xyz)
    for bad in ([(1, 5, 2)], [(20, 20, 2), (22, 22, 1)]):                         # a block leaving the grid, two blocks sharing cells
        try:
            meshgen.hub_terrain(32, bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def _lattice_checked(mesh, chi, valences):
    """a (u, v) lattice mesh: manifold, the oracle's edge ids, Euler characteristic, valence range, no zero-length edge"""
    om = O.OracleMesh(mesh.xyz, mesh.faces)
    assert om.manifold
    assert np.array_equal(om.edges(), mesh.edges) and np.array_equal(om.face_edges(), mesh.face_edges)
    assert np.array_equal(om.edge_distances().view(np.uint32), meshgen.edge_lengths(mesh).view(np.uint32))
    assert mesh.V - mesh.E + mesh.F == chi
    deg = np.bincount(mesh.edges.ravel(), minlength=mesh.V)
    assert (int(deg.min()), int(deg.max())) == valences
    assert om.edge_distances().min() > 0
    return om, deg


def test_ramp_is_an_open_helicoid_of_several_storeys():
    m = meshgen.ramp(320, 12, 8.0, 0.05, 1.0, 1.2, 0)
    _, deg = _lattice_checked(m, 1, (2, 6))                         # a disc
    assert (m.V, m.F, m.E) == (3840, 7018, 10857)
    assert np.array_equal(m.xyz, meshgen.ramp(320, 12, 8.0, 0.05, 1.0, 1.2, 0).xyz) and not np.array_equal(m.xyz, meshgen.ramp(seed=1).xyz)
    assert np.array_equal(m.faces[:2], [[0, 1, 321], [0, 321, 320]])   # vertex id j * nu + i, cell (a, b, c, d) -> (a, b, c), (a, c, d)
    assert sorted(deg[[0, 319, 320 * 11, 320 * 12 - 1]]) == [2, 2, 3, 3] and (deg.reshape(12, 320)[1:-1, 1:-1] == 6).all()
    rho = np.hypot(m.xyz[:, 0], m.xyz[:, 1])
    assert 0.97 < rho.min() < 1.03 and 2.17 < rho.max() < 2.23       # lane from r0 to r0 + width, jittered inside the surface
    assert 0.39 < np.ptp(m.xyz[:, 2]) < 0.41                         # 8 turns, 0.05 apart: the height is far below the footprint
    up = m.xyz[5 * 320 + 100 + 40] - m.xyz[5 * 320 + 100]            # one turn further along the lane (319 / 8 ~ 40): one storey up
    assert abs(up[2] - 0.05) < 0.005 and np.hypot(up[0], up[1]) < 0.2


def test_torus_is_closed_with_valence_six_everywhere():
    m = meshgen.torus(64, 32, 2.0, 0.8, 0)
    _lattice_checked(m, 0, (6, 6))
    assert (m.V, m.F, m.E) == (2048, 4096, 6144)
    assert (np.bincount(m.face_edges.ravel(), minlength=m.E) == 2).all()   # no boundary: every edge in two faces
    rho = np.hypot(m.xyz[:, 0], m.xyz[:, 1])
    assert np.abs(np.hypot(rho - 2.0, m.xyz[:, 2]) - 0.8).max() < 1e-5


def test_tube_is_a_vertical_wall_with_horizontal_normals():
    m = meshgen.tube(48, 40, 0.8, 3.0, 0)
    om, deg = _lattice_checked(m, 0, (4, 6))                         # an annulus
    assert (m.V, m.F, m.E) == (1920, 3744, 5664)
    fn = om.face_normals()
    assert (fn[:, 2] == 0).all() and np.abs(np.hypot(fn[:, 0], fn[:, 1]) - 1).max() < 1e-6
    assert (om.vertex_normals(fn)[:, 2] == 0).all()
    assert (np.bincount(m.face_edges.ravel(), minlength=m.E) == 1).sum() == 2 * 48   # two boundary loops


def test_moved_translates_in_float64_and_rounds_once():
    m = meshgen.ramp(64, 6, 2.0, 0.05, 1.0, 1.2, 3)
    t = (-2048.0, 4096.0, 300.0)
    mv = meshgen.moved(m, t)
    _lattice_checked(mv, 1, (2, 6))
    assert np.array_equal(mv.faces, m.faces) and np.array_equal(mv.edges, m.edges)
    assert np.array_equal(mv.xyz, (m.xyz.astype(np.float64) + np.array(t)).astype(np.float32))
    assert np.abs(mv.xyz.astype(np.float64) - np.array(t) - m.xyz).max() <= 2.0 ** -12          # half an ulp of [4096, 8192)
