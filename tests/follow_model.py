"""The vector-field follower in Python / numpy, written from the reference's lines (mesh_controller.cpp:67-170
computeVelocityCommands, :225-242 naiveControl; mesh_map.cpp:625-672 directionAtPosition / costAtPosition, :999-1068
searchNeighbourFaces; util.h:182-183), NOT from mnav_follow.h: what tests/test_follow_model.py (CPU, against the header
compiled for the host) and tests/test_gpu_follow.py (device) compare with.  The pinned pieces are the oracle's:
om.containing_face (with om.nearest_vertex inside it) and its projectedBarycentricCoords (tests/locate_model.py).  acosf is
the host libm's own through ctypes, not the product's restatement.

Conventions the library adds (include/mnav.h): a vertex has a vector when its row of the vector map is not all zero, or
when it is a vertex of the plan's seed face and that face was passed; how = 1 first tick, 2 stayed, 3 neighbour search,
4 global search, 0 none; outputs a tick did not reach are zero (face: NONE)."""
import ctypes as C
import ctypes.util
import math

import numpy as np

from tests import locate_model as LM

F32 = np.float32
NONE = 0xFFFFFFFF
OK, OUT_OF_MAP, NO_FIELD = 0, 1, 2
HOW_NONE, HOW_FIRST, HOW_STAY, HOW_NEIGHBOUR, HOW_GLOBAL = 0, 1, 2, 3, 4

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = C.c_float
_libm.acosf.argtypes = [C.c_float]

DEFAULTS = dict(max_lin_velocity=1.0, max_ang_velocity=0.5, arrival_fading=0.5, ang_vel_factor=1.0, lin_vel_factor=1.0,
                max_angle=20.0, max_search_radius=0.4, max_search_distance=0.4)          # mesh_controller.h:193-200
CFG_NAMES = list(DEFAULTS)


def config(**kw):
    return {**DEFAULTS, **kw}


# -- lvr2::BaseVector<float> operations, every step rounded to float32 ------------------------------------------------------
def vec(p):
    return [F32(p[0]), F32(p[1]), F32(p[2])]


def add(a, b):
    return [F32(a[0] + b[0]), F32(a[1] + b[1]), F32(a[2] + b[2])]


def sub(a, b):
    return [F32(a[0] - b[0]), F32(a[1] - b[1]), F32(a[2] - b[2])]


def scale(a, s):
    return [F32(a[0] * s), F32(a[1] * s), F32(a[2] * s)]


def div(a, s):
    return [F32(a[0] / s), F32(a[1] / s), F32(a[2] / s)]


def dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def cross(a, b):
    return [F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])), F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))]


def length(a):
    return F32(np.sqrt(dot(a, a)))


def std_min(a, b):
    """std::min(a, b): b if b < a, else a (so a NaN second argument returns the first)"""
    return b if b < a else a


class Model:
    """the mesh as the controller's MeshMap sees it: positions, faces, getFacesOfVertex rows, vertex costs, the oracle"""

    def __init__(self, mesh, om, costs):
        self.xyz = np.ascontiguousarray(mesh.xyz, F32)
        self.faces = np.ascontiguousarray(mesh.faces, np.uint32)
        self.ptr, self.vf = om.vertex_faces()
        self.om = om
        self.costs = np.ascontiguousarray(costs, F32)
        self.V, self.F = self.xyz.shape[0], self.faces.shape[0]

    def tri(self, f):
        return [self.xyz[v] for v in self.faces[f]]

    def bary(self, p, f):
        """projectedBarycentricCoords (util.cpp:320-347): inside, bary, signed distance"""
        return LM.projected_barycentric(np.asarray(p, F32), *self.tri(f))

    def combine(self, f, b):
        """linearCombineBarycentricCoords over the face's vertex positions (util.h:182-183)"""
        t = self.tri(f)
        return add(add(scale(vec(t[0]), b[0]), scale(vec(t[1]), b[1])), scale(vec(t[2]), b[2]))

    def search_containing_face(self, p):
        """mesh_map.cpp:1120-1159 (the oracle's): (face, bary) or (NONE, zeros)"""
        f, b = self.om.containing_face(np.asarray(p, F32))
        return (NONE, np.zeros(3, F32)) if f == NONE or f < 0 else (int(f), b)

    def search_neighbour_faces(self, p, face, max_radius, max_dist):
        """mesh_map.cpp:999-1068; max_radius / max_dist are `const float&` parameters"""
        max_radius, max_dist = F32(max_radius), F32(max_dist)
        possible, listed = [int(face)], {int(face)}
        start = [vec(v) for v in self.tri(face)]
        center = [F32(0), F32(0), F32(0)]
        for v in start:
            center = add(center, v)                                               # :1010-1013
        center = div(center, F32(3))                                              # :1014
        vertex_center_max = F32(0)
        for v in start:
            d = sub(v, center)
            vertex_center_max = max(vertex_center_max, length(d))                 # :1019
        ext_radius = F32(max_radius + vertex_center_max)                          # :1022
        max_radius_sq = F32(ext_radius * ext_radius)                              # :1023
        it = 0
        while it < len(possible):                                                 # :1030
            f = possible[it]
            inside, b, dist = self.bary(p, f)
            if inside and F32(abs(dist)) < max_dist:                              # :1034
                return f, b
            for v in self.faces[f]:                                               # :1041
                d = sub(center, vec(self.xyz[v]))
                if dot(d, d) < max_radius_sq:                                     # :1043
                    for nn in self.vf[int(self.ptr[v]):int(self.ptr[v + 1])]:     # :1047-1048
                        if int(nn) not in listed:
                            possible.append(int(nn))
                            listed.add(int(nn))
            it += 1
        return NONE, np.zeros(3, F32)


def has_vector(model, vecmap, seed_face):
    """the library's convention: bool[V]"""
    has = (np.asarray(vecmap, F32) != 0).any(axis=1)
    if seed_face != NONE:
        has[model.faces[seed_face]] = True
    return has


def naive_control(cfg, mesh_dir, robot_dir, mesh_normal):
    """mesh_controller.cpp:225-242: (linear, angular) as float32"""
    phi = F32(_libm.acosf(float(dot(mesh_dir, robot_dir))))                         # :232
    sign_phi = dot(cross(mesh_dir, robot_dir), mesh_normal)                       # :233
    with np.errstate(invalid="ignore"):
        angular = F32(np.copysign(F32(float(phi) * cfg["max_ang_velocity"] / math.pi), F32(-sign_phi)))   # :237
        max_angle = F32(cfg["max_angle"] * math.pi / 180.0)                       # :238
        max_linear = F32(cfg["max_lin_velocity"])                                 # :239
        linear = F32(max_linear - F32(F32(phi * max_linear) / max_angle)) if phi <= max_angle else F32(0)   # :240
    return linear, angular


def lost(pos):
    return dict(code=OUT_OF_MAP, how=HOW_NONE, face=NONE, bary=np.zeros(3, F32), pos=np.asarray(pos, F32).copy(), mesh_dir=np.zeros(3, F32),
                cost=F32(0), cmd=np.zeros(2, np.float64))


def tick(model, cfg, vecmap, has, pos, robot_dir, up, face_in):
    """computeVelocityCommands (:67-170) for one robot; `has`: has_vector(...) of the plan's field"""
    pos = vec(pos)
    face, how = face_in, HOW_STAY
    with np.errstate(all="ignore"):
        if face_in == NONE:                                                       # :79
            face, b = model.search_containing_face(pos)                           # :82-83 (max_search_distance is ignored there)
            if face == NONE:
                return lost(pos)                                                  # :96
            pos, how = model.combine(face, b), HOW_FIRST                          # :91
        else:
            inside, b, dist = model.bary(pos, face_in)
            if inside and float(dist) < cfg["max_search_distance"]:               # :109-111 (float against double, signed)
                pass                                                              # :113-115: the position is kept
            else:
                face, b = model.search_neighbour_faces(pos, face_in, cfg["max_search_radius"], cfg["max_search_distance"])   # :116-117
                how = HOW_NEIGHBOUR
                if face == NONE:
                    face, b = model.search_containing_face(pos)                   # :129-130
                    how = HOW_GLOBAL
                    if face == NONE:
                        return lost(pos)                                          # :142
                pos = model.combine(face, b)                                      # :125 / :137
        out = lost(pos)
        out.update(code=NO_FIELD, how=how, face=int(face), bary=np.asarray(b, F32).copy())
        vs = model.faces[face]
        if not (has[vs[0]] or has[vs[1]] or has[vs[2]]):                          # mesh_map.cpp:634
            return out
        v = [F32(0), F32(0), F32(0)]
        for k in range(3):
            if has[vs[k]]:
                v = add(v, scale(vec(vecmap[vs[k]]), F32(b[k])))                  # :637-639
        if not (np.isfinite(v[0]) and np.isfinite(v[1]) and np.isfinite(v[2])):   # :640
            return out
        mesh_dir = div(v, length(v))                                              # mesh_controller.cpp:157 (normalised once)
        c = model.costs
        cost = F32(F32(F32(c[vs[0]] * b[0]) + F32(c[vs[1]] * b[1])) + F32(c[vs[2]] * b[2]))   # :158
        linear, angular = naive_control(cfg, mesh_dir, vec(robot_dir), vec(up))   # :160
        lin = std_min(cfg["max_lin_velocity"], float(linear) * cfg["lin_vel_factor"])   # :161
        ang = std_min(cfg["max_ang_velocity"], float(angular) * cfg["ang_vel_factor"])  # :162
        out.update(code=OK, mesh_dir=np.asarray(mesh_dir, F32), cost=cost, cmd=np.array([lin, ang], np.float64))
        return out


def tick_batch(model, cfg, fields, robots):
    """tick for every robot of `robots` (dict of arrays: pos, dir, up, face_in, slot, seed_face); fields[s] = vector map of
    plan s.  seed_face may be None.  Returns a dict of arrays."""
    n = robots["pos"].shape[0]
    out = dict(code=np.zeros(n, np.int32), how=np.zeros(n, np.int32), face=np.zeros(n, np.uint32), bary=np.zeros((n, 3), F32),
               pos=np.zeros((n, 3), F32), mesh_dir=np.zeros((n, 3), F32), cost=np.zeros(n, F32), cmd=np.zeros((n, 2), np.float64))
    cache = {}
    for i in range(n):
        s = int(robots["slot"][i])
        sf = NONE if robots.get("seed_face") is None else int(robots["seed_face"][i])
        if (s, sf) not in cache:
            cache[(s, sf)] = has_vector(model, fields[s], sf)
        r = tick(model, cfg, fields[s], cache[(s, sf)], robots["pos"][i], robots["dir"][i], robots["up"][i], int(robots["face_in"][i]))
        for k in out:
            out[k][i] = r[k]
    return out


def same_bits(a, b):
    """equal as bits; two NaNs are equal whatever their sign and payload (IEEE 754 leaves both to the implementation)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same(got, want, what=""):
    for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if not same_bits(g.astype(w.dtype) if g.dtype.kind != "f" else g, w):
            bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
            raise AssertionError((what, k, bad[:8], g[bad[:3]], w[bad[:3]]))


def plan_ends(mesh, n_plans):
    """goal and robot faces of n_plans plans: goals around the mesh's middle, robots on rings further and further out (the
    waves stop a little beyond them: the outer part of the mesh has no vectors).  Returns (goal_faces, robot_faces)."""
    cen = mesh.xyz[mesh.faces].astype(np.float64).mean(axis=1)
    order = np.argsort(np.linalg.norm(cen - cen.mean(axis=0), axis=1), kind="stable")
    goal = [int(order[min(7 * k, mesh.F - 1)]) for k in range(n_plans)]
    robot = [int(order[int((0.35 + 0.4 * k / max(n_plans, 1)) * (mesh.F - 1))]) for k in range(n_plans)]
    return np.array(goal, np.uint32), np.array(robot, np.uint32)


# -- robots ----------------------------------------------------------------------------------------------------------------
def face_normals(model):
    t = model.xyz[model.faces].astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)


def face_points(model, f, rng, lo=0.08):
    """a point well inside each face of f (every barycentric >= lo)"""
    w = rng.dirichlet(np.ones(3), f.shape[0]) * (1.0 - 3.0 * lo) + lo
    return (model.xyz[model.faces[f]].astype(np.float64) * w[:, :, None]).sum(axis=1)


def rotate(v, axis, angle):
    """Rodrigues, in double"""
    v, axis = np.asarray(v, np.float64), np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return v * math.cos(angle) + np.cross(axis, v) * math.sin(angle) + axis * np.dot(axis, v) * (1.0 - math.cos(angle))


FAMILIES = ["first", "stay", "neighbour", "far", "beside", "above", "below", "degenerate", "angles"]


def make_robots(model, n_slots, seed_faces, seed, per_family=48):
    """Robots of every query family, `per_family` each, robot i on plan i % n_slots; seed_faces[s] = seed face of plan s
    or NONE.  Returns (robots, family index per robot).  Headings are random unit vectors near the tangent plane, `up` is
    +z tilted a little; the "angles" family gets its headings from set_angles()."""
    rng = np.random.default_rng(seed)
    cen = model.xyz[model.faces].astype(np.float64).mean(axis=1)
    nrm = face_normals(model)
    lo, hi = np.nanmin(model.xyz, axis=0).astype(np.float64), np.nanmax(model.xyz, axis=0).astype(np.float64)
    pos, face_in, fam = [], [], []
    m = per_family
    for k, name in enumerate(FAMILIES):
        f = rng.integers(0, model.F, m)
        p = face_points(model, f, rng)
        if name == "first":
            p = p + nrm[f] * rng.normal(0, 0.03, (m, 1))
            fi = np.full(m, NONE)
        elif name in ("stay", "angles"):
            p = p + nrm[f] * rng.uniform(-0.05, 0.05, (m, 1))
            fi = f
        elif name in ("neighbour", "far"):
            fi = f.copy()
            for j in range(m):                                                    # the robot was on fi[j], now stands on another face
                while True:
                    d = np.linalg.norm(cen - cen[fi[j]], axis=1)
                    near = np.nonzero((d > 0.05) & (d < 0.3) if name == "neighbour" else d > 0.95)[0]
                    if near.size:
                        break
                    fi[j] = rng.integers(0, model.F)                              # (a small mesh: not every face has a far partner)
                p[j] = face_points(model, np.array([rng.choice(near)]), rng)[0]
        elif name == "beside":
            side = rng.integers(0, 4, m)
            off = rng.uniform(0.3, 1.0, m)
            p[:, 0] = np.where(side == 0, lo[0] - off, np.where(side == 1, hi[0] + off, p[:, 0]))
            p[:, 1] = np.where(side == 2, lo[1] - off, np.where(side == 3, hi[1] + off, p[:, 1]))
            fi = np.where(rng.uniform(size=m) < 0.3, NONE, f)
        elif name in ("above", "below"):
            p = p + nrm[f] * (0.6 if name == "above" else -0.6)                   # beyond max_search_distance on either side
            fi = f
        else:                                                                     # degenerate
            bad = [np.nan, np.inf, -np.inf]
            for j in range(m):
                p[j, j % 3] = bad[(j // 3) % 3]
            fi = np.where(np.arange(m) % 2 == 0, NONE, f)
        pos.append(p); face_in.append(fi); fam.append(np.full(m, k))
    pos = np.concatenate(pos).astype(F32)
    n = pos.shape[0]
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.sin(a), rng.normal(0, 0.1, n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    up = np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), np.ones(n)], axis=1)
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    slot = (np.arange(n) % n_slots).astype(np.uint32)
    sf = np.asarray(seed_faces, np.uint32)[slot]
    return dict(pos=pos, dir=d.astype(F32), up=up.astype(F32), face_in=np.concatenate(face_in).astype(np.uint32), slot=slot, seed_face=sf), \
        np.concatenate(fam)


ANGLES_DEG = [0.0, 180.0, 5.0, -5.0, 19.0, -19.0, 21.0, -21.0, 60.0, -60.0, 44.0, -46.0]


def set_angles(model, cfg, fields, robots, fam):
    """the "angles" family: heading = the field's direction at the robot turned about `up` by ANGLES_DEG in turn (0 and
    180: heading parallel to mesh_dir, sign_phi == 0 exactly; the others: both signs, both sides of max_angle)"""
    idx = np.nonzero(fam == FAMILIES.index("angles"))[0]
    sub_r = {k: (None if v is None else v[idx]) for k, v in robots.items()}
    first = tick_batch(model, cfg, fields, sub_r)
    for j, i in enumerate(idx):
        if first["code"][j] != OK or not np.isfinite(first["mesh_dir"][j]).all():
            continue
        md, ang = first["mesh_dir"][j], ANGLES_DEG[j % len(ANGLES_DEG)]
        if ang == 0.0:
            robots["dir"][i] = md
        elif ang == 180.0:
            robots["dir"][i] = -md
        else:
            robots["dir"][i] = rotate(md, robots["up"][i], math.radians(ang)).astype(F32)
    return robots


def assert_every_branch(want, fam, cfg, what):
    """the MODEL took every `how` and every code, and the families did what they are there for"""
    hows, codes = set(want["how"].tolist()), set(want["code"].tolist())
    assert hows >= {1, 2, 3, 4} and codes == {OK, OUT_OF_MAP, NO_FIELD}, (what, hows, codes)
    of = lambda name: fam == FAMILIES.index(name)
    assert (want["how"][of("first")] <= 1).all() and (want["how"][of("first")] == 1).any()
    assert (want["how"][of("stay")] == 2).all()
    assert (want["how"][of("neighbour")] == 3).mean() > 0.5, what
    assert (want["how"][of("far")] == 4).mean() > 0.5, what
    assert (want["code"][of("beside")] == OUT_OF_MAP).all()
    assert (want["code"][of("degenerate")] == OUT_OF_MAP).all()
    if cfg["max_search_distance"] < 0.6:
        assert (want["how"][of("above")] != 2).all()                  # too far above: the face is given up ...
        assert (want["how"][of("below")] == 2).all()                  # ... but the signed compare keeps a robot far below it
    ok = want["code"] == OK
    lin, ang = want["cmd"][ok, 0], want["cmd"][ok, 1]
    assert (lin > 0).any() and (lin == 0).any() and (ang > 0).any() and (ang < 0).any(), what    # phi on both sides of max_angle, both signs
    return ok


def unicycle_step(pos, d, up, lin, ang, dt):
    """the test's own integrator: pos += dir * lin * dt, heading turned by ang * dt about up (double, stored as float32)"""
    p = (np.asarray(pos, np.float64) + np.asarray(d, np.float64) * lin * dt).astype(F32)
    nd = rotate(d, up, ang * dt)
    return p, (nd / np.linalg.norm(nd)).astype(F32)
