"""Headless scene builders for the admm-elastic hot path (host side, numpy).

These replace the reference's GUI sample glue that *feeds* `admm::Solver`
(SURVEY.md §8f item 2):

* `tri_blocks(nx, ny)`  -- the mesh of mclscene `factory::make_tri_blocks`
  (admm_anderson_hard_zxu/deps/mclscene/include/MCL/ShapeFactory.hpp:499-548): unit
  squares with a centre vertex, 4 triangles per square [(d,a,e),(a,b,e),(b,c,e),(c,d,e)].
  Vertices are indexed directly on the structured grid (corners first, then centres)
  instead of through mclscene's O(T*n) `refine()` merge -- the connectivity is the same,
  only the vertex numbering differs.
* `tet_blocks(cx, cy, cz)` -- `factory::make_tet_blocks` (ShapeFactory.hpp:436-496), five
  tets per unit cube with the reference's corner labelling (a..h) and tet table.
* lumped masses as `TriangleMesh::weighted_masses` (TriangleMesh.hpp:281-296) and
  `TetMesh::weighted_masses` (TetMesh.hpp:297-315), bound per node x3 like
  `binding::add_trimesh/add_tetmesh` (samples/utils/AddMeshes.hpp:97-235).
* pin rules of the samples: windyflag `get_pins` (two corners of the min-x edge,
  samples/Asia2019/windyflag.cpp:29-61) and the cantilever "x = min face" rule.

A `Scene` is a plain container of fp64/int32 arrays -- exactly what the C ABI
(`include/aa_admm.h`) takes -- plus the solver settings of the reference's
`Solver::Settings` (Solver.hpp:45-67). `oracle/refio.write_scene` serialises it for the reference
driver under oracle/ (test infrastructure only).
"""
from __future__ import annotations

import dataclasses
import os
from typing import List, Optional

import numpy as np

TET, TRI = 0, 1
# passive obstacles (PassiveObject.hpp:32-136; include/aa_admm.h AA_OBS_*)
OBS_FLOOR, OBS_SLIDE_FLOOR, OBS_SPHERE, OBS_PLANE_HALF_SPHERE, OBS_CYLINDER = 0, 1, 2, 3, 4
OBS_MESH = 5   # PassiveMesh (:138-178): Scene.mesh_obstacles / capi.Solver.add_mesh_obstacle
LINEAR, NEOHOOKEAN, STVK = 0, 1, 2
# spring modes (include/aa_admm.h AA_SPRING_*): two-sided, slack below / above L; | SPRING_HARD
SPRING, SPRING_TETHER, SPRING_STRUT, SPRING_HARD = 0, 1, 2, 4
VARIANT_X, VARIANT_H = 0, 1  # admm_anderson_xzu (z-AA) / admm_anderson_hard_zxu ((u,x)-AA)


def lame(E: float, nu: float):
    """mu, lambda, bulk modulus k = lambda + 2/3 mu (EnergyTerm.hpp:35-61)."""
    mu = E / (2.0 * (1.0 + nu))
    lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return mu, lam, lam + (2.0 / 3.0) * mu


@dataclasses.dataclass
class ElementGroup:
    kind: int             # TET or TRI
    material: int         # LINEAR / NEOHOOKEAN / STVK (tets); LINEAR for tris
    E: float              # E, nu, limit_min, limit_max: scalars, or arrays of the group's length
    nu: float             # (per-element materials: the reference's one Lame per EnergyTerm)
    idx: np.ndarray       # int32 (count, 4) or (count, 3)
    limit_min: float = -100.0   # Lame defaults (EnergyTerm.hpp:54-55)
    limit_max: float = 100.0

    @property
    def per_element(self) -> bool:
        return any(np.ndim(a) > 0 for a in (self.E, self.nu, self.limit_min, self.limit_max))

    def material_arrays(self):
        """E, nu, limit_min, limit_max as fp64 arrays of the group's length (scalars broadcast)."""
        n = len(self.idx)
        out = []
        for a in (self.E, self.nu, self.limit_min, self.limit_max):
            a = np.asarray(a, np.float64)
            if a.ndim > 0 and a.shape != (n,):
                raise ValueError(f"per-element material array of shape {a.shape} for a group of {n} elements")
            out.append(np.broadcast_to(a, (n,)).copy())
        return out


@dataclasses.dataclass
class Scene:
    x: np.ndarray                 # (n, 3) fp64 rest/initial positions
    masses: np.ndarray            # (n,) fp64 lumped node masses
    groups: List[ElementGroup]
    pin_idx: np.ndarray           # (p,) int32
    pin_pts: np.ndarray           # (p, 3) fp64 pin targets for the first step
    pin_vel: np.ndarray           # (p, 3) fp64 pin displacement per time step
    variant: int = VARIANT_H
    dt: float = 1.0 / 30.0
    gravity: float = -9.8
    penalty: float = 1.0
    iters: int = 100
    accel: int = 1
    aa_m: int = 6
    n_steps: int = 1
    name: str = "scene"
    rest: Optional[np.ndarray] = None   # (n, 3) rest positions of the elements; None = x
    # (u,x) variant extras (admm_anderson_hard_zxu): passive obstacles [(type, params)] and the
    # collision-checked nodes (Solver::add_obstacle / set_collisions), and WindForces
    # [(tris (t, 3) int32, direction (3,))] (Solver::ext_forces)
    obstacles: list = dataclasses.field(default_factory=list)
    collision_idx: Optional[np.ndarray] = None
    # triangle-mesh obstacles [(V (n, 3), F (m, 3))]: closed, outward-oriented surfaces, added after
    # `obstacles` in the insertion order (capi.solver_from_scene)
    mesh_obstacles: list = dataclasses.field(default_factory=list)
    # kinematic mesh obstacles: (n_steps, n_meshes, 12) rigid poses, R row-major (obstacle frame ->
    # world) then t; the scene runner sets row k - 1 before step k, where it advances the moving
    # pins (capi.run_scene). None = the meshes stay as given.
    mesh_obstacle_poses: Optional[np.ndarray] = None
    # deforming mesh obstacles: a list over steps, each entry a list over meshes of (nv, 3) vertex
    # arrays (the mesh's own vertex count and triangles) or None for "leave as is"; step k runs
    # against entry k - 1 and the last entry holds on (capi.run_scene, after the poses). None = the
    # meshes keep their shape.
    mesh_obstacle_vertices: Optional[list] = None
    # bound mesh obstacles (the obstacle is another simulated body): a list over meshes of (nv,) node
    # index arrays -- vertex i of the mesh follows node [i] from every step's start state -- or None
    # for a mesh the caller drives; and, per mesh, the nodes whose collision terms skip that mesh
    # (a body is exempt from its own surface). None = no mesh is bound / no node is exempt.
    mesh_obstacle_bindings: Optional[list] = None
    mesh_obstacle_exempt: Optional[list] = None
    # carry: per mesh, True = the friction pass takes the mesh's displacement at a contact from its
    # vertices' own motion (capi.solver_from_scene switches it on). None = no mesh carries.
    mesh_obstacle_carry: Optional[list] = None
    # (n, 3) node velocities set through set_v after initialize (capi.run_scene); None = at rest
    initial_velocity: Optional[np.ndarray] = None
    winds: list = dataclasses.field(default_factory=list)
    # Coulomb friction: a coefficient (or None) per obstacle row of the insertion order, `obstacles`
    # first, then `mesh_obstacles` (capi.solver_from_scene); record_contacts keeps the per-term contact
    # records even with every coefficient 0. None / False = no friction pass, today's scene.
    obstacle_friction: Optional[list] = None
    record_contacts: bool = False
    # moving analytic obstacles: a list over steps, each entry a list over the rows of `obstacles` of
    # new parameters or None for "leave as is"; step k runs against entry k - 1 and the last entry
    # holds on (capi.run_scene, with the poses)
    obstacle_motion: Optional[list] = None
    # bending: a list of (tris (m, 3) int32, k_bend, flat_rest) -- hinges on the interior edges of each
    # triangle list, rest shape from rest_x (capi.solver_from_scene binds them after the groups,
    # Solver.add_bending). Not an ElementGroup: the reference has no bending term, so the oracle and the
    # reference driver never see it. None = a pure membrane, today's scene.
    bending: Optional[list] = None
    # springs: a list of (pairs (m, 2) int32, k (scalar or (m,)), rest ((m,), scalar or None = the
    # pairs' distances in rest_x), mode) -- two-node springs, tethers and struts, one group per entry
    # (capi.solver_from_scene binds them after the bending entries, Solver.add_springs). Like
    # bending, unknown to the oracle and the reference driver. None = no springs, today's scene.
    springs: Optional[list] = None
    # ties: a list of (nodes_a (m, na) int32, w_a (m, na), nodes_b (m, nb) int32, w_b (m, nb), k (scalar
    # or (m,)), rest ((m,), scalar or None = the anchors' distances in rest_x), mode) -- springs between
    # barycentric anchors, one group per entry (capi.solver_from_scene binds them after the springs,
    # Solver.add_ties). Unknown to the oracle and the reference driver. None = no ties.
    ties: Optional[list] = None

    @property
    def rest_x(self) -> np.ndarray:
        return self.x if self.rest is None else self.rest

    @property
    def n_nodes(self) -> int:
        return int(self.x.shape[0])

    def n_elements(self) -> int:
        return int(sum(len(g.idx) for g in self.groups))


def per_element_groups(scene: Scene) -> Scene:
    """The equivalent scene with one one-element scalar group per element, in element order: the
    reference's layout (one EnergyTerm per element, each with its own Lame), which the reference
    driver and the oracle read. Uniform groups are expanded the same way."""
    groups = []
    for g in scene.groups:
        E, nu, lmin, lmax = g.material_arrays()
        idx = np.asarray(g.idx, np.int32)
        for e in range(len(idx)):
            groups.append(ElementGroup(g.kind, g.material, float(E[e]), float(nu[e]), idx[e:e + 1].copy(),
                                       float(lmin[e]), float(lmax[e])))
    return dataclasses.replace(scene, groups=groups)


def with_material_levels(scene: Scene, E_levels, nu_levels, lmin_levels=None, lmax_levels=None, seed=7) -> Scene:
    """The scene (a single group) with a random material level per element: level
    np.random.default_rng(seed).integers(0, L, n) of the given tables, as per-element arrays."""
    if len(scene.groups) != 1:
        raise ValueError("with_material_levels: the scene must have a single group")
    g = scene.groups[0]
    E_levels, nu_levels = np.asarray(E_levels, np.float64), np.asarray(nu_levels, np.float64)
    L = len(E_levels)
    if len(nu_levels) != L or any(t is not None and len(t) != L for t in (lmin_levels, lmax_levels)):
        raise ValueError("with_material_levels: the level tables must have one length")
    lvl = np.random.default_rng(seed).integers(0, L, len(g.idx))
    new = dataclasses.replace(
        g, E=E_levels[lvl], nu=nu_levels[lvl],
        limit_min=g.limit_min if lmin_levels is None else np.asarray(lmin_levels, np.float64)[lvl],
        limit_max=g.limit_max if lmax_levels is None else np.asarray(lmax_levels, np.float64)[lvl])
    return dataclasses.replace(scene, groups=[new])


# ----------------------------------------------------------------------------------------
# mesh generators
# ----------------------------------------------------------------------------------------

def tri_blocks(nx: int, ny: int):
    """Vertices (n,3) and triangles (4*nx*ny, 3) of make_tri_blocks(nx, ny)."""
    nx, ny = max(1, nx), max(1, ny)
    gx, gy = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    corners = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    cx, cy = np.meshgrid(np.arange(nx, dtype=np.float64) + 0.5, np.arange(ny, dtype=np.float64) + 0.5, indexing="ij")
    centres = np.stack([cx.ravel(), cy.ravel(), np.zeros(cx.size)], axis=1)
    verts = np.concatenate([corners, centres], axis=0)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    ix, iy = ix.ravel(), iy.ravel()          # cell order x-major, y-minor as in the reference loops
    corner = lambda i, j: i * (ny + 1) + j
    a = corner(ix, iy)
    b = corner(ix + 1, iy)
    c = corner(ix + 1, iy + 1)
    d = corner(ix, iy + 1)
    e = (nx + 1) * (ny + 1) + ix * ny + iy
    tris = np.stack([np.stack([d, a, e], 1), np.stack([a, b, e], 1),
                     np.stack([b, c, e], 1), np.stack([c, d, e], 1)], axis=1).reshape(-1, 3)
    return verts, tris.astype(np.int32)


def tri_grid(nx: int, ny: int, size: float = 1.0):
    """Vertices ((nx + 1)(ny + 1), 3) in the x-z plane, node j (nx + 1) + i at (i, 0, j) size / nx,
    and triangles (2 nx ny, 3): every cell (a b / c d) cut into (a, b, d) and (a, d, c), consistently
    oriented. 3 nx ny - nx - ny interior edges."""
    xs = np.linspace(0.0, size, nx + 1)
    zs = np.linspace(0.0, size * ny / nx, ny + 1)
    verts = np.array([[x, 0.0, z] for z in zs for x in xs], np.float64)
    tris = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c = a + 1, a + nx + 1
            d = c + 1
            tris += [[a, b, d], [a, d, c]]
    return verts, np.array(tris, np.int32)


def tet_blocks(cx: int, cy: int, cz: int):
    """Vertices (n,3) and tets (5*cx*cy*cz, 4) of make_tet_blocks(cx, cy, cz)."""
    cx, cy, cz = max(1, cx), max(1, cy), max(1, cz)
    g = np.stack(np.meshgrid(np.arange(cx + 1), np.arange(cy + 1), np.arange(cz + 1), indexing="ij"), -1)
    verts = g.reshape(-1, 3).astype(np.float64)
    node = lambda i, j, k: (i * (cy + 1) + j) * (cz + 1) + k
    X, Y, Z = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    X, Y, Z = X.ravel(), Y.ravel(), Z.ravel()
    a = node(X + 1, Y + 1, Z + 1)
    b = node(X, Y + 1, Z + 1)
    c = node(X, Y + 1, Z)
    d = node(X + 1, Y + 1, Z)
    e = node(X + 1, Y, Z + 1)
    f = node(X, Y, Z + 1)
    gg = node(X, Y, Z)
    h = node(X + 1, Y, Z)
    lab = [a, b, c, d, e, f, gg, h]
    table = [(0, 5, 7, 4), (5, 7, 2, 0), (5, 0, 2, 1), (7, 2, 0, 3), (5, 2, 7, 6)]
    tets = np.stack([np.stack([lab[t[0]], lab[t[1]], lab[t[2]], lab[t[3]]], 1) for t in table], 1).reshape(-1, 4)
    return verts, tets.astype(np.int32)


def tet_voxels(occ):
    """make_tet_blocks' 5 tets (same table, same corner labels) for every occupied cell of a
    boolean grid occ[x, y, z]; vertices = the lattice nodes the cells use (lattice units),
    numbered in lattice order. Cells in x-major, then y, then z order as in tet_blocks."""
    cx, cy, cz = occ.shape
    X, Y, Z = (a.astype(np.int64) for a in np.nonzero(occ))   # x-major order
    node = lambda i, j, k: (i * (cy + 1) + j) * (cz + 1) + k
    lab = [node(X + 1, Y + 1, Z + 1), node(X, Y + 1, Z + 1), node(X, Y + 1, Z), node(X + 1, Y + 1, Z),
           node(X + 1, Y, Z + 1), node(X, Y, Z + 1), node(X, Y, Z), node(X + 1, Y, Z)]
    table = [(0, 5, 7, 4), (5, 7, 2, 0), (5, 0, 2, 1), (7, 2, 0, 3), (5, 2, 7, 6)]
    tets = np.stack([np.stack([lab[t[0]], lab[t[1]], lab[t[2]], lab[t[3]]], 1) for t in table], 1).reshape(-1, 4)
    used = np.unique(tets)
    remap = np.full((cx + 1) * (cy + 1) * (cz + 1), -1, np.int64)
    remap[used] = np.arange(len(used))
    i, r = np.divmod(used, (cy + 1) * (cz + 1))
    j, k = np.divmod(r, cz + 1)
    verts = np.stack([i, j, k], 1).astype(np.float64)
    return verts, remap[tets].astype(np.int32)


def load_voxels(name):
    """Occupancy grid committed under aa-admm_amd/data (tools/make_bunny_voxels.py)."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name + ".npz"))
    dims = tuple(int(a) for a in d["dims"])
    return np.unpackbits(d["bits"])[:int(np.prod(dims))].reshape(dims).astype(bool)


def tri_masses(verts, tris, density=1.0):
    e1 = verts[tris[:, 1]] - verts[tris[:, 0]]
    e2 = verts[tris[:, 2]] - verts[tris[:, 0]]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    m = np.zeros(len(verts))
    for k in range(3):
        np.add.at(m, tris[:, k], density * area / 3.0)
    return m


def tet_masses(verts, tets, density=1522.0):
    B = np.stack([verts[tets[:, k]] - verts[tets[:, 0]] for k in (1, 2, 3)], axis=2)
    vol = np.abs(np.linalg.det(B)) / 6.0
    m = np.zeros(len(verts))
    for k in range(4):
        np.add.at(m, tets[:, k], density * vol / 4.0)
    return m


# ----------------------------------------------------------------------------------------
# the BASELINE.json scenes
# ----------------------------------------------------------------------------------------

def cloth(nx: int = 112, ny: int = 112, size: float = 2.0, *, variant=VARIANT_H, aa_m=6, iters=100,
          n_steps=1, accel=1, bend=None) -> Scene:
    """C2: cloth drop (`make_tri_blocks(112,112)` scaled to `size` m, 50 176 tris).
    bend: a bending stiffness k_bend for hinges on the sheet's interior edges (flat rest); None = the
    reference's pure membrane.

    Material Lame(50, 0.1) with strain limits [0.95, 1.05] and area density 1 as the
    windyflag sample (windyflag.cpp:84-87, AddMeshes.hpp:203); two corners of the min-x
    edge pinned in place (windyflag.cpp:29-61,101); wind omitted (out of scope).
    """
    v, t = tri_blocks(nx, ny)
    v = v * (size / max(nx, ny))
    m = tri_masses(v, t, 1.0)
    xmin = v[:, 0].min() + 1e-3 * size / max(nx, ny)
    cand = np.nonzero(v[:, 0] <= xmin)[0]
    up = cand[np.argmin(v[cand, 1])]
    down = cand[np.argmax(v[cand, 1])]
    pins = np.array([up, down], dtype=np.int32)
    return Scene(x=v, masses=m, groups=[ElementGroup(TRI, LINEAR, 50.0, 0.1, t, 0.95, 1.05)],
                 pin_idx=pins, pin_pts=v[pins].copy(), pin_vel=np.zeros((2, 3)), variant=variant,
                 iters=iters, aa_m=aa_m, n_steps=n_steps, accel=accel, name=f"cloth{nx}x{ny}",
                 bending=None if bend is None else [(t, float(bend), True)])


def cantilever_strip(nx=12, ny=12, k_bend=1e-2, *, flat_rest=True, size=0.1, clamp=True, membrane=True, iters=30, aa_m=6,
                     accel=1, n_steps=10, penalty=1.0) -> Scene:
    """Demo of the bending term: a tri_grid(nx, ny) strip of length `size` lying in the x-z plane
    under gravity, held at its x = 0 edge; cloth()'s membrane (Lame(50, 0.1), strain limits
    [0.95, 1.05], area density 1) plus hinges of stiffness k_bend on its interior edges ((u,x)
    variant). clamp: the next column of nodes is pinned too, which fixes the strip's slope at the
    edge -- a cantilever. Pinning the edge alone leaves a free hinge line: no hinge spans a boundary
    edge, so the strip turns about it at no cost (and, stiff, its tip falls faster than a limp
    strip's, as a rod's does). size: a strip of length L sags under its own weight once L^3 exceeds
    about k_bend / (density g), i.e. L = 0.05 for k_bend 1e-3 and 0.2 for 1e-1; the default 0.1 lies
    between, so that range of k_bend spans limp to stiff. k_bend None = no bending. membrane False =
    hinges only."""
    v, t = tri_grid(nx, ny, size)
    pins = np.nonzero(v[:, 0] <= (1.5 if clamp else 0.5) * size / nx)[0].astype(np.int32)
    return Scene(x=v, masses=tri_masses(v, t, 1.0),
                 groups=[ElementGroup(TRI, LINEAR, 50.0, 0.1, t, 0.95, 1.05)] if membrane else [],
                 pin_idx=pins, pin_pts=v[pins].copy(), pin_vel=np.zeros((len(pins), 3)), variant=VARIANT_H,
                 iters=iters, aa_m=aa_m, n_steps=n_steps, accel=accel, penalty=penalty, name=f"cantilever_strip{nx}x{ny}",
                 bending=None if k_bend is None else [(t, float(k_bend), bool(flat_rest))])


# ----------------------------------------------------------------------------------------
# springs, tethers and struts (Scene.springs)
# ----------------------------------------------------------------------------------------

def pair_lengths(x, pairs):
    """|x[b] - x[a]| per pair, summed as the host builder does."""
    d = np.asarray(x, np.float64)[np.asarray(pairs)[:, 1]] - np.asarray(x, np.float64)[np.asarray(pairs)[:, 0]]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def net_pairs(nx: int, ny: int, shear=True):
    """Pairs (m, 2) int32 of an nx x ny grid of nodes, node j nx + i: the structural springs along
    the rows, then along the columns, then (shear) both diagonals of every cell."""
    node = lambda i, j: j * nx + i
    p = [(node(i, j), node(i + 1, j)) for j in range(ny) for i in range(nx - 1)]
    p += [(node(i, j), node(i, j + 1)) for j in range(ny - 1) for i in range(nx)]
    if shear:
        for j in range(ny - 1):
            for i in range(nx - 1):
                p += [(node(i, j), node(i + 1, j + 1)), (node(i + 1, j), node(i, j + 1))]
    return np.array(p, np.int32).reshape(-1, 2)


def spring_net(nx=5, ny=5, *, k=50.0, size=1.0, node_mass=0.01, mode=SPRING, rest_scale=None, shear=True, gravity=-9.8,
               iters=30, aa_m=6, accel=1, n_steps=5, penalty=1.0) -> Scene:
    """Demo of the spring term: a net of nx x ny nodes in the x-z plane, `size` wide, made of springs
    alone -- structural ones along the grid lines plus shear ones on the cells' diagonals, stiffness
    k -- its four corners pinned, under gravity ((u,x) variant). Rest lengths are the initial
    distances (derived by the solver), or rest_scale times them."""
    xs = np.linspace(0.0, size, nx)
    zs = np.linspace(0.0, size * (ny - 1) / max(1, nx - 1), ny)
    v = np.array([[x, 0.0, z] for z in zs for x in xs], np.float64)
    pairs = net_pairs(nx, ny, shear)
    pins = np.array([0, nx - 1, (ny - 1) * nx, ny * nx - 1], np.int32)
    rest = None if rest_scale is None else float(rest_scale) * pair_lengths(v, pairs)
    return Scene(x=v, masses=np.full(len(v), float(node_mass)), groups=[], pin_idx=pins, pin_pts=v[pins].copy(),
                 pin_vel=np.zeros((4, 3)), variant=VARIANT_H, gravity=gravity, iters=iters, aa_m=aa_m, accel=accel,
                 n_steps=n_steps, penalty=penalty, name=f"spring_net{nx}x{ny}", springs=[(pairs, float(k), rest, int(mode))])


def stitched_panels(n=4, *, gap=0.05, k=20.0, bend=1e-2, size=0.5, iters=30, aa_m=6, accel=1, n_steps=3) -> Scene:
    """Demo of a seam: two tri_grid(n, n) cloth panels of side `size` side by side in the x-z plane,
    `gap` apart, cloth()'s membrane and hinges of stiffness `bend` on each, sewn along the facing
    edges by zero-length springs of stiffness k (stitches); the far edge of the first panel is held
    by its two corners. Springs, triangles and hinges in one solver."""
    v, t = tri_grid(n, n, size)
    nv = len(v)
    x = np.concatenate([v, v + np.array([size + gap, 0.0, 0.0])])
    tris = np.concatenate([t, t + nv]).astype(np.int32)
    pairs = np.array([[j * (n + 1) + n, nv + j * (n + 1)] for j in range(n + 1)], np.int32)
    pins = np.array([0, n * (n + 1)], np.int32)
    return Scene(x=x, masses=tri_masses(x, tris, 1.0), groups=[ElementGroup(TRI, LINEAR, 50.0, 0.1, tris, 0.95, 1.05)],
                 pin_idx=pins, pin_pts=x[pins].copy(), pin_vel=np.zeros((2, 3)), variant=VARIANT_H, iters=iters, aa_m=aa_m,
                 accel=accel, n_steps=n_steps, name="stitched_panels",
                 bending=None if bend is None else [(tris, float(bend), True)],
                 springs=[(pairs, float(k), np.zeros(len(pairs)), SPRING)])


def tethered_cloth(nx=8, ny=8, *, k=50.0, size=1.0, slack=0.02, pull=0.06, obstacle=True, collide_radius=0.25, friction=0.5, drop=0.03, iters=30, aa_m=6,
                   accel=1, n_steps=8, bend=None) -> Scene:
    """Demo of long-range attachments: a tri_grid(nx, ny) cloth (cloth()'s membrane) in the x-z
    plane, its x = 0 edge pinned, with one hard tether (SPRING_HARD | SPRING_TETHER, weight sqrt(k))
    from every pinned node straight across to the free edge, (1 + slack) times as long as the cloth
    is wide: the free edge cannot move further from the pinned one than that however the soft
    membrane stretches (its own strain limit is 1.05). pull: the sheet starts pulled out along x,
    by nothing at its z = 0 side and by `pull` at the other (the rest shape is the square sheet), so
    the tethers on that side are taut from the first iteration and the others slack. obstacle: a
    torus (mesh obstacle, Coulomb coefficient `friction`, contacts recorded) lies `drop` under the
    sheet and catches it as it swings down. collide_radius: the collision-checked nodes are those
    within this distance (times size, in the rest sheet) of the torus' axis -- the patch that
    reaches the tube first; None = every free node. A collision term carries the reference's weight
    sqrt(2 k_soft_rubber) = 5.7e3 whether it touches or not, against the tethers' sqrt(k) = 7: with
    all 72 free nodes checked 30 iterations leave comb at 1e-1 and a taut tether 4 to 10 % long (200
    iterations: 7 %), with the default patch of 10 nodes 3.5e-8."""
    rest, t = tri_grid(nx, ny, size)
    v = rest.copy()
    v[:, 0] *= 1.0 + pull * rest[:, 2] / rest[:, 2].max()
    pins = np.nonzero(v[:, 0] <= 0.5 * size / nx)[0].astype(np.int32)
    pairs = np.array([[j * (nx + 1), j * (nx + 1) + nx] for j in range(ny + 1)], np.int32)
    sc = Scene(x=v, masses=tri_masses(rest, t, 1.0), groups=[ElementGroup(TRI, LINEAR, 50.0, 0.1, t, 0.95, 1.05)],
               pin_idx=pins, pin_pts=v[pins].copy(), pin_vel=np.zeros((len(pins), 3)), variant=VARIANT_H, iters=iters,
               aa_m=aa_m, accel=accel, n_steps=n_steps, name="tethered_cloth", rest=rest,
               bending=None if bend is None else [(t, float(bend), True)],
               springs=[(pairs, float(k), (1.0 + slack) * pair_lengths(rest, pairs), SPRING_HARD | SPRING_TETHER)])
    if obstacle:
        R, r = 0.25 * size, 0.1 * size
        ctr = (0.6 * size, -(r + drop), 0.5 * size * ny / nx)
        sc.mesh_obstacles = [torus_mesh(16, 8, R, r, ctr)]
        near = np.setdiff1d(np.arange(sc.n_nodes, dtype=np.int32), pins).astype(np.int32)
        if collide_radius is not None:
            d = np.hypot(rest[near, 0] - ctr[0], rest[near, 2] - ctr[2])
            near = near[d < collide_radius * size]
        sc.collision_idx = near.astype(np.int32)
        sc.obstacle_friction = [float(friction)]
        sc.record_contacts = True
    return sc


def hanging_block(cells=(2, 2, 2), cell=0.2, material=LINEAR, *, E=1e5, nu=0.3, k=4000.0, hang=0.3, lift=(0.01, 0.005, 0.0),
                  iters=30, aa_m=6, accel=1, n_steps=6) -> Scene:
    """Demo of the soft attachment: a tet block (kuhn_tet_blocks, `material`) hanging by four springs
    of stiffness k from its top corners to four anchor nodes `hang` above them. The anchors are extra
    nodes in no element, pinned, and move by `lift` per step (pin_vel, i.e. set_pins every step): a
    handle of finite stiffness that drags the body. Block nodes come first, then the anchors."""
    bv, bt = kuhn_tet_blocks(*cells)
    bv = bv * float(cell)
    nb = len(bv)
    top, lo, hi = bv[:, 1].max(), bv.min(0), bv.max(0)
    corners = [int(np.argmin(np.abs(bv - np.array([cx, top, cz])).sum(1))) for cx in (lo[0], hi[0]) for cz in (lo[2], hi[2])]
    anchors = bv[corners] + np.array([0.0, hang, 0.0])
    x = np.concatenate([bv, anchors])
    pins = np.arange(nb, nb + 4, dtype=np.int32)
    pairs = np.array([[nb + i, c] for i, c in enumerate(corners)], np.int32)
    return Scene(x=x, masses=np.concatenate([tet_masses(bv, bt, 1522.0), np.ones(4)]),
                 groups=[ElementGroup(TET, int(material), E, nu, bt)], pin_idx=pins, pin_pts=anchors.copy(),
                 pin_vel=np.tile(np.asarray(lift, np.float64), (4, 1)), variant=VARIANT_H, iters=iters, aa_m=aa_m,
                 accel=accel, n_steps=n_steps, name="hanging_block", springs=[(pairs, float(k), None, SPRING)])


# ----------------------------------------------------------------------------------------
# ties: springs between barycentric anchors (Scene.ties)
# ----------------------------------------------------------------------------------------

def tri_barycentric(A, B, C, P):
    """Barycentric weights (n, 3) of the points P on the triangles (A, B, C), all (n, 3): Cramer's rule
    on the edge Gram matrix, the statement of the solver's closest-point query."""
    d3 = lambda u, w: (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
    e1, e2, d = B - A, C - A, P - A
    d11, d12, d22, p1, p2 = d3(e1, e1), d3(e1, e2), d3(e2, e2), d3(d, e1), d3(d, e2)
    den = d11 * d22 - d12 * d12
    b1 = (d22 * p1 - d12 * p2) / den
    b2 = (d11 * p2 - d12 * p1) / den
    return np.stack([(1.0 - b1) - b2, b1, b2], 1)


def closest_on_surface(V, F, Q):
    """Where the points Q (n, 3) land on the triangle list (V, F), on the host: (closest points (n, 3),
    triangle (n,), barycentric weights (n, 3)). Every triangle is tested (geom_report's Ericson
    test); among equally close ones the lowest index wins. For scene builders: capi.closest_on_triangles
    answers the same question on the device."""
    from .geom_report import closest_on_triangles
    V, F, Q = np.asarray(V, np.float64), np.asarray(F, np.int64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    c, tri = np.zeros_like(Q), np.zeros(len(Q), np.int32)
    for i, q in enumerate(Q):
        cl = closest_on_triangles(np.broadcast_to(q, A.shape).copy(), A, B, C)
        t = int(np.argmin(((cl - q) ** 2).sum(1)))
        c[i], tri[i] = cl[t], t
    return c, tri, tri_barycentric(A[tri], B[tri], C[tri], c)


def sewn_panels_offset(n=4, *, gap=0.04, shift=0.37, inset=0.3, stitches=7, k=20.0, bend=None, size=0.5, iters=30, aa_m=6,
                       accel=1, n_steps=3) -> Scene:
    """Demo of a seam between panels whose nodes do not line up: two tri_grid(n, n) cloth panels of
    side `size` side by side in the x-z plane, `gap` apart, the second slid along the seam by
    `shift` cells, so that no node of one faces a node of the other. `stitches` zero-length
    triangle-triangle ties (na = nb = 3) of stiffness k sew them: stitch i joins the point `inset`
    cells inside the first panel's seam edge to the point as far inside the second's, at the same
    height along the stretch of the seam that both panels cover; each point's triangle and weights
    come from closest_on_surface. cloth()'s membrane on both; the far edge of the first panel is
    held by its two corners."""
    v, t = tri_grid(n, n, size)
    nv, h = len(v), size / n
    x = np.concatenate([v, v + np.array([size + gap, 0.0, shift * h])])
    tris = np.concatenate([t, t + nv]).astype(np.int32)
    zs = np.linspace(shift * h + 0.11 * h, size - 0.13 * h, stitches)
    pa = np.stack([np.full(stitches, size - inset * h), np.zeros(stitches), zs], 1)
    pb = np.stack([np.full(stitches, size + gap + inset * h), np.zeros(stitches), zs], 1)
    _, ta, wa = closest_on_surface(x, tris[:len(t)], pa)
    _, tb, wb = closest_on_surface(x, tris[len(t):], pb)
    pins = np.array([0, n * (n + 1)], np.int32)
    return Scene(x=x, masses=tri_masses(x, tris, 1.0), groups=[ElementGroup(TRI, LINEAR, 50.0, 0.1, tris, 0.95, 1.05)],
                 pin_idx=pins, pin_pts=x[pins].copy(), pin_vel=np.zeros((2, 3)), variant=VARIANT_H, iters=iters, aa_m=aa_m,
                 accel=accel, n_steps=n_steps, name="sewn_panels_offset",
                 bending=None if bend is None else [(tris, float(bend), True)],
                 ties=[(tris[:len(t)][ta], wa, tris[len(t):][tb], wb, float(k), np.zeros(stitches), SPRING)])


def patch_on_block(cells=(2, 2, 2), cell=0.2, *, n=4, lift=0.03, k=200.0, mode=SPRING, rest=None, E=5e4, nu=0.3, floor=True,
                   friction=0.5, drop=0.0, iters=30, aa_m=6, accel=1, n_steps=4) -> Scene:
    """Demo of sewing a patch onto a body: a tet block (kuhn_tet_blocks, linear) and a tri_grid(n, n)
    cloth patch, 0.7 of the block's top face wide, `lift` above it. Every rim node of the patch is
    tied (node-triangle, na = 3, nb = 1, stiffness k, `mode`) to the point of the block's boundary
    triangles it lies over -- closest_on_surface on the block's faces; rest = None: the distance at
    the start. The patch shares no node with the block. floor: the block stands `drop` above a
    FLOOR at y = 0 (obstacle row 0, Coulomb coefficient `friction`, contacts recorded), its bottom
    nodes collision-checked. Block nodes come first, then the patch's."""
    bv, bt = kuhn_tet_blocks(*cells)
    bv = bv * float(cell) + np.array([0.0, drop, 0.0])
    nb = len(bv)
    faces = tet_boundary_faces(bv, bt)
    lo, hi = bv.min(0), bv.max(0)
    side = 0.7 * min(hi[0] - lo[0], hi[2] - lo[2])
    pv, pt = tri_grid(n, n, side)
    # off the block's own lattice lines, so that no rim node lies over an edge of a face
    pv = pv + np.array([0.5 * (lo[0] + hi[0]) - 0.5 * side + 0.013 * cell, hi[1] + lift, 0.5 * (lo[2] + hi[2]) - 0.5 * side + 0.007 * cell])
    x = np.concatenate([bv, pv])
    g = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    rim = np.unique(np.concatenate([g[0], g[-1], g[:, 0], g[:, -1]])).astype(np.int32)
    _, tri, w = closest_on_surface(bv, faces, pv[rim])
    ptris = (pt + nb).astype(np.int32)
    sc = Scene(x=x, masses=np.concatenate([tet_masses(bv, bt, 1522.0), tri_masses(pv, pt, 1.0)]),
               groups=[ElementGroup(TET, LINEAR, E, nu, bt), ElementGroup(TRI, LINEAR, 50.0, 0.1, ptris, 0.95, 1.05)],
               pin_idx=np.zeros(0, np.int32), pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=VARIANT_H,
               iters=iters, aa_m=aa_m, accel=accel, n_steps=n_steps, name="patch_on_block",
               ties=[(faces[tri].astype(np.int32), w, (rim + nb).reshape(-1, 1).astype(np.int32), np.ones((len(rim), 1)),
                      float(k), rest, int(mode))])
    if floor:
        sc.obstacles = [(OBS_FLOOR, (0.0,))]
        sc.collision_idx = np.nonzero(bv[:, 1] < lo[1] + 1e-3 * cell)[0].astype(np.int32)
        sc.obstacle_friction = [float(friction)]
        sc.record_contacts = True
    return sc


def cantilever(cx=20, cy=4, cz=5, material=NEOHOOKEAN, *, variant=VARIANT_X, aa_m=6, iters=50,
               n_steps=1, accel=1, E=1e7, nu=0.399) -> Scene:
    """C1: single cantilever `make_tet_blocks(20,4,5)` scaled 1/cy, x = 0 face pinned."""
    v, t = tet_blocks(cx, cy, cz)
    v = v / float(cy)
    m = tet_masses(v, t, 1522.0)
    pins = np.nonzero(v[:, 0] < v[:, 0].min() + 1e-3)[0].astype(np.int32)
    return Scene(x=v, masses=m, groups=[ElementGroup(TET, material, E, nu, t)],
                 pin_idx=pins, pin_pts=v[pins].copy(), pin_vel=np.zeros((len(pins), 3)), variant=variant,
                 iters=iters, aa_m=aa_m, n_steps=n_steps, accel=accel, name=f"cantilever{cx}x{cy}x{cz}")


def tet_drop(cx=100, cy=40, cz=50, material=NEOHOOKEAN, *, squash=0.9, variant=VARIANT_X, aa_m=6, iters=100,
             n_steps=1, accel=1, E=1e7, nu=0.399) -> Scene:
    """C4: elastic block free fall, `make_tet_blocks(cx, cy, cz)` (5 tets per cube; 100x40x50 =
    1 000 000 tets, 211 191 nodes) scaled by 1/cy, density 1522, NeoHookean Lame(1e7, 0.399).
    No pins, no collisions; the initial pose is the rest shape squashed to `squash` in y so that
    the elastic prox has work (a rigid free fall converges trivially) -- SURVEY.md §8d C4.
    The z-AA (X) order, as BASELINE.json asks (the (u,x) order goes NaN on large-deformation
    NeoHookean scenes)."""
    v, t = tet_blocks(cx, cy, cz)
    v = v / float(cy)
    m = tet_masses(v, t, 1522.0)
    x = v.copy()
    c = 0.5 * (v[:, 1].min() + v[:, 1].max())
    x[:, 1] = c + squash * (v[:, 1] - c)
    return Scene(x=x, masses=m, groups=[ElementGroup(TET, material, E, nu, t)], pin_idx=np.zeros(0, np.int32),
                 pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=variant, iters=iters, aa_m=aa_m,
                 n_steps=n_steps, accel=accel, name=f"drop{cx}x{cy}x{cz}", rest=v)


def bunny_drop(res=100, material=NEOHOOKEAN, *, cell=1.0 / 40.0, squash=0.9, variant=VARIANT_X, aa_m=6, iters=100,
               n_steps=1, accel=1, E=1e7, nu=0.399) -> Scene:
    """C4 on the mesh BASELINE configs[3] names: the reference's closed bunny
    (deps/mclscene/src/data/bunny_closed.obj) voxelised into `res` cells along its longest side
    (aa-admm_amd/data/bunny_vox<res>.npz; res 100 = 200 556 cells = 1 002 780 tets), 5
    make_tet_blocks tets per cell of size `cell` (the C4 block's 1/40 m), then the tet_drop
    recipe: NeoHookean Lame(1e7, 0.399), density 1522, free fall from the rest shape squashed to
    `squash` in y, z-AA (X order). An irregular, boundary-heavy mesh beside the regular block."""
    v, t = tet_voxels(load_voxels(f"bunny_vox{res}"))
    v = v * cell
    m = tet_masses(v, t, 1522.0)
    x = v.copy()
    c = 0.5 * (v[:, 1].min() + v[:, 1].max())
    x[:, 1] = c + squash * (v[:, 1] - c)
    return Scene(x=x, masses=m, groups=[ElementGroup(TET, material, E, nu, t)], pin_idx=np.zeros(0, np.int32),
                 pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=variant, iters=iters, aa_m=aa_m,
                 n_steps=n_steps, accel=accel, name=f"bunny{res}", rest=v)


def beams(dim=3, *, variant=VARIANT_X, aa_m=6, iters=100, n_steps=1, accel=1, materials=(LINEAR, NEOHOOKEAN, STVK)) -> Scene:
    """C1 beams: three make_tet_blocks(4*dim, dim, dim) beams, 1 m tall, at y = +1.75 / 0 / -1.75,
    Lame(1e7, 0.399), x-extreme faces pinned and pulled apart by dt per step
    (samples/Asia2019/beams.cpp:94-167 and its stretch_beams callback)."""
    xs, groups, pins, pts, vel = [], [], [], [], []
    off = 0
    dt = 1.0 / 30.0
    for i, mat in enumerate(materials):
        v, t = tet_blocks(4 * dim, dim, dim)
        lo, hi = v.min(0), v.max(0)
        v = (v - 0.5 * (lo + hi)) / (hi[1] - lo[1])
        v[:, 1] += (1.75, 0.0, -1.75)[i % 3]
        bl, bh = v[:, 0].min() + 1e-2, v[:, 0].max() - 1e-2
        for j in range(len(v)):
            if v[j, 0] < bl:
                pins.append(off + j); pts.append(v[j] - [dt, 0, 0]); vel.append([-dt, 0, 0])
            if v[j, 0] > bh:
                pins.append(off + j); pts.append(v[j] + [dt, 0, 0]); vel.append([dt, 0, 0])
        groups.append(ElementGroup(TET, mat, 1e7, 0.399, t + off))
        xs.append(v)
        off += len(v)
    x = np.concatenate(xs)
    m = np.concatenate([tet_masses(xs[i], groups[i].idx - sum(len(xx) for xx in xs[:i])) for i in range(len(xs))])
    return Scene(x=x, masses=m, groups=groups, pin_idx=np.array(pins, np.int32), pin_pts=np.array(pts),
                 pin_vel=np.array(vel), variant=variant, iters=iters, aa_m=aa_m, n_steps=n_steps, accel=accel,
                 name=f"beams{dim}")


# ----------------------------------------------------------------------------------------
# tet-mesh files and the sample binding (f2)
# ----------------------------------------------------------------------------------------

def load_elenode(path: str):
    """mcl::meshio::load_elenode (deps/mclscene/include/MCL/MeshIO.hpp:180-290): `path`.ele and
    `path`.node (TetGen format); 1-based files are detected from the first record's index, as the
    reference does. Vertices come back as float32 (mcl::TetMesh stores Vec3f), tets as int32."""
    def records(fname):
        with open(fname) as f:
            lines = [ln.split("#", 1)[0].split() for ln in f]
        lines = [ln for ln in lines if ln]
        return int(lines[0][0]), lines[1:]
    n_tets, rows = records(path + ".ele")
    tets = np.zeros((n_tets, 4), np.int32)
    seen = np.zeros(n_tets, bool)
    one = False
    for i, r in enumerate(rows[:n_tets]):
        idx, ids = int(r[0]), [int(v) for v in r[1:5]]
        if i == 0 and idx == 1:
            one = True
        if one:
            idx -= 1
            ids = [v - 1 for v in ids]
        if idx >= n_tets:
            raise ValueError("**TetMesh Error: Your indices are bad for file " + path + ".ele")
        tets[idx] = ids
        seen[idx] = True
    if not seen.all():
        raise ValueError("**TetMesh Error: Your indices are bad for file " + path + ".ele")
    n_nodes, rows = records(path + ".node")
    verts = np.zeros((n_nodes, 3), np.float32)
    seen = np.zeros(n_nodes, bool)
    one = False
    for i, r in enumerate(rows[:n_nodes]):
        idx = int(r[0])
        if i == 0 and idx == 1:
            one = True
        if one:
            idx -= 1
        if idx >= n_nodes:
            raise ValueError("**TetMesh Error: Your indices are bad for file " + path + ".node")
        verts[idx] = np.array([float(r[1]), float(r[2]), float(r[3])], np.float64).astype(np.float32)
        seen[idx] = True
    if not seen.all():
        raise ValueError("**TetMesh Error: Your indices are bad for file " + path + ".node")
    return verts, tets


def xform_scale_trans(verts32: np.ndarray, scale, trans) -> np.ndarray:
    """mesh->apply_xform(make_trans(t) * make_scale(s)) in float32 (mcl::XForm<float>): v' = s v + t."""
    s = np.asarray(scale, np.float32).reshape(1, 3)
    t = np.asarray(trans, np.float32).reshape(1, 3)
    return (verts32.astype(np.float32) * s + t).astype(np.float32)


def tetmesh_masses32(verts32: np.ndarray, tets: np.ndarray, density: float = 1522.0) -> np.ndarray:
    """TetMesh::weighted_masses (TetMesh.hpp:297-315) in float32, tets in order: |det(E)/6| * density / 4
    added to each corner, det of the edge matrix by Eigen's 3x3 cofactor expansion."""
    v = verts32.astype(np.float32)
    m = np.zeros(len(v), np.float32)
    dens = np.float32(density)
    six, four = np.float32(6.0), np.float32(4.0)
    e1 = v[tets[:, 1]] - v[tets[:, 0]]
    e2 = v[tets[:, 2]] - v[tets[:, 0]]
    e3 = v[tets[:, 3]] - v[tets[:, 0]]
    # columns are the edges: m(r, c) = e_c[r]
    m00, m10, m20 = e1[:, 0], e1[:, 1], e1[:, 2]
    m01, m11, m21 = e2[:, 0], e2[:, 1], e2[:, 2]
    m02, m12, m22 = e3[:, 0], e3[:, 1], e3[:, 2]
    # Eigen determinant_impl<3>: first-row expansion (Eigen/src/LU/Determinant.h)
    det = (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20)
    tm = (dens * np.abs(det / six)).astype(np.float32) / four
    for t in range(len(tets)):          # float accumulation in tet order
        for a in range(4):
            m[tets[t, a]] = np.float32(m[tets[t, a]] + tm[t])
    return m


def tetmesh_scene(verts32, tets, material=LINEAR, E=1e7, nu=0.499, **kw) -> Scene:
    """binding::add_tetmesh (samples/utils/AddMeshes.hpp:97-178) for one mesh: positions and the
    element rest shape are the float32 vertices (create_tets_from_mesh<float, ...>), masses
    TetMesh::weighted_masses(1522) per node x3 (zero mass throws, as the binding does)."""
    m = tetmesh_masses32(verts32, tets)
    if np.any(m <= 0):
        raise ValueError("TetMesh Error: Zero mass")
    x = verts32.astype(np.float64)
    return Scene(x=x, masses=m.astype(np.float64), groups=[ElementGroup(TET, material, E, nu, np.asarray(tets, np.int32))],
                 pin_idx=np.zeros(0, np.int32), pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), **kw)


# ----------------------------------------------------------------------------------------
# collision / wind scenes of the (u,x) variant (samples/Asia2019/plinko*.cpp, windyflag.cpp)
# ----------------------------------------------------------------------------------------

def plinko_hit(verts32, tets, *, y0=-1.0, iters=13, accel=0, aa_m=2, n_steps=20, dt=1.0 / 30.0, squash=0.95) -> Scene:
    """plinkohit.cpp:39-103: a linear-rubber tet mesh (Lame::rubber, `binding::LINEAR`) scaled by 13
    and moved to (0.25, y0, 0), dropped on PlaneAndHalfSphere(center (0,-3,0), radius 1) with every
    node collision-checked; admm_iters 13 and the other Solver::Settings defaults (dt 1/30, no
    acceleration, m = 2). y0 = 2.5 in the sample; lower here so contact starts within a few steps.
    The initial pose is the rest shape squashed to `squash` in y (rest kept for the elements), so
    the residuals carry signal before the first contact (an unstressed free fall is all rounding
    noise, which Anderson mixing then amplifies differently from run to run of any two codes)."""
    v = xform_scale_trans(verts32, (13.0, 13.0, 13.0), (0.25, y0, 0.0))
    sc = tetmesh_scene(v, tets, LINEAR, 10000000.0, 0.499, variant=VARIANT_H, iters=iters, accel=accel, aa_m=aa_m,
                       n_steps=n_steps, dt=dt, name="plinkohit")
    _squash(sc, squash)
    sc.obstacles = [(OBS_PLANE_HALF_SPHERE, (0.0, float(np.float32(-3.0)), 0.0, float(np.float32(1.0))))]
    sc.collision_idx = np.arange(sc.n_nodes, dtype=np.int32)
    return sc


def obstacle_course(verts32, tets, *, iters=15, accel=1, aa_m=5, n_steps=18, dt=1.0 / 30.0, squash=0.95) -> Scene:
    """Every PassiveObject.hpp shape at once under a falling rubber mesh (plinkopony.cpp:54-117
    uses Cylinder and SlideFloor, plinkohit PlaneAndHalfSphere): a sphere and two z-axis cylinders
    the mesh hits first, then a tilted SlideFloor, a Floor and a PlaneAndHalfSphere below."""
    v = xform_scale_trans(verts32, (13.0, 13.0, 13.0), (0.0, 0.2, 0.0))
    sc = tetmesh_scene(v, tets, LINEAR, 10000000.0, 0.499, variant=VARIANT_H, iters=iters, accel=accel, aa_m=aa_m,
                       n_steps=n_steps, dt=dt, name="obstacles")
    _squash(sc, squash)
    sc.obstacles = [
        (OBS_SPHERE, (0.3, -1.2, 0.1, 0.45)),
        (OBS_CYLINDER, (-0.6, -1.0, 0.0, 0.3)),
        (OBS_CYLINDER, (0.9, -1.4, 0.0, 0.25)),
        (OBS_SLIDE_FLOOR, (0.0, -2.0, 0.0, 0.5, 3.0 ** 0.5 / 2.0, 0.0)),
        (OBS_FLOOR, (-2.3,)),
        (OBS_PLANE_HALF_SPHERE, (0.2, -2.6, 0.0, 0.8)),
    ]
    sc.collision_idx = np.arange(sc.n_nodes, dtype=np.int32)
    return sc


def _squash(sc: Scene, f: float) -> None:
    """initial pose = rest squashed by f in y about its centre (tet_drop's recipe); rest unchanged"""
    if f == 1.0:
        return
    sc.rest = sc.x.copy()
    c = 0.5 * (sc.x[:, 1].min() + sc.x[:, 1].max())
    sc.x = sc.x.copy()
    sc.x[:, 1] = c + f * (sc.x[:, 1] - c)


def windy_cloth(nx=12, ny=12, *, iters=30, aa_m=6, accel=1, n_steps=3, direction=(25.0, 0.0, 5.0)) -> Scene:
    """windyflag.cpp:63-127 headless: the C2 cloth (two pinned corners) with a WindForce on all of
    its faces, direction = orig_wind (10, 0, 2) * 2.5."""
    sc = cloth(nx, ny, iters=iters, n_steps=n_steps, aa_m=aa_m, accel=accel)
    sc.winds = [(np.asarray(sc.groups[0].idx, np.int32), np.asarray(direction, np.float64))]
    sc.name = f"windycloth{nx}x{ny}"
    return sc


def tet_boundary_faces(verts, tets) -> np.ndarray:
    """(m, 3) boundary triangles of a tet mesh -- the faces used by exactly one tet -- oriented
    outward (away from the tet's fourth vertex), in tet order: what a solid tet mesh passes as a
    mesh obstacle."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    loc = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])
    faces = tets[:, loc].reshape(-1, 3)          # face k of a tet is opposite its vertex k
    opp = tets.reshape(-1)                        # ... which is opp[4 t + k]
    _, inv, cnt = np.unique(np.sort(faces, axis=1), axis=0, return_inverse=True, return_counts=True)
    keep = cnt[inv.reshape(-1)] == 1
    faces, opp = faces[keep], opp[keep]
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    inward = np.einsum("ij,ij->i", np.cross(b - a, c - a), verts[opp] - a) > 0
    faces[inward] = faces[inward][:, [0, 2, 1]]
    return faces.astype(np.int32)


def torus_mesh(nu=16, nv=8, R=1.0, r=0.4, center=(0.0, 0.0, 0.0)):
    """Closed torus surface around the y axis: nu x nv quads split in two, 2 nu nv triangles,
    oriented outward."""
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    U, Vv = np.meshgrid(u, v, indexing="ij")
    V = np.stack([(R + r * np.cos(Vv)) * np.cos(U), r * np.sin(Vv), (R + r * np.cos(Vv)) * np.sin(U)], axis=-1).reshape(-1, 3)
    V = V + np.asarray(center, np.float64)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    F = []
    for i in range(nu):
        for j in range(nv):
            p00, p10, p01, p11 = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            F += [(p00, p01, p11), (p00, p11, p10)]
    return V, np.asarray(F, np.int32)


def cloth_on_torus(nx=12, ny=12, *, iters=30, aa_m=6, accel=1, n_steps=10, drop=0.15, ring=0.3, bend=None) -> Scene:
    """Demo of the mesh obstacle: an unpinned cloth sheet dropped flat onto a torus lying in the
    x-z plane ((u,x) variant; every node collision-checked). The torus' major radius is `ring` times
    the sheet's side, its tube radius 0.4 of that. bend: cloth()'s."""
    sc = cloth(nx, ny, variant=VARIANT_H, aa_m=aa_m, iters=iters, n_steps=n_steps, accel=accel, bend=bend)
    sc.name = "cloth_on_torus"
    x = np.array(sc.x, np.float64)
    ext = x.max(0) - x.min(0)
    flat = np.argsort(ext)[0]                     # lay the sheet in the x-z plane
    if flat != 1:
        x[:, [flat, 1]] = x[:, [1, flat]]
    ctr = 0.5 * (x.max(0) + x.min(0))
    x = x - ctr
    R = ring * float(max(ext))
    r = 0.4 * R
    x[:, 1] = r + drop
    sc.x = x
    sc.pin_idx = np.zeros(0, np.int32)
    sc.pin_pts = np.zeros((0, 3))
    sc.pin_vel = np.zeros((0, 3))
    sc.mesh_obstacles = [torus_mesh(16, 8, R, r)]
    sc.collision_idx = np.arange(sc.n_nodes, dtype=np.int32)
    return sc


def rotation_y(angle: float) -> np.ndarray:
    """Rotation by `angle` about the y axis (3, 3)."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def cloth_on_spinning_torus(nx=12, ny=12, *, iters=30, aa_m=6, accel=1, n_steps=10, drop=0.15, dtheta=0.05,
                            friction=None, bend=None) -> Scene:
    """Demo of the kinematic mesh obstacle: cloth_on_torus with the torus turning about the y axis
    by `dtheta` per step (step k runs against the torus turned by k dtheta). friction: the torus'
    Coulomb coefficient -- with it the cloth is carried round; None = no friction pass."""
    sc = cloth_on_torus(nx, ny, iters=iters, aa_m=aa_m, accel=accel, n_steps=n_steps, drop=drop, bend=bend)
    sc.name = "cloth_on_spinning_torus"
    poses = np.zeros((n_steps, 1, 12))
    for k in range(n_steps):
        poses[k, 0, :9] = rotation_y((k + 1) * dtheta).reshape(9)
    sc.mesh_obstacle_poses = poses
    if friction is not None:
        sc.obstacle_friction = [friction]
    return sc


def cloth_on_breathing_torus(nx=12, ny=12, *, iters=30, aa_m=6, accel=1, n_steps=10, drop=0.15, amplitude=0.25,
                             period=20, ring=0.42, bend=None) -> Scene:
    """Demo of the deforming mesh obstacle: cloth_on_torus -- with a ring wide enough that the middle
    of the sheet's edges comes to lie on the tube while the corners hang free -- and the torus' tube
    radius oscillating, r_k = r (1 + amplitude sin^2(pi k / period)) in step k: never below the
    radius r the torus is added with, and at its largest in steps period / 2, 3 period / 2, ..."""
    sc = cloth_on_torus(nx, ny, iters=iters, aa_m=aa_m, accel=accel, n_steps=n_steps, drop=drop, ring=ring, bend=bend)
    sc.name = "cloth_on_breathing_torus"
    R = ring * float(max(sc.x.max(0) - sc.x.min(0)))
    r = 0.4 * R
    sc.mesh_obstacle_vertices = [[torus_mesh(16, 8, R, r * (1.0 + amplitude * np.sin(np.pi * k / period) ** 2))[0]]
                                 for k in range(1, n_steps + 1)]
    return sc


def kuhn_tet_blocks(cx: int, cy: int, cz: int):
    """Vertices (n, 3) (tet_blocks' lattice and numbering) and tets (6 cx cy cz, 4) of the Kuhn
    subdivision: every cube cut into the six tets around its main diagonal, one per order of the
    axes. Unlike make_tet_blocks' five tets it is conforming -- neighbouring cubes cut their shared
    face along the same diagonal -- so its boundary faces form a closed surface. Positive volumes."""
    import itertools
    g = np.stack(np.meshgrid(np.arange(cx + 1), np.arange(cy + 1), np.arange(cz + 1), indexing="ij"), -1)
    verts = g.reshape(-1, 3).astype(np.float64)
    node = lambda p: (p[:, 0] * (cy + 1) + p[:, 1]) * (cz + 1) + p[:, 2]
    cells = np.stack(np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij"), -1).reshape(-1, 3)
    tets = []
    for perm in itertools.permutations(range(3)):
        p = [cells]
        for a in perm:
            p.append(p[-1] + np.eye(3, dtype=cells.dtype)[a])
        t = np.stack([node(q) for q in p], 1)
        if np.linalg.det(np.eye(3)[list(perm)]) < 0:     # odd order of the axes: mirror image
            t = t[:, [0, 2, 1, 3]]
        tets.append(t)
    return verts, np.stack(tets, 1).reshape(-1, 4).astype(np.int32)


def cloth_on_soft_block(nx=12, ny=12, *, cells=(3, 2, 3), cell=0.3, E=5e4, nu=0.3, iters=30, aa_m=6, accel=1, n_steps=8,
                        drop=0.05, bend=None) -> Scene:
    """Demo of the bound mesh obstacle (body-to-body contact, (u,x) variant): a linear-tet block of
    `cells` cubes of side `cell` (kuhn_tet_blocks: conforming, so its boundary is closed), its bottom-face nodes pinned, soft enough to sag under its own
    weight over the steps; its boundary faces are mesh obstacle 0, bound to its surface nodes, so
    the obstacle follows the sagging block. An unpinned nx x ny cloth sheet, a little wider than the
    block, starts `drop` above the block's top face; its nodes are the collision nodes. Block nodes
    come first, then the cloth's."""
    bv, bt = kuhn_tet_blocks(*cells)
    bv = bv * float(cell)
    bm = tet_masses(bv, bt, 1522.0)
    side = 1.2 * cell * max(cells[0], cells[2])
    cv, ct = tri_blocks(nx, ny)
    cv = cv * (side / max(nx, ny))
    cm = tri_masses(cv, ct, 1.0)
    top = bv[:, 1].max()
    mid = 0.5 * (bv.max(0) + bv.min(0))
    cx = np.stack([cv[:, 0] - 0.5 * side + mid[0], np.full(len(cv), top + drop), cv[:, 1] - 0.5 * side + mid[2]], axis=1)
    nb = len(bv)
    x = np.concatenate([bv, cx], axis=0)
    rest = np.concatenate([bv, cv], axis=0)
    pins = np.nonzero(bv[:, 1] < bv[:, 1].min() + 1e-3 * cell)[0].astype(np.int32)
    faces = tet_boundary_faces(bv, bt)
    surf = np.unique(faces).astype(np.int32)           # the block's surface nodes, ascending
    local = np.full(nb, -1, np.int32)
    local[surf] = np.arange(len(surf), dtype=np.int32)
    sc = Scene(x=x, masses=np.concatenate([bm, cm]),
               groups=[ElementGroup(TET, LINEAR, E, nu, bt), ElementGroup(TRI, LINEAR, 50.0, 0.1, (ct + nb).astype(np.int32), 0.95, 1.05)],
               pin_idx=pins, pin_pts=bv[pins].copy(), pin_vel=np.zeros((len(pins), 3)), variant=VARIANT_H, iters=iters,
               aa_m=aa_m, n_steps=n_steps, accel=accel, name="cloth_on_soft_block", rest=rest)
    if bend is not None:   # hinges on the cloth sheet (rest shape: the flat sheet in `rest`)
        sc.bending = [((ct + nb).astype(np.int32), float(bend), True)]
    sc.mesh_obstacles = [(bv[surf].copy(), local[faces].astype(np.int32))]
    sc.mesh_obstacle_bindings = [surf]
    sc.collision_idx = np.arange(nb, nb + len(cx), dtype=np.int32)
    return sc


# ----------------------------------------------------------------------------------------
# friction scenes: a stiff linear tet block on a plane ((u,x) variant, its bottom nodes collision-checked)
# ----------------------------------------------------------------------------------------

def _block(cells, cell, E, nu):
    v, t = tet_blocks(*cells)
    v = v * float(cell)
    v = v - np.array([0.5 * (v[:, 0].max() + v[:, 0].min()), 0.0, 0.5 * (v[:, 2].max() + v[:, 2].min())])
    bottom = np.nonzero(v[:, 1] < 1e-3 * cell)[0].astype(np.int32)
    return v, t, tet_masses(v, t, 1522.0), bottom


def block_on_incline(theta_deg=20.0, friction=None, *, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40, aa_m=5,
                     accel=1, n_steps=40, dt=1.0 / 60.0, record=True, lift=0.0) -> Scene:
    """A block laid at rest on a SLIDE_FLOOR through the origin tilted by theta about z: the unit
    normal is (sin theta, cos theta, 0), downhill is (cos theta, -sin theta, 0). Without friction it
    slides at g sin theta; with the coefficient `friction` at g (sin theta - mu cos theta), and it
    stays where it is for mu > tan theta. Obstacle row 0. lift: the block starts that far above
    the plane (along the normal) instead of on it."""
    v, t, m, bottom = _block(cells, cell, E, nu)
    th = np.deg2rad(theta_deg)
    c, s = np.cos(th), np.sin(th)
    R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])   # e_x -> downhill, e_y -> the normal
    sc = Scene(x=v @ R.T + lift * R[:, 1], masses=m, groups=[ElementGroup(TET, LINEAR, E, nu, t)], pin_idx=np.zeros(0, np.int32),
               pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=VARIANT_H, dt=dt, iters=iters, aa_m=aa_m,
               n_steps=n_steps, accel=accel, name="block_on_incline", rest=v)
    sc.obstacles = [(OBS_SLIDE_FLOOR, (0.0, 0.0, 0.0, s, c, 0.0))] if theta_deg != 0.0 else [(OBS_FLOOR, (0.0,))]
    sc.collision_idx = bottom
    sc.obstacle_friction = None if friction is None else [friction]
    sc.record_contacts = record
    return sc


def block_on_moving_floor(friction=None, *, shift=0.01, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40, aa_m=5,
                          accel=1, n_steps=40, dt=1.0 / 60.0, record=True) -> Scene:
    """The block on a horizontal SLIDE_FLOOR whose centre moves by `shift` in x every step (step k
    runs against the centre at k shift). With friction the block is carried along; without it stays."""
    sc = block_on_incline(0.0, friction, cells=cells, cell=cell, E=E, nu=nu, iters=iters, aa_m=aa_m, accel=accel,
                          n_steps=n_steps, dt=dt, record=record)
    sc.name = "block_on_moving_floor"
    sc.obstacles = [(OBS_SLIDE_FLOOR, (0.0, 0.0, 0.0, 0.0, 1.0, 0.0))]
    sc.obstacle_motion = [[(k * shift, 0.0, 0.0, 0.0, 1.0, 0.0)] for k in range(1, n_steps + 1)]
    return sc


def block_on_turntable(friction=None, *, dtheta=0.01, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40, aa_m=5,
                       accel=1, n_steps=40, dt=1.0 / 60.0, record=True) -> Scene:
    """The block on a slab mesh (a box, its top face at y = 0) that turns about the y axis by
    `dtheta` per step through its pose (step k runs against the slab turned by k dtheta). With
    friction the block turns with the slab. Obstacle row 0 is the mesh."""
    sc = block_on_incline(0.0, None, cells=cells, cell=cell, E=E, nu=nu, iters=iters, aa_m=aa_m, accel=accel,
                          n_steps=n_steps, dt=dt, record=record)
    sc.name = "block_on_turntable"
    sc.obstacles = []
    ext = 2.0 * cell * max(cells[0], cells[2])
    V = np.array([[x, y, z] for x in (-ext, ext) for y in (-0.5 * ext, 0.0) for z in (-ext, ext)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # outward
    F = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)
    sc.mesh_obstacles = [(V, F)]
    poses = np.zeros((n_steps, 1, 12))
    for k in range(n_steps):
        poses[k, 0, :9] = rotation_y((k + 1) * dtheta).reshape(9)
    sc.mesh_obstacle_poses = poses
    sc.obstacle_friction = None if friction is None else [friction]
    return sc


def _slab(cells, cell):
    """block_on_turntable's slab: a box, its top face at y = 0."""
    ext = 2.0 * cell * max(cells[0], cells[2])
    V = np.array([[x, y, z] for x in (-ext, ext) for y in (-0.5 * ext, 0.0) for z in (-ext, ext)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # outward
    return V, np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)


def block_on_conveyor_mesh(friction=None, shift=0.01, *, carry=True, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40,
                           aa_m=5, accel=1, n_steps=40, dt=1.0 / 60.0, record=True) -> Scene:
    """The block on block_on_turntable's slab, every vertex of which is translated by `shift` in x
    per step through the vertex setter (step k runs against the slab moved by k shift): the motion of
    block_on_moving_floor expressed as a change of shape. With friction and carry the block is
    carried along; with carry off the pass takes the surface as standing still and the block is
    braked where it is. Obstacle row 0 is the mesh."""
    sc = block_on_incline(0.0, None, cells=cells, cell=cell, E=E, nu=nu, iters=iters, aa_m=aa_m, accel=accel,
                          n_steps=n_steps, dt=dt, record=record)
    sc.name = "block_on_conveyor_mesh"
    sc.obstacles = []
    V, F = _slab(cells, cell)
    sc.mesh_obstacles = [(V, F)]
    sc.mesh_obstacle_vertices = [[V + np.array([k * shift, 0.0, 0.0])] for k in range(1, n_steps + 1)]
    sc.mesh_obstacle_carry = [bool(carry)]
    sc.obstacle_friction = None if friction is None else [friction]
    return sc


def block_on_twisting_slab(friction=None, dtheta=0.01, *, carry=True, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40,
                           aa_m=5, accel=1, n_steps=40, dt=1.0 / 60.0, record=True) -> Scene:
    """block_on_turntable with the turn expressed through the vertex setter: step k runs against the
    slab's vertices rotated about y by k dtheta (rotation_y, as the turntable's pose)."""
    sc = block_on_conveyor_mesh(friction, 0.0, carry=carry, cells=cells, cell=cell, E=E, nu=nu, iters=iters, aa_m=aa_m,
                                accel=accel, n_steps=n_steps, dt=dt, record=record)
    sc.name = "block_on_twisting_slab"
    V = sc.mesh_obstacles[0][0]
    sc.mesh_obstacle_vertices = [[V @ rotation_y(k * dtheta).T] for k in range(1, n_steps + 1)]
    return sc


def block_on_sliding_block(friction=None, v0=0.6, *, carry=True, cells=(4, 2, 4), cell=0.25, E=1e7, nu=0.3, iters=40, aa_m=5,
                           accel=1, n_steps=40, dt=1.0 / 60.0, record=True, lower_cells=(8, 1, 8)) -> Scene:
    """Body on body: a stiff lower block (kuhn_tet_blocks, whose boundary is closed) resting on a
    FLOOR (row 0, mu = 0) and given the velocity v0 in x (Scene.initial_velocity, which the scene
    runner applies through set_v); its boundary faces are mesh obstacle 0 (row 1, the coefficient
    `friction`), bound to its surface nodes, which are exempt from it. The upper block (_block) lies
    at rest on the lower one's top face; its bottom nodes and the lower block's bottom nodes are the
    collision terms. With friction and carry the upper block rides along; with carry off it is
    braked against the world. Lower block nodes come first: they are mesh_obstacle_exempt[0]."""
    lv, lt = kuhn_tet_blocks(*lower_cells)
    lv = lv * float(cell)
    lv = lv - np.array([0.5 * lv[:, 0].max(), 0.0, 0.5 * lv[:, 2].max()])
    lm = tet_masses(lv, lt, 1522.0)
    top = lv[:, 1].max()
    uv, ut, um, ubottom = _block(cells, cell, E, nu)
    uv = uv + np.array([0.0, top, 0.0])
    nl = len(lv)
    faces = tet_boundary_faces(lv, lt)
    surf = np.unique(faces).astype(np.int32)
    local = np.full(nl, -1, np.int32)
    local[surf] = np.arange(len(surf), dtype=np.int32)
    lbottom = np.nonzero(lv[:, 1] < 1e-3 * cell)[0].astype(np.int32)
    x = np.concatenate([lv, uv], axis=0)
    sc = Scene(x=x, masses=np.concatenate([lm, um]),
               groups=[ElementGroup(TET, LINEAR, E, nu, lt), ElementGroup(TET, LINEAR, E, nu, (ut + nl).astype(np.int32))],
               pin_idx=np.zeros(0, np.int32), pin_pts=np.zeros((0, 3)), pin_vel=np.zeros((0, 3)), variant=VARIANT_H, dt=dt,
               iters=iters, aa_m=aa_m, n_steps=n_steps, accel=accel, name="block_on_sliding_block", rest=x.copy())
    sc.obstacles = [(OBS_FLOOR, (0.0,))]
    sc.mesh_obstacles = [(lv[surf].copy(), local[faces].astype(np.int32))]
    sc.mesh_obstacle_bindings = [surf]
    sc.mesh_obstacle_exempt = [np.arange(nl, dtype=np.int32)]
    sc.mesh_obstacle_carry = [bool(carry)]
    sc.collision_idx = np.concatenate([lbottom, ubottom + nl]).astype(np.int32)
    sc.obstacle_friction = None if friction is None else [0.0, friction]
    sc.record_contacts = record
    sc.initial_velocity = np.zeros_like(x)
    sc.initial_velocity[:nl, 0] = v0
    return sc
