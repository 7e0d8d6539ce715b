"""ctypes binding of libaa_admm.so (include/aa_admm.h) -- the Python host mirror of the
reference's admm::Solver API (admm_anderson_hard_zxu/src/Solver.hpp:39-262).

This is exactly the stub a maintainer would add on the Python side of the boundary
(INTEGRATION.md). There is no CPU fallback: if the HIP library is missing or no GPU is
visible, constructing a context raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AA_ADMM_LIB") or os.path.join(HERE, "libaa_admm.so")   # override: A/B builds

AA_LINEAR, AA_NEOHOOKEAN, AA_STVK = 0, 1, 2
AA_VARIANT_Z, AA_VARIANT_UX = 0, 1
AA_SPRING, AA_SPRING_TETHER, AA_SPRING_STRUT, AA_SPRING_HARD = 0, 1, 2, 4
NOACC, ANDERSON = 0, 1

EXPORTS = [
    "aa_last_error", "aa_version", "aa_ctx_create", "aa_ctx_destroy", "aa_ctx_synchronize", "aa_ctx_bench_read",
    "aa_ctx_warm_dense", "aa_lame_from_young",
    "aa_settings_default", "aa_elastic_create", "aa_elastic_destroy", "aa_elastic_add_nodes", "aa_elastic_add_tets",
    "aa_elastic_add_tris", "aa_elastic_add_tets_var", "aa_elastic_add_tris_var", "aa_elastic_add_bending", "aa_elastic_add_springs", "aa_elastic_add_ties", "aa_closest_on_triangles", "aa_elastic_set_pins", "aa_elastic_initialize", "aa_elastic_step",
    "aa_elastic_add_obstacle", "aa_elastic_add_mesh_obstacle", "aa_elastic_set_mesh_obstacle_pose",
    "aa_elastic_get_mesh_obstacle_pose", "aa_elastic_set_mesh_obstacle_vertices", "aa_elastic_get_mesh_obstacle_vertices",
    "aa_elastic_bind_mesh_obstacle", "aa_elastic_mesh_obstacle_status", "aa_elastic_set_mesh_obstacle_exempt",
    "aa_elastic_num_obstacles", "aa_elastic_set_obstacle", "aa_elastic_set_obstacle_friction", "aa_elastic_get_obstacle_friction",
    "aa_elastic_record_contacts", "aa_elastic_get_contacts", "aa_elastic_set_mesh_obstacle_carry", "aa_elastic_get_mesh_obstacle_carry",
    "aa_elastic_get_contact_features", "aa_elastic_set_collisions", "aa_elastic_add_wind", "aa_elastic_set_wind",
    "aa_elastic_num_nodes", "aa_elastic_get_x", "aa_elastic_get_v", "aa_elastic_set_v", "aa_elastic_get_history",
    "aa_elastic_get_times", "aa_elastic_set_iterations", "aa_elastic_set_x",
    "aa_elastic_runtime", "aa_elastic_bench_iterations", "aa_elastic_kernel_stats", "aa_elastic_local_stats",
    "aa_elastic_setup_phases",
    "aa_runtime_libraries", "aa_comm_unique_id", "aa_comm_create_rccl", "aa_comm_create_host", "aa_comm_create_solo", "aa_comm_destroy", "aa_comm_info",
    "aa_comm_allreduce_host", "aa_elastic_set_comm", "aa_geom_set_comm",
    "aa_geom_create", "aa_geom_create_kind", "aa_geom_destroy", "aa_geom_add_ref_surface", "aa_geom_add_constraints", "aa_geom_add_laplacian",
    "aa_geom_add_closeness", "aa_geom_add_laplacians", "aa_geom_add_closenesses", "aa_geom_setup", "aa_geom_solve", "aa_geom_set_stop", "aa_geom_get_solution", "aa_geom_get_history",
    "aa_geom_runtime_info", "aa_geom_closest_points", "aa_geom_bench_iterations", "aa_geom_kernel_stats",
    "aa_test_prox", "aa_test_cod_solve", "aa_test_geom_project", "aa_test_mesh_sdf", "aa_test_collision_prox",
    "aa_test_mesh_sdf_posed", "aa_test_collision_prox_posed", "aa_test_mesh_refit_tables", "aa_test_mesh_sdf_deformed", "aa_test_direct_solve",
    "aa_test_bound_refit", "aa_test_collision_prox_exempt", "aa_test_contact_friction", "aa_test_contact_friction_carry",
    "aa_test_anderson_step",
]

# Geometry constraint types (Geometry/Constraint.h) and SPD solver types (SolverCommon.h)
AA_CON_PLANE, AA_CON_ANGLE, AA_CON_EDGE, AA_CON_CLOSENESS, AA_CON_POINT_TO_REF, AA_CON_REF_SURFACE = range(6)
AA_SPD_LDLT, AA_SPD_LLT = 0, 1
AA_GEOM_ALM, AA_GEOM_PLAIN = 0, 1   # ALMGeometrySolver<3> / GeometrySolver<3>


class Lame(C.Structure):
    """admm::Lame (EnergyTerm.hpp:35-61)."""
    _fields_ = [("mu", C.c_double), ("lambda_", C.c_double), ("limit_min", C.c_double), ("limit_max", C.c_double)]

    @classmethod
    def from_young(cls, E, nu, limit_min=-100.0, limit_max=100.0):
        mu = E / (2.0 * (1.0 + nu))
        lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
        return cls(mu, lam, limit_min, limit_max)


class Settings(C.Structure):
    """admm::Solver::Settings (Solver.hpp:45-67) + the variant."""
    _fields_ = [("timestep_s", C.c_double), ("verbose", C.c_int), ("admm_iters", C.c_int), ("gravity", C.c_double),
                ("constraint_w", C.c_double), ("anderson_m", C.c_int), ("penalty", C.c_double),
                ("acceleration_type", C.c_int), ("variant", C.c_int), ("eps_rel", C.c_double)]

    def __init__(self, **kw):
        super().__init__(1.0 / 30.0, 1, 500, -9.8, -1.0, 2, 1.0, NOACC, AA_VARIANT_UX, 0.0)
        for k, v in kw.items():
            setattr(self, k, v)


class Runtime(C.Structure):
    _fields_ = [("global_ms", C.c_double), ("local_ms", C.c_double), ("acceleration_ms", C.c_double),
                ("initialization_ms", C.c_double), ("step_ms", C.c_double), ("setup_ms", C.c_double),
                ("iterations", C.c_int), ("rejects", C.c_int), ("nnz_factor", C.c_longlong), ("n_free", C.c_int),
                ("n_pinned", C.c_int), ("n_elements", C.c_int), ("z_dim", C.c_int)]


_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"aa_admm HIP library not built: {LIB_PATH} (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.aa_last_error.restype = C.c_char_p
        L.aa_version.restype = C.c_char_p
        _LIB = L
    return _LIB


RUNTIME_LIBS = ("amdhip64", "hsa-runtime64", "rocblas", "rocsolver", "rccl")


def runtime_libraries() -> dict:
    """{name: path} of the HIP / HSA / rocBLAS / rocSOLVER / RCCL objects this process has bound
    (aa_runtime_libraries, dladdr; loads librccl, needs no GPU)."""
    n = C.c_longlong()
    buf = C.create_string_buffer(4096)
    _chk(lib().aa_runtime_libraries(buf, C.c_longlong(len(buf)), C.byref(n)))
    out = {}
    for ln in buf.value.decode().splitlines():
        k, _, v = ln.partition("=")
        out[k] = v
    return out


def expected_runtime_dir() -> str:
    """The ROCm lib directory `ldd libaa_admm.so` resolves libamdhip64 to (the build's RUNPATH)."""
    import subprocess
    r = subprocess.run(["ldd", LIB_PATH], capture_output=True, text=True, check=True)
    for ln in r.stdout.splitlines():
        if "libamdhip64" in ln and "=>" in ln:
            return os.path.dirname(os.path.realpath(ln.split("=>")[1].split("(")[0].strip()))
    raise RuntimeError(f"ldd {LIB_PATH}: libamdhip64 not found")


def mapped_runtime_objects() -> dict:
    """{name: sorted real paths} of every mapped copy of the RUNTIME_LIBS (/proc/self/maps)."""
    out = {k: set() for k in RUNTIME_LIBS}
    with open("/proc/self/maps") as f:
        for ln in f:
            parts = ln.split()
            if len(parts) < 6 or not parts[5].startswith("/"):
                continue
            base = os.path.basename(parts[5])
            for k in RUNTIME_LIBS:
                if base.startswith("lib" + k + ".so"):
                    out[k].add(os.path.realpath(parts[5]))
    return {k: sorted(v) for k, v in out.items()}


def check_runtime() -> dict:
    """Fail unless every runtime object bound by this process (and every mapped copy of one) lives in
    the ROCm directory the library was linked against -- e.g. not a framework's bundled ROCm loaded
    before libaa_admm.so. Returns {"expected": dir, "bound": {...}, "mapped": {...}}."""
    want = expected_runtime_dir()
    bound = {k: os.path.realpath(v) if v else "" for k, v in runtime_libraries().items()}
    mapped = mapped_runtime_objects()
    bad = [f"{k} bound to {v or '(not loaded)'}" for k, v in bound.items() if os.path.dirname(v) != want]
    bad += [f"{k} mapped from {p}" for k, ps in mapped.items() for p in ps if os.path.dirname(p) != want]
    if bad:
        raise RuntimeError(f"libaa_admm.so was built against {want}, but this process uses: " + "; ".join(bad)
                           + " (load the library before any framework that bundles its own ROCm runtime)")
    return {"expected": want, "bound": bound, "mapped": mapped}


class AAError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _chk(rc):
    if rc != 0:
        raise AAError(rc, lib().aa_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(lib().aa_ctx_create(C.c_int(device), C.byref(self.h)))

    def bench_read(self, nbytes=1 << 30):
        """GB/s of a 16-B/lane streaming read of nbytes (aa_ctx_bench_read): the measured HBM ceiling."""
        g = C.c_double()
        _chk(lib().aa_ctx_bench_read(self.h, C.c_longlong(nbytes), C.byref(g)))
        return g.value

    def warm_dense(self):
        """Wall ms of the one-time rocBLAS / rocSOLVER code-object load (aa_ctx_warm_dense); 0 when warm."""
        ms = C.c_double()
        _chk(lib().aa_ctx_warm_dense(self.h, C.byref(ms)))
        return ms.value

    def synchronize(self):
        _chk(lib().aa_ctx_synchronize(self.h))

    def close(self):
        if self.h:
            lib().aa_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_longlong, C.c_void_p)


class Comm:
    """Communicator of the partitioned multi-GPU solver (aa_comm_*).

    Comm.rccl(ctx, rank, size, unique_id): RCCL over xGMI, one process per GPU.
    Comm.host(fn, rank, size): host-staged transport; fn(np.ndarray) sums the array in place
    over the ranks (e.g. torch.distributed over gloo) -- lets several ranks share one GPU.
    """

    def __init__(self, h, keep=None):
        self.h = h
        self._keep = keep

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        _chk(lib().aa_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def rccl(cls, ctx: Context, rank: int, size: int, unique_id: bytes):
        h = C.c_void_p()
        uid = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        _chk(lib().aa_comm_create_rccl(ctx.h, uid, C.c_int(rank), C.c_int(size), C.byref(h)))
        return cls(h)

    @classmethod
    def host(cls, fn, rank: int, size: int):
        def cb(buf, n, _user):
            try:
                fn(np.ctypeslib.as_array(buf, shape=(int(n),)))
                return 0
            except Exception:   # noqa: BLE001 -- reported to C as a failed reduction
                return 1
        cfn = HOST_ALLREDUCE_FN(cb)
        h = C.c_void_p()
        _chk(lib().aa_comm_create_host(cfn, None, C.c_int(rank), C.c_int(size), C.byref(h)))
        return cls(h, keep=cfn)

    @classmethod
    def solo(cls, rank: int, size: int):
        """Timing rehearsal: one rank of a size-way partition alone (aa_comm_create_solo)."""
        h = C.c_void_p()
        _chk(lib().aa_comm_create_solo(C.c_int(rank), C.c_int(size), C.byref(h)))
        return cls(h)

    def info(self):
        r, n = C.c_int(), C.c_int()
        _chk(lib().aa_comm_info(self.h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def allreduce_host(self, a):
        a = np.ascontiguousarray(a, np.float64)
        _chk(lib().aa_comm_allreduce_host(self.h, _dp(a), C.c_longlong(a.size)))
        return a

    def close(self):
        if self.h:
            lib().aa_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Solver:
    """Mirror of admm::Solver: add_nodes / create_*_from_mesh / set_pins / initialize / step."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.h = C.c_void_p()
        _chk(lib().aa_elastic_create(ctx.h, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().aa_elastic_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_nodes(self, x, m3):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        m3 = np.ascontiguousarray(m3, np.float64).reshape(-1)
        tot = C.c_int()
        _chk(lib().aa_elastic_add_nodes(self.h, _dp(x), _dp(m3), C.c_int(len(x) // 3), C.byref(tot)))
        return tot.value

    def add_tets(self, verts, tets, material, lame: Lame, vertex_offset=0):
        v = np.ascontiguousarray(verts, np.float64).reshape(-1)
        t = np.ascontiguousarray(tets, np.int32).reshape(-1)
        _chk(lib().aa_elastic_add_tets(self.h, _dp(v), _ip(t), C.c_int(len(t) // 4), C.c_int(material),
                                       C.byref(lame), C.c_int(vertex_offset)))

    def add_tris(self, verts, tris, lame: Lame, vertex_offset=0):
        v = np.ascontiguousarray(verts, np.float64).reshape(-1)
        t = np.ascontiguousarray(tris, np.int32).reshape(-1)
        _chk(lib().aa_elastic_add_tris(self.h, _dp(v), _ip(t), C.c_int(len(t) // 3), C.byref(lame),
                                       C.c_int(vertex_offset)))

    @staticmethod
    def _lame_array(n, mu, lam, limit_min=None, limit_max=None):
        """[n] aa_lame records from per-element arrays (scalars broadcast; limits default to Lame's)."""
        a = np.empty((n, 4), np.float64)
        a[:, 0] = mu
        a[:, 1] = lam
        a[:, 2] = -100.0 if limit_min is None else limit_min
        a[:, 3] = 100.0 if limit_max is None else limit_max
        return a

    def add_tets_var(self, verts, tets, material, mu, lam, vertex_offset=0):
        """One group of tets with per-element Lame parameters (aa_elastic_add_tets_var): mu, lam are
        arrays of the group's length -- the reference's loop of one-element create_tets_from_mesh calls."""
        v = np.ascontiguousarray(verts, np.float64).reshape(-1)
        t = np.ascontiguousarray(tets, np.int32).reshape(-1)
        la = self._lame_array(len(t) // 4, mu, lam)
        _chk(lib().aa_elastic_add_tets_var(self.h, _dp(v), _ip(t), C.c_int(len(t) // 4), C.c_int(material),
                                           la.ctypes.data_as(C.POINTER(Lame)), C.c_int(vertex_offset)))

    def add_tris_var(self, verts, tris, mu, lam, limit_min=None, limit_max=None, vertex_offset=0):
        """One group of triangles with per-element Lame parameters and strain limits (aa_elastic_add_tris_var)."""
        v = np.ascontiguousarray(verts, np.float64).reshape(-1)
        t = np.ascontiguousarray(tris, np.int32).reshape(-1)
        la = self._lame_array(len(t) // 3, mu, lam, limit_min, limit_max)
        _chk(lib().aa_elastic_add_tris_var(self.h, _dp(v), _ip(t), C.c_int(len(t) // 3),
                                           la.ctypes.data_as(C.POINTER(Lame)), C.c_int(vertex_offset)))

    def add_bending(self, verts, tris, k_bend, flat_rest=True, vertex_offset=0):
        """Bending hinges on the interior edges of a triangle list (aa_elastic_add_bending): rest
        shape verts[tris], stiffness k_bend; flat_rest False keeps the rest shape's curvature as the
        equilibrium. Before initialize. Returns the hinge count."""
        v = np.ascontiguousarray(verts, np.float64).reshape(-1)
        t = np.ascontiguousarray(tris, np.int32).reshape(-1)
        k = C.c_int()
        _chk(lib().aa_elastic_add_bending(self.h, _dp(v), _ip(t), C.c_int(len(t) // 3), C.c_double(k_bend),
                                          C.c_int(1 if flat_rest else 0), C.c_int(vertex_offset), C.byref(k)))
        return k.value

    def add_springs(self, pairs, k, rest=None, mode=AA_SPRING, verts=None, vertex_offset=0):
        """Two-node springs (aa_elastic_add_springs): pairs (n, 2), stiffness k (a scalar is broadcast),
        rest lengths rest (n,) or None = the pairs' distances in verts (default: the solver's current
        node positions). mode: AA_SPRING / AA_SPRING_TETHER / AA_SPRING_STRUT, | AA_SPRING_HARD.
        Before initialize."""
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1)
        n = len(p) // 2
        kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.float64), (n,)))
        r = None if rest is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rest, np.float64), (n,)))
        if verts is None and rest is None:
            verts = self.x
        v = None if verts is None else np.ascontiguousarray(verts, np.float64).reshape(-1)
        _chk(lib().aa_elastic_add_springs(self.h, None if v is None else _dp(v), _ip(p), C.c_int(n), C.c_int(int(mode)), _dp(kk),
                                          None if r is None else _dp(r), C.c_int(vertex_offset)))

    def add_ties(self, nodes_a, w_a, nodes_b, w_b, k, rest=None, mode=AA_SPRING, verts=None, vertex_offset=0):
        """Ties between barycentric anchors (aa_elastic_add_ties): nodes_a / w_a (n, na), nodes_b / w_b
        (n, nb), 1 <= na, nb <= 4 and 3 <= na + nb <= 6; anchor = sum of weight x node, weights used as
        given. Stiffness k (a scalar is broadcast), rest lengths rest (n,) or None = the anchors'
        distances in verts (default: the solver's current node positions). mode as for add_springs.
        Before initialize."""
        wa, wb = np.asarray(w_a, np.float64), np.asarray(w_b, np.float64)
        if wa.ndim != 2 or wb.ndim != 2 or len(wa) != len(wb):
            raise ValueError("add_ties: w_a (n, na) and w_b (n, nb) with the same n")
        n, na, nb = wa.shape[0], wa.shape[1], wb.shape[1]
        ia = np.ascontiguousarray(np.asarray(nodes_a, np.int32).reshape(n, na))
        ib = np.ascontiguousarray(np.asarray(nodes_b, np.int32).reshape(n, nb))
        wa, wb = np.ascontiguousarray(wa), np.ascontiguousarray(wb)
        kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.float64), (n,)))
        r = None if rest is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rest, np.float64), (n,)))
        if verts is None and rest is None:
            verts = self.x
        v = None if verts is None else np.ascontiguousarray(verts, np.float64).reshape(-1)
        _chk(lib().aa_elastic_add_ties(self.h, None if v is None else _dp(v), C.c_int(na), _ip(ia), _dp(wa), C.c_int(nb), _ip(ib),
                                       _dp(wb), C.c_int(n), C.c_int(int(mode)), _dp(kk), None if r is None else _dp(r),
                                       C.c_int(vertex_offset)))

    def set_pins(self, inds, points=None):
        i = np.ascontiguousarray(inds, np.int32).reshape(-1)
        if points is None:
            _chk(lib().aa_elastic_set_pins(self.h, _ip(i), None, C.c_int(len(i))))
        else:
            p = np.ascontiguousarray(points, np.float64).reshape(-1)
            _chk(lib().aa_elastic_set_pins(self.h, _ip(i), _dp(p), C.c_int(len(i))))

    def add_obstacle(self, kind, params):
        """Solver::add_obstacle with a PassiveObject.hpp shape (AA_OBS_*)."""
        p = np.zeros(8)
        q = np.asarray(params, np.float64).reshape(-1)
        p[:len(q)] = q
        _chk(lib().aa_elastic_add_obstacle(self.h, C.c_int(kind), _dp(p)))

    def add_mesh_obstacle(self, V, F):
        """PassiveMesh as a closed, outward-oriented triangle surface: vertices V (n, 3), triangles
        F (m, 3). Takes its place in add_obstacle's insertion order; returns the mesh's number."""
        v = np.ascontiguousarray(V, np.float64).reshape(-1)
        f = np.ascontiguousarray(F, np.int32).reshape(-1)
        k = C.c_int()
        _chk(lib().aa_elastic_add_mesh_obstacle(self.h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(len(f) // 3),
                                                C.byref(k)))
        return k.value

    def set_mesh_obstacle_pose(self, mesh_id, R=None, t=None):
        """A mesh obstacle's rigid pose for every later step: the surface seen is R v + t for the
        vertices v it was added with (R (3, 3) a rotation, used as given). R None: back to unposed.
        One table row is written; nothing is rebuilt and the captured step graph is kept."""
        if R is None:
            _chk(lib().aa_elastic_set_mesh_obstacle_pose(self.h, C.c_int(mesh_id), None))
            return
        _chk(lib().aa_elastic_set_mesh_obstacle_pose(self.h, C.c_int(mesh_id), _dp(pose12(R, t))))

    def mesh_obstacle_pose(self, mesh_id):
        """(R, t, posed) of a mesh obstacle: the pose in force (identity when unposed)."""
        p = np.zeros(12)
        posed = C.c_int()
        _chk(lib().aa_elastic_get_mesh_obstacle_pose(self.h, C.c_int(mesh_id), _dp(p), C.byref(posed)))
        return p[:9].reshape(3, 3).copy(), p[9:].copy(), bool(posed.value)

    def set_mesh_obstacle_vertices(self, mesh_id, V):
        """A deforming mesh obstacle: new positions V (n, 3) for the vertices it was added with (same
        count, same triangles, obstacle frame) for every later step. The BVH, the leaf triangles and
        the pseudonormals are refitted on the device; no row is taken, nothing is rebuilt and the
        captured step graph is kept. A refused V (non-finite, a zero-area triangle, a signed volume
        that is not positive) changes nothing."""
        n = self.mesh_obstacle_vertices(mesh_id, count_only=True)
        v = np.ascontiguousarray(V, np.float64).reshape(-1)
        if len(v) != 3 * n:
            raise AAError(-1, f"set_mesh_obstacle_vertices: {len(v) // 3} vertices given, the mesh has {n}")
        _chk(lib().aa_elastic_set_mesh_obstacle_vertices(self.h, C.c_int(mesh_id), _dp(v)))

    def mesh_obstacle_vertices(self, mesh_id, count_only=False):
        """The vertices (n, 3) of a mesh obstacle in force (count_only: just n)."""
        n = C.c_int()
        _chk(lib().aa_elastic_get_mesh_obstacle_vertices(self.h, C.c_int(mesh_id), None, C.byref(n)))
        if count_only:
            return n.value
        v = np.zeros((n.value, 3))
        _chk(lib().aa_elastic_get_mesh_obstacle_vertices(self.h, C.c_int(mesh_id), _dp(v), None))
        return v

    def bind_mesh_obstacle(self, mesh_id, nodes):
        """A bound mesh obstacle: vertex i of the mesh follows solver node nodes[i] (any node). Every
        later step starts by gathering the vertices from its start state on the device, checking the
        shape there and refitting; the obstacle holds that shape for the step's iterations. A shape
        that fails the check (mesh_obstacle_status) is skipped and the last good one stays.
        nodes None: unbind, the shape last in force stays."""
        if nodes is None:
            _chk(lib().aa_elastic_bind_mesh_obstacle(self.h, C.c_int(mesh_id), None, C.c_int(0)))
            return
        i = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        _chk(lib().aa_elastic_bind_mesh_obstacle(self.h, C.c_int(mesh_id), _ip(i), C.c_int(len(i))))

    def mesh_obstacle_status(self, mesh_id):
        """dict(bound, refits, skipped, last_cause): refits taken and skipped since binding and the
        cause of the last skipped one (0 none, 1 non-finite, 2 zero area, 3 signed volume)."""
        b, r, k, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(lib().aa_elastic_mesh_obstacle_status(self.h, C.c_int(mesh_id), C.byref(b), C.byref(r), C.byref(k), C.byref(c)))
        return dict(bound=bool(b.value), refits=r.value, skipped=k.value, last_cause=c.value)

    def set_mesh_obstacle_exempt(self, mesh_id, nodes):
        """The collision terms of `nodes` skip this mesh as if it were not in the obstacle list.
        Replaces the earlier list; empty or None clears it."""
        i = np.ascontiguousarray([] if nodes is None else nodes, np.int32).reshape(-1)
        _chk(lib().aa_elastic_set_mesh_obstacle_exempt(self.h, C.c_int(mesh_id), _ip(i) if len(i) else None, C.c_int(len(i))))

    def num_obstacles(self):
        """Obstacle rows, analytic and mesh, in the shared insertion order."""
        n = C.c_int()
        _chk(lib().aa_elastic_num_obstacles(self.h, C.byref(n)))
        return n.value

    def set_obstacle(self, index, kind, params):
        """Re-parameterises the analytic obstacle at `index` of the insertion order (add_obstacle's
        parameter layout); `kind` must be the row's stored type."""
        if params is None:
            _chk(lib().aa_elastic_set_obstacle(self.h, C.c_int(index), C.c_int(kind), None))
            return
        p = np.zeros(8)
        q = np.asarray(params, np.float64).reshape(-1)
        p[:len(q)] = q
        _chk(lib().aa_elastic_set_obstacle(self.h, C.c_int(index), C.c_int(kind), _dp(p)))

    def set_obstacle_friction(self, index, mu):
        """Coulomb friction coefficient of obstacle row `index` of the insertion order (analytic and
        mesh rows alike; default 0). Before or after initialize, between steps; the step graph is kept.
        The friction pass runs in a step iff some row has mu > 0 or recording is on."""
        _chk(lib().aa_elastic_set_obstacle_friction(self.h, C.c_int(index), C.c_double(mu)))

    def obstacle_friction(self, index):
        mu = C.c_double()
        _chk(lib().aa_elastic_get_obstacle_friction(self.h, C.c_int(index), C.byref(mu)))
        return mu.value

    def record_contacts(self, on=True):
        """Keep the per-term contact records of every later step even with all coefficients 0."""
        _chk(lib().aa_elastic_record_contacts(self.h, C.c_int(1 if on else 0)))

    def contacts(self):
        """The last step's collision terms in contact, in term order: dict(node (caller's numbering),
        obstacle (row), point, normal, push (j = dt^2 f_n / m), slip (rt), scale (s)); empty when
        the friction pass did not run."""
        n = C.c_int()
        _chk(lib().aa_elastic_get_contacts(self.h, C.c_int(0), C.byref(n), None, None, None, None, None, None, None))
        k = n.value
        node, obs = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
        pt, nr, sl = np.zeros((max(k, 1), 3)), np.zeros((max(k, 1), 3)), np.zeros((max(k, 1), 3))
        push, sc = np.zeros(max(k, 1)), np.zeros(max(k, 1))
        if k:
            _chk(lib().aa_elastic_get_contacts(self.h, C.c_int(k), C.byref(n), _ip(node), _ip(obs), _dp(pt), _dp(nr), _dp(push),
                                               _dp(sl), _dp(sc)))
        return dict(node=node[:k], obstacle=obs[:k], point=pt[:k], normal=nr[:k], push=push[:k], slip=sl[:k], scale=sc[:k])

    def set_mesh_obstacle_carry(self, mesh_id, on=True):
        """Carry, per mesh, default off: the friction pass takes this mesh's displacement at a contact
        from its vertices' own motion since the previous step's pass, so a mesh moved through
        set_mesh_obstacle_vertices or bound to solver nodes drags the nodes on it as a posed one does.
        Before or after initialize, between steps; the step graph is kept."""
        _chk(lib().aa_elastic_set_mesh_obstacle_carry(self.h, C.c_int(mesh_id), C.c_int(1 if on else 0)))

    def mesh_obstacle_carry(self, mesh_id):
        on = C.c_int()
        _chk(lib().aa_elastic_get_mesh_obstacle_carry(self.h, C.c_int(mesh_id), C.byref(on)))
        return bool(on.value)

    def contact_features(self):
        """The last step's contacts in contacts()'s order: dict(tri (the caller's triangle index, -1
        for an analytic row), bary (k, 3) the barycentric weights of the contact point on it). Empty
        when that step's pass was not the carry form."""
        n = C.c_int()
        _chk(lib().aa_elastic_get_contact_features(self.h, C.c_int(0), C.byref(n), None, None))
        k = n.value
        tri, b = np.zeros(max(k, 1), np.int32), np.zeros((max(k, 1), 3))
        if k:
            _chk(lib().aa_elastic_get_contact_features(self.h, C.c_int(k), C.byref(n), _ip(tri), _dp(b)))
        return dict(tri=tri[:k], bary=b[:k])

    def set_collisions(self, inds):
        i = np.ascontiguousarray(inds, np.int32).reshape(-1)
        _chk(lib().aa_elastic_set_collisions(self.h, _ip(i), C.c_int(len(i))))

    def add_wind(self, tris, direction):
        t = np.ascontiguousarray(tris, np.int32).reshape(-1)
        d = np.ascontiguousarray(direction, np.float64).reshape(3)
        k = C.c_int()
        _chk(lib().aa_elastic_add_wind(self.h, _ip(t), C.c_int(len(t) // 3), _dp(d), C.byref(k)))
        return k.value

    def set_wind(self, wid, direction):
        d = np.ascontiguousarray(direction, np.float64).reshape(3)
        _chk(lib().aa_elastic_set_wind(self.h, C.c_int(wid), _dp(d)))

    def set_comm(self, comm):
        """Partition over comm's ranks at initialize() (every rank binds the same scene)."""
        self.comm = comm   # the communicator must outlive the solver
        _chk(lib().aa_elastic_set_comm(self.h, comm.h if comm is not None else None))

    def initialize(self, settings: Settings):
        _chk(lib().aa_elastic_initialize(self.h, C.byref(settings)))
        self.settings = settings

    def save(self, result_dir="./result"):
        """Solver::save() (Solver.hpp:130-155): result_dir/residual-<m>.txt (residual-no.txt
        without acceleration), one row per iteration of the last step -- time (ms since the step
        started, device clock), prim, comb and, for the (u,x) variant (admm_anderson_hard_zxu),
        the reject flag; numbers as `ofs << setprecision(16)` writes them (%.16g)."""
        st = self.settings
        h = self.history()
        t = self.times()
        rej = h["reject"] if st.variant == AA_VARIANT_UX else None
        return write_residual_file(result_dir, st.anderson_m if st.acceleration_type else 0, t, h["prim"], h["comb"], rej)

    def step(self):
        _chk(lib().aa_elastic_step(self.h))

    def num_nodes(self):
        n = C.c_int()
        _chk(lib().aa_elastic_num_nodes(self.h, C.byref(n)))
        return n.value

    @property
    def x(self):
        out = np.zeros(3 * self.num_nodes())
        _chk(lib().aa_elastic_get_x(self.h, _dp(out)))
        return out.reshape(-1, 3)

    @property
    def v(self):
        out = np.zeros(3 * self.num_nodes())
        _chk(lib().aa_elastic_get_v(self.h, _dp(out)))
        return out.reshape(-1, 3)

    def set_v(self, v):
        """Solver::m_v assignment between steps (velocities, n x 3)."""
        v = np.ascontiguousarray(v, np.float64).reshape(-1)
        _chk(lib().aa_elastic_set_v(self.h, _dp(v)))

    def set_state(self, x, v):
        """Solver::m_x / m_v assignment between steps (positions and velocities, n x 3)."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        v = np.ascontiguousarray(v, np.float64).reshape(-1)
        _chk(lib().aa_elastic_set_x(self.h, _dp(x)))
        _chk(lib().aa_elastic_set_v(self.h, _dp(v)))

    def history(self, cap=100000):
        p, c, r = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
        n = C.c_int()
        _chk(lib().aa_elastic_get_history(self.h, _dp(p), _dp(c), _ip(r), C.c_int(cap), C.byref(n)))
        k = min(n.value, cap)
        return dict(prim=p[:k].copy(), comb=c[:k].copy(), reject=r[:k].copy())

    def times(self, cap=100000):
        """Device-clock ms from the start of the last step to the end of each recorded iteration."""
        t = np.zeros(cap)
        n = C.c_int()
        _chk(lib().aa_elastic_get_times(self.h, _dp(t), C.c_int(cap), C.byref(n)))
        return t[:min(n.value, cap)].copy()

    def set_iterations(self, admm_iters, eps_rel=0.0):
        """Settings::admm_iters and the run-to-epsilon stop of later steps (no re-factor)."""
        _chk(lib().aa_elastic_set_iterations(self.h, C.c_int(admm_iters), C.c_double(eps_rel)))

    def runtime(self) -> Runtime:
        rt = Runtime()
        _chk(lib().aa_elastic_runtime(self.h, C.byref(rt)))
        return rt

    def bench_iterations(self, iters):
        ms = C.c_double()
        _chk(lib().aa_elastic_bench_iterations(self.h, C.c_int(iters), C.byref(ms)))
        return ms.value

    def setup_phases(self):
        """{phase: ms} of the last initialize() (aa_elastic_setup_phases), in order."""
        names = C.create_string_buffer(4096)
        ms = (C.c_double * 64)()
        n = C.c_int()
        _chk(lib().aa_elastic_setup_phases(self.h, names, 4096, ms, 64, C.byref(n)))
        keys = names.value.decode().split("\n") if n.value else []
        return {k: round(ms[i], 1) for i, k in enumerate(keys[:64])}

    def kernel_stats(self, name):
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        _chk(lib().aa_elastic_kernel_stats(self.h, name.encode(), C.byref(a), C.byref(b), C.byref(n)))
        return dict(avg_ms=a.value, bytes=b.value, launches=n.value)

    def local_stats(self, reset=True):
        """Work-queue diagnostics of the hyperelastic local step (AA_LQ_STATS=1 at initialize):
        the per-element L-BFGS iteration histogram and the trip / refill / wave counts."""
        out = np.zeros(104, np.int64)
        n = C.c_int()
        _chk(lib().aa_elastic_local_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_longlong)), C.c_int(104),
                                          C.c_int(1 if reset else 0), C.byref(n)))
        return dict(hist=out[:101].copy(), trips=int(out[101]), refills=int(out[102]), waves=int(out[103]))


def pose12(R, t=None):
    """R (3, 3) and t (3,) as the 12 doubles of aa_elastic_set_mesh_obstacle_pose: R row-major, then t."""
    p = np.zeros(12)
    p[:9] = np.asarray(R, np.float64).reshape(9)
    if t is not None:
        p[9:] = np.asarray(t, np.float64).reshape(3)
    return p


def _pose_arg(pose):
    """A pose given as (R, t) or as 12 doubles."""
    if isinstance(pose, (tuple, list)) and len(pose) == 2:
        return pose12(pose[0], pose[1])
    return np.ascontiguousarray(pose, np.float64).reshape(12).copy()


def solver_from_scene(ctx: Context, scene, comm=None) -> Solver:
    """Binds a scenes.Scene the way binding::add_trimesh/add_tetmesh + the samples do."""
    s = Solver(ctx)
    if comm is not None:
        s.set_comm(comm)
    s.add_nodes(scene.x, np.repeat(np.asarray(scene.masses, np.float64), 3))
    for g in scene.groups:
        if g.per_element:   # arrays of the group's length: one group with per-element materials
            E, nu, lmin, lmax = g.material_arrays()
            mu = E / (2.0 * (1.0 + nu))    # Lame.from_young's expressions, per element
            lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
            if g.kind == 0:
                s.add_tets_var(scene.rest_x, g.idx, g.material, mu, lam)
            else:
                s.add_tris_var(scene.rest_x, g.idx, mu, lam, lmin, lmax)
            continue
        lame = Lame.from_young(g.E, g.nu, g.limit_min, g.limit_max)
        if g.kind == 0:
            s.add_tets(scene.rest_x, g.idx, g.material, lame)
        else:
            s.add_tris(scene.rest_x, g.idx, lame)
    for tris, k_bend, flat_rest in getattr(scene, "bending", None) or []:   # after the groups
        s.add_bending(scene.rest_x, tris, k_bend, flat_rest)
    for pairs, k, rest, mode in getattr(scene, "springs", None) or []:   # after the bending entries
        s.add_springs(pairs, k, rest, mode, verts=scene.rest_x)
    for nodes_a, w_a, nodes_b, w_b, k, rest, mode in getattr(scene, "ties", None) or []:   # after the springs
        s.add_ties(nodes_a, w_a, nodes_b, w_b, k, rest, mode, verts=scene.rest_x)
    s.set_pins(scene.pin_idx, scene.pin_pts)
    for kind, prm in getattr(scene, "obstacles", []):
        s.add_obstacle(kind, prm)
    for V, F in getattr(scene, "mesh_obstacles", []):   # after the analytic ones in the insertion order
        s.add_mesh_obstacle(V, F)
    if getattr(scene, "collision_idx", None) is not None:
        s.set_collisions(scene.collision_idx)
    for tris, direction in getattr(scene, "winds", []):
        s.add_wind(tris, direction)
    for m, nodes in enumerate(getattr(scene, "mesh_obstacle_bindings", None) or []):
        if nodes is not None:
            s.bind_mesh_obstacle(m, nodes)
    for m, nodes in enumerate(getattr(scene, "mesh_obstacle_exempt", None) or []):
        if nodes is not None:
            s.set_mesh_obstacle_exempt(m, nodes)
    for row, mu in enumerate(getattr(scene, "obstacle_friction", None) or []):   # per row of the insertion order
        if mu is not None:
            s.set_obstacle_friction(row, mu)
    if getattr(scene, "record_contacts", False):
        s.record_contacts(True)
    for m, on in enumerate(getattr(scene, "mesh_obstacle_carry", None) or []):
        if on:
            s.set_mesh_obstacle_carry(m, True)
    return s


def closest_on_triangles(ctx: Context, V, F, Q):
    """Where the queries Q (n, 3) land on the triangle list (V, F) (aa_closest_on_triangles; any list,
    open or non-manifold): (closest points (n, 3), triangle (n,) in F's numbering, barycentric
    weights (n, 3) of the closest point on that triangle's corners)."""
    v = np.ascontiguousarray(V, np.float64).reshape(-1)
    f = np.ascontiguousarray(F, np.int32).reshape(-1)
    q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    n = q.shape[0]
    c, tri, b = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros((n, 3))
    _chk(lib().aa_closest_on_triangles(ctx.h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(len(f) // 3), _dp(q), C.c_int(n),
                                       _dp(c), _ip(tri), _dp(b)))
    return c, tri, b


def ties_to_surface(ctx: Context, x, nodes, F, k, mode=AA_SPRING, rest=None):
    """Ties from the nodes `nodes` to where they land on the surface (x, F): the query runs for
    x[nodes] against (x, F), and the result is a Scene.ties entry (nodes_a, w_a, nodes_b, w_b, k, rest,
    mode) with na = 3 (the triangle's corners, the query's barycentric weights) and nb = 1 (the node,
    weight 1). The triangles must not contain the tied nodes (a tie names no node twice). rest = None:
    the distance at binding time."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    nodes = np.asarray(nodes, np.int32).reshape(-1)
    F = np.asarray(F, np.int32).reshape(-1, 3)
    _, tri, b = closest_on_triangles(ctx, x, F, x[nodes])
    return (F[tri].astype(np.int32), b, nodes.reshape(-1, 1), np.ones((len(nodes), 1)), k, rest, int(mode))


def settings_from_scene(scene) -> Settings:
    return Settings(timestep_s=scene.dt, admm_iters=scene.iters, gravity=scene.gravity, anderson_m=scene.aa_m,
                    penalty=scene.penalty, acceleration_type=ANDERSON if scene.accel else NOACC,
                    variant=scene.variant, verbose=0)


def run_scene(ctx: Context, scene, n_steps=None, comm=None):
    """Runs the scene like the reference driver; returns per-step dicts (prim, comb, reject, x, v)."""
    s = solver_from_scene(ctx, scene, comm)
    s.initialize(settings_from_scene(scene))
    if getattr(scene, "initial_velocity", None) is not None:
        s.set_v(scene.initial_velocity)
    out = []
    n_steps = scene.n_steps if n_steps is None else n_steps
    for k in range(1, n_steps + 1):
        if np.any(scene.pin_vel != 0):
            s.set_pins(scene.pin_idx, scene.pin_pts + k * scene.pin_vel)
        poses = getattr(scene, "mesh_obstacle_poses", None)
        if poses is not None:   # kinematic obstacles: step k runs against row k - 1 (the last row holds on)
            row = np.asarray(poses, np.float64)[min(k, len(poses)) - 1]
            for m in range(row.shape[0]):
                s.set_mesh_obstacle_pose(m, row[m, :9].reshape(3, 3), row[m, 9:])
        moves = getattr(scene, "obstacle_motion", None)
        if moves:   # moving analytic obstacles: step k runs against entry k - 1 (the last entry holds on)
            for row, prm in enumerate(moves[min(k, len(moves)) - 1]):
                if prm is not None:
                    s.set_obstacle(row, scene.obstacles[row][0], prm)
        shapes = getattr(scene, "mesh_obstacle_vertices", None)
        if shapes:   # deforming obstacles: step k runs against entry k - 1 (the last entry holds on)
            for m, V in enumerate(shapes[min(k, len(shapes)) - 1]):
                if V is not None:
                    s.set_mesh_obstacle_vertices(m, V)
        s.step()
        h = s.history()
        h["x"], h["v"] = s.x, s.v
        rt = s.runtime()
        h["step_ms"] = rt.step_ms
        h["iterations"], h["rejects"] = rt.iterations, rt.rejects
        out.append(h)
    return out, s


# ------------------------------------------------------------------------------------------
# Geometry: ALMGeometrySolver<3> (Geometry/ALMGeometrySolver.h)
# ------------------------------------------------------------------------------------------

def write_residual_file(result_dir, anderson_m, *cols):
    """The residual-<m>.txt / residual-no.txt writer shared by Solver.save and GeomSolver.save:
    tab-separated columns, floats as %.16g (C++ setprecision(16), default float format), ints
    as %d; a None column is left out."""
    cols = [c for c in cols if c is not None]
    n = min(len(c) for c in cols)
    path = os.path.join(result_dir, f"residual-{anderson_m}.txt" if anderson_m > 0 else "residual-no.txt")
    with open(path, "w") as f:
        for i in range(n):
            f.write("\t".join(("%d" % c[i]) if np.issubdtype(np.asarray(c).dtype, np.integer) else ("%.16g" % c[i])
                              for c in cols) + "\n")
    return path


class GeomRuntime(C.Structure):
    _fields_ = [("setup_ms", C.c_double), ("factor_ms", C.c_double), ("solve_ms", C.c_double),
                ("iterations", C.c_int), ("accepted", C.c_int), ("rejects", C.c_int), ("n_points", C.c_int),
                ("nnz_factor", C.c_longlong), ("hard_cols", C.c_longlong), ("soft_cols", C.c_longlong),
                ("n_constraints", C.c_longlong)]


class GeomSolver:
    """Mirror of ALMGeometrySolver<3> (kind AA_GEOM_ALM) or GeometrySolver<3> (AA_GEOM_PLAIN):
    add_hard/soft constraints, add_*laplacian, add_closeness, setup_ADMM, solve_ADMM,
    get_solution, function_values_ / elapsed_time_."""

    def __init__(self, ctx: Context, kind=AA_GEOM_ALM):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n = 0
        _chk(lib().aa_geom_create_kind(ctx.h, C.c_int(kind), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().aa_geom_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_ref_surface(self, V, F):
        V = np.ascontiguousarray(V, np.float64).reshape(-1)
        F = np.ascontiguousarray(F, np.int32).reshape(-1)
        i = C.c_int()
        _chk(lib().aa_geom_add_ref_surface(self.h, _dp(V), C.c_int(len(V) // 3), _ip(F), C.c_int(len(F) // 3),
                                           C.byref(i)))
        return i.value

    def add_constraints(self, hard, ctype, idx, weight=1.0, params=None):
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.ndim == 1:
            idx = idx[:, None]
        count, k = idx.shape
        prm = None if params is None else np.ascontiguousarray(params, np.float64).reshape(count, -1)
        _chk(lib().aa_geom_add_constraints(self.h, C.c_int(int(hard)), C.c_int(ctype), _ip(idx), C.c_int(k),
                                           C.c_int(count), C.c_double(weight), None if prm is None else _dp(prm)))

    def add_laplacian(self, idx, coefs, weight, ref_points=None):
        i = np.ascontiguousarray(idx, np.int32)
        c = np.ascontiguousarray(coefs, np.float64)
        r = None if ref_points is None else np.ascontiguousarray(ref_points, np.float64).reshape(-1)
        _chk(lib().aa_geom_add_laplacian(self.h, _ip(i), _dp(c), C.c_int(len(i)), C.c_double(weight),
                                         None if r is None else _dp(r)))

    def add_closeness(self, idx, weight, target):
        t = np.ascontiguousarray(target, np.float64)
        _chk(lib().aa_geom_add_closeness(self.h, C.c_int(idx), C.c_double(weight), _dp(t)))

    def add_laplacians(self, row_ptr, idx, coefs, weights, relative=None, ref_points=None):
        """n_rows add_laplacian calls in one (CSR rows; relative[r] != 0: add_relative_laplacian)."""
        rp = np.ascontiguousarray(row_ptr, np.int32)
        i = np.ascontiguousarray(idx, np.int32)
        c = np.ascontiguousarray(coefs, np.float64)
        w = np.ascontiguousarray(weights, np.float64)
        rl = None if relative is None else np.ascontiguousarray(relative, np.int32)
        r = None if ref_points is None else np.ascontiguousarray(ref_points, np.float64).reshape(-1)
        _chk(lib().aa_geom_add_laplacians(self.h, C.c_int(len(rp) - 1), _ip(rp), _ip(i), _dp(c), _dp(w),
                                          None if rl is None else _ip(rl), None if r is None else _dp(r)))

    def add_closenesses(self, idx, weights, targets):
        i = np.ascontiguousarray(idx, np.int32)
        w = np.ascontiguousarray(weights, np.float64)
        t = np.ascontiguousarray(targets, np.float64).reshape(-1)
        _chk(lib().aa_geom_add_closenesses(self.h, C.c_int(len(i)), _ip(i), _dp(w), _dp(t)))

    def set_comm(self, comm):
        """Partition over comm's ranks at the first solve (every rank adds the same problem)."""
        self.comm = comm
        _chk(lib().aa_geom_set_comm(self.h, comm.h if comm is not None else None))

    def setup(self, n_points, penalty, spd=AA_SPD_LDLT):
        self.n = n_points
        _chk(lib().aa_geom_setup(self.h, C.c_int(n_points), C.c_double(penalty), C.c_int(spd)))

    def solve(self, init_x, rel_eps, max_iter, m):
        x = np.ascontiguousarray(init_x, np.float64).reshape(-1)
        _chk(lib().aa_geom_solve(self.h, _dp(x), C.c_double(rel_eps), C.c_int(max_iter), C.c_int(m)))

    def set_stop(self, at_eps=False, eps_rel=0.0):
        """Run-to-epsilon for later solves (aa_geom_set_stop): stop at the reference's
        commented-out criterion comb < rel_eps^2 hard_cols^2 2 and/or comb <= eps_rel comb_0."""
        _chk(lib().aa_geom_set_stop(self.h, C.c_int(1 if at_eps else 0), C.c_double(eps_rel)))

    def solution(self):
        out = np.zeros(3 * self.n)
        _chk(lib().aa_geom_get_solution(self.h, _dp(out)))
        return out.reshape(-1, 3)

    def history(self, cap=1 << 20):
        n = C.c_int()
        _chk(lib().aa_geom_get_history(self.h, None, None, C.c_int(0), C.byref(n)))
        k = n.value
        c, t = np.zeros(max(k, 1)), np.zeros(max(k, 1))
        _chk(lib().aa_geom_get_history(self.h, _dp(c), _dp(t), C.c_int(k), C.byref(n)))
        return dict(comb=c[:k].copy(), time_s=t[:k].copy())

    def save(self, anderson_m, result_dir="./result"):
        """ALMGeometrySolver::save(Anderson_m) (ALMGeometrySolver.h:343-365; GeometrySolver.h
        likewise): "elapsed_time_ <tab> function_values_" per recorded iteration."""
        h = self.history()
        return write_residual_file(result_dir, anderson_m, h["time_s"], h["comb"])

    def runtime(self) -> GeomRuntime:
        rt = GeomRuntime()
        _chk(lib().aa_geom_runtime_info(self.h, C.byref(rt)))
        return rt

    def closest_points(self, surface, P):
        P = np.ascontiguousarray(P, np.float64).reshape(-1)
        out = np.zeros_like(P)
        _chk(lib().aa_geom_closest_points(self.h, C.c_int(surface), _dp(P), C.c_int(len(P) // 3), _dp(out)))
        return out.reshape(-1, 3)

    def bench_iterations(self, iters):
        ms = C.c_double()
        _chk(lib().aa_geom_bench_iterations(self.h, C.c_int(iters), C.byref(ms)))
        return ms.value

    def kernel_stats(self, name):
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        _chk(lib().aa_geom_kernel_stats(self.h, name.encode(), C.byref(a), C.byref(b), C.byref(n)))
        return dict(avg_ms=a.value, bytes=b.value, launches=n.value)


def geom_from_scene(ctx: Context, sc, comm=None, timings=None) -> GeomSolver:
    """Binds a geom_scenes.GeomScene the way optimize_mesh (PlanarityOpt.cpp / WireMeshOpt.cpp) does.
    timings (dict, optional) receives the wall ms of each binding phase."""
    import time
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        if timings is not None:
            timings[name] = round((t[-1] - t[-2]) * 1e3, 1)
    g = GeomSolver(ctx, AA_GEOM_PLAIN if getattr(sc, "solver", "alm") == "plain" else AA_GEOM_ALM)
    lap("create_ms")
    if comm is not None:
        g.set_comm(comm)
    sids = [g.add_ref_surface(V, F) for V, F in sc.surfaces]
    for grp in sc.groups:
        prm = grp.params
        if grp.type in (AA_CON_POINT_TO_REF, AA_CON_REF_SURFACE):   # scene surface ids -> solver ids
            prm = np.asarray(sids, np.float64)[np.asarray(prm).reshape(grp.count, -1)[:, 0].astype(np.int64)][:, None]
        g.add_constraints(grp.hard, grp.type, grp.idx, grp.weight, prm)
    lap("surfaces_constraints_ms")
    # regularisation rows in insertion order, one batched call per run of laplacian (kinds 0, 1)
    # or closeness (kind 2) rows -- the same rows as one add_* call each
    kind = np.asarray(sc.reg_kind, np.int32)
    ptr = np.asarray(sc.reg_ptr, np.int64)
    i = 0
    while i < len(kind):
        clo = kind[i] == 2
        j = i + 1
        while j < len(kind) and (kind[j] == 2) == clo:
            j += 1
        if clo:
            g.add_closenesses(np.asarray(sc.reg_idx)[ptr[i:j]], np.asarray(sc.reg_weight)[i:j],
                              np.asarray(sc.reg_target)[i:j])
        else:
            a, b = int(ptr[i]), int(ptr[j])
            rel = kind[i:j] == 1
            g.add_laplacians(ptr[i:j + 1] - a, np.asarray(sc.reg_idx)[a:b], np.asarray(sc.reg_coef)[a:b],
                             np.asarray(sc.reg_weight)[i:j], rel.astype(np.int32) if rel.any() else None,
                             sc.ref_points if rel.any() else None)
        i = j
    lap("regularization_ms")
    g.setup(sc.n_points, sc.penalty)
    lap("setup_admm_ms")
    return g


def run_geom(ctx: Context, sc, comm=None):
    """setup_ADMM + solve_ADMM of a GeomScene; returns dict(comb, time_s, x) and the solver."""
    g = geom_from_scene(ctx, sc, comm)
    g.solve(sc.x0, 1e-8 * max(sc.avg_edge_length(), 1e-300), sc.iters, sc.aa_m)
    h = g.history()
    h["x"] = g.solution()
    return h, g


# ------------------------------------------------------------------------------------------
# element-level test hooks (aa_test_*): the device prox / COD / projection functions
# ------------------------------------------------------------------------------------------

def hook_prox(ctx: Context, op, prm4, X):
    """op 0 linear tet, 1 NeoHookean, 2 StVK (prm4 = E, nu, h), 3 / 4 tri H / X prox (prm4[2:] =
    limits), 5 the bending hinge's prox (prm4[0] = r), 6 the spring's prox (prm4 = L, mode); X (n, 9|6|3). Returns (out, L-BFGS iterations)."""
    X = np.ascontiguousarray(X, np.float64)
    n = X.shape[0]
    out, it = np.zeros_like(X), np.zeros(n, np.int32)
    p = np.zeros(4)
    q = np.asarray(prm4, np.float64).reshape(-1)
    p[:len(q)] = q
    _chk(lib().aa_test_prox(ctx.h, C.c_int(op), _dp(p), _dp(X), C.c_int(n), _dp(out), _ip(it)))
    return out, it


def hook_cod_solve(ctx: Context, M, b):
    Mc = np.asfortranarray(M, np.float64).ravel(order="F").copy()
    bb = np.ascontiguousarray(b, np.float64)
    th = np.zeros(len(bb))
    _chk(lib().aa_test_cod_solve(ctx.h, C.c_int(len(bb)), _dp(Mc), _dp(bb), _dp(th)))
    return th


def hook_geom_project(ctx: Context, ctype, k, params, P):
    """P (n, cols, 3) transformed points; params (2,) (angle min/max or edge length)."""
    P = np.ascontiguousarray(P, np.float64)
    out = np.zeros_like(P)
    prm = np.zeros(2)
    if params is not None:
        a = np.atleast_1d(np.asarray(params, np.float64))
        prm[:len(a)] = a
    _chk(lib().aa_test_geom_project(ctx.h, C.c_int(ctype), C.c_int(k), _dp(prm), _dp(P), C.c_int(P.shape[0]), _dp(out)))
    return out


def hook_mesh_sdf(ctx: Context, V, F, Q, pose=None):
    """The mesh obstacle's signed distance on queries Q (n, 3): (closest points, dx, triangle) with
    dx = -|q - c| inside and +|q - c| otherwise, the triangle in F's numbering. pose = (R, t) or 12
    doubles: the obstacle posed (Q and the closest points in the world frame)."""
    v = np.ascontiguousarray(V, np.float64).reshape(-1)
    f = np.ascontiguousarray(F, np.int32).reshape(-1)
    q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    n = q.shape[0]
    c, dx, tri = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    if pose is not None:
        _chk(lib().aa_test_mesh_sdf_posed(ctx.h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(len(f) // 3),
                                          _dp(_pose_arg(pose)), _dp(q), C.c_int(n), _dp(c), _dp(dx), _ip(tri)))
        return c, dx, tri
    _chk(lib().aa_test_mesh_sdf(ctx.h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(len(f) // 3), _dp(q), C.c_int(n),
                                _dp(c), _dp(dx), _ip(tri)))
    return c, dx, tri


def hook_mesh_refit_tables(ctx, V, F, V_new=None, device=1):
    """The tables of the mesh obstacle (V, F), refitted to V_new when given: dict of nodes (n_nodes,
    128) uint8, tris (m, 9), pn (m, 21), orig (m,), lo (3,), hi (3,). device = 0: the host
    restatement (ctx may be None); 1: what the kernels wrote."""
    v = np.ascontiguousarray(V, np.float64).reshape(-1)
    f = np.ascontiguousarray(F, np.int32).reshape(-1)
    w = None if V_new is None else np.ascontiguousarray(V_new, np.float64).reshape(-1)
    if w is not None and len(w) != len(v):
        raise ValueError("hook_mesh_refit_tables: V_new must have V's shape")
    m = len(f) // 3
    h = ctx.h if ctx is not None else None
    nodes = np.zeros((2 * max(m, 1), 128), np.uint8)   # a leaf holds a triangle at least: fewer than 2 m nodes
    tris, pn, orig, lohi, nn = np.zeros((m, 9)), np.zeros((m, 21)), np.zeros(m, np.int32), np.zeros(6), C.c_int()
    _chk(lib().aa_test_mesh_refit_tables(h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(m), None if w is None else _dp(w),
                                         C.c_int(device), nodes.ctypes.data_as(C.c_void_p), _dp(tris), _dp(pn), _ip(orig),
                                         _dp(lohi), C.byref(nn)))
    return dict(nodes=nodes[:nn.value].copy(), tris=tris, pn=pn, orig=orig, lo=lohi[:3].copy(), hi=lohi[3:].copy())


def hook_bound_refit(ctx, V, F, X, nodes, device=1, timing=False, X_first=None):
    """aa_test_bound_refit: the mesh (V, F), its vertices gathered as X[nodes] from the node array X
    (n, 3), checked and -- when the check passes -- refitted. hook_mesh_refit_tables' dict plus
    taken (bool), cause (0..3) and vol6. device = 0: the host restatement (ctx may be None).
    X_first: a bound refit from these positions runs first, as an earlier step's would (its status is
    not reported). timing (device = 1): also ms, the device time of gather + check + refit (median of 5)."""
    v = np.ascontiguousarray(V, np.float64).reshape(-1)
    f = np.ascontiguousarray(F, np.int32).reshape(-1)
    x = np.ascontiguousarray(X, np.float64).reshape(-1)
    i = np.ascontiguousarray(nodes, np.int32).reshape(-1)
    if 3 * len(i) != len(v):
        raise ValueError("hook_bound_refit: one node per vertex")
    m = len(f) // 3
    h = ctx.h if ctx is not None else None
    nd = np.zeros((2 * max(m, 1), 128), np.uint8)
    tris, pn, orig, lohi, nn = np.zeros((m, 9)), np.zeros((m, 21)), np.zeros(m, np.int32), np.zeros(6), C.c_int()
    st, vol6, ms = np.zeros(2, np.int32), C.c_double(), C.c_double()
    x0 = None if X_first is None else np.ascontiguousarray(X_first, np.float64).reshape(-1)
    if x0 is not None and len(x0) != len(x):
        raise ValueError("hook_bound_refit: X_first must have X's shape")
    _chk(lib().aa_test_bound_refit(h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(m), _dp(x), C.c_int(len(x) // 3), _ip(i),
                                   C.c_int(device), nd.ctypes.data_as(C.c_void_p), _dp(tris), _dp(pn), _ip(orig), _dp(lohi),
                                   C.byref(nn), _ip(st), C.byref(vol6), C.byref(ms) if timing else None,
                                   None if x0 is None else _dp(x0)))
    out = dict(nodes=nd[:nn.value].copy(), tris=tris, pn=pn, orig=orig, lo=lohi[:3].copy(), hi=lohi[3:].copy(),
               taken=bool(st[0]), cause=int(st[1]), vol6=float(vol6.value))
    if timing:
        out["ms"] = float(ms.value)
    return out


def hook_collision_prox_exempt(ctx: Context, obstacles, meshes, Q, q_nodes, exempt, poses=None):
    """hook_collision_prox with the node of every query (q_nodes (n,)) and, per mesh, the nodes
    exempt from it (exempt: one list or None per mesh)."""
    rows = np.zeros((len(obstacles), 8))
    for k, (kind, prm) in enumerate(obstacles):
        a = np.asarray(prm, np.float64).reshape(-1)
        rows[k, 0] = kind
        rows[k, 1:1 + len(a)] = a
    vs = [np.ascontiguousarray(V, np.float64).reshape(-1, 3) for V, _ in meshes]
    fs = [np.ascontiguousarray(F, np.int32).reshape(-1, 3) for _, F in meshes]
    vptr = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int32)
    fptr = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int32)
    vv = np.ascontiguousarray(np.concatenate(vs) if vs else np.zeros((1, 3)))
    ff = np.ascontiguousarray(np.concatenate(fs) if fs else np.zeros((1, 3), np.int32))
    q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    qn = np.ascontiguousarray(q_nodes, np.int32).reshape(-1)
    if len(qn) != len(q) or len(exempt) != len(meshes):
        raise ValueError("hook_collision_prox_exempt: one node per query, one exempt list (or None) per mesh")
    lists = [np.asarray([] if e is None else e, np.int32).reshape(-1) for e in exempt]
    eptr = np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.int32)
    enodes = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)
    pp = None
    if poses is not None:
        pp = np.full((max(len(meshes), 1), 12), np.nan)
        for m, p in enumerate(poses):
            if p is not None:
                pp[m] = _pose_arg(p)
    out = np.zeros_like(q)
    _chk(lib().aa_test_collision_prox_exempt(ctx.h, _dp(rows), C.c_int(len(obstacles)), _dp(vv), _ip(vptr), _ip(ff), _ip(fptr),
                                             C.c_int(len(meshes)), None if pp is None else _dp(pp), _dp(q), _ip(qn),
                                             C.c_int(q.shape[0]), _ip(eptr), _ip(enodes), _dp(out)))
    return out


def hook_contact_friction(ctx: Context, obstacles, obstacles_prev, mu, meshes, x_old, x_new, u, w, m, penalty, dt,
                          q_nodes=None, pinned=None, exempt=None, poses=None, poses_prev=None, mesh_still=None, _carry=None):
    """The friction pass's device function (aa_test_contact_friction) on n queries. obstacles /
    obstacles_prev: (type, params) rows now and during the previous step (a mesh as (AA_OBS_MESH,
    [k]) naming meshes[k] = (V, F)), mu one coefficient per row; poses / poses_prev: per mesh (R, t),
    12 doubles or None; mesh_still: per mesh, True = no displacement is derived for it. Per query
    x_old, x_new, u (n, 3), w, m (n,), the exemption node id and a pinned flag. Returns dict(x, hit,
    row, point, normal, push, slip, scale)."""
    def rows_of(obs):
        rows = np.zeros((max(len(obs), 1), 8))
        for k, (kind, prm) in enumerate(obs):
            a = np.asarray(prm, np.float64).reshape(-1)
            rows[k, 0] = kind
            rows[k, 1:1 + len(a)] = a
        return rows
    if len(obstacles_prev) != len(obstacles) or len(mu) != len(obstacles):
        raise ValueError("hook_contact_friction: one previous row and one coefficient per obstacle row")
    rows, rows_prev = rows_of(obstacles), rows_of(obstacles_prev)
    mus = np.ascontiguousarray(np.concatenate([np.asarray(mu, np.float64).reshape(-1), np.zeros(1)]))
    vs = [np.ascontiguousarray(V, np.float64).reshape(-1, 3) for V, _ in meshes]
    fs = [np.ascontiguousarray(F, np.int32).reshape(-1, 3) for _, F in meshes]
    vptr = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int32)
    fptr = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int32)
    vv = np.ascontiguousarray(np.concatenate(vs) if vs else np.zeros((1, 3)))
    ff = np.ascontiguousarray(np.concatenate(fs) if fs else np.zeros((1, 3), np.int32))
    xo = np.ascontiguousarray(x_old, np.float64).reshape(-1, 3)
    xn = np.ascontiguousarray(x_new, np.float64).reshape(-1, 3)
    uu = np.ascontiguousarray(u, np.float64).reshape(-1, 3)
    n = len(xn)
    ww = np.ascontiguousarray(np.broadcast_to(np.asarray(w, np.float64), (n,)))
    mm = np.ascontiguousarray(np.broadcast_to(np.asarray(m, np.float64), (n,)))
    qn = np.ascontiguousarray(np.zeros(n) if q_nodes is None else q_nodes, np.int32).reshape(-1)
    pin = np.ascontiguousarray(np.zeros(n) if pinned is None else pinned, np.uint8).reshape(-1)
    if not (len(xo) == len(uu) == len(qn) == len(pin) == n):
        raise ValueError("hook_contact_friction: the per-query arrays differ in length")
    lists = [np.asarray([] if e is None else e, np.int32).reshape(-1) for e in (exempt or [None] * len(meshes))]
    if len(lists) != len(meshes):
        raise ValueError("hook_contact_friction: one exempt list (or None) per mesh")
    eptr = np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.int32)
    enodes = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)

    def pose_rows(poses):
        pp = np.full((max(len(meshes), 1), 12), np.nan)   # a row of NaNs: that mesh unposed
        for k, p in enumerate(poses or []):
            if p is not None:
                pp[k] = _pose_arg(p)
        return pp
    pp, pq = pose_rows(poses), pose_rows(poses_prev)
    still = np.ascontiguousarray(np.zeros(max(len(meshes), 1)) if mesh_still is None else
                                 np.concatenate([np.asarray(mesh_still, np.float64).reshape(-1), np.zeros(1)]), np.uint8)
    _ub = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
    k1 = max(n, 1)
    x, hit, row = np.zeros((k1, 3)), np.zeros(k1, np.int32), np.zeros(k1, np.int32)
    pt, nr, sl, push, sc = np.zeros((k1, 3)), np.zeros((k1, 3)), np.zeros((k1, 3)), np.zeros(k1), np.zeros(k1)
    head = (ctx.h, _dp(rows), _dp(rows_prev), _dp(mus), C.c_int(len(obstacles)), _dp(vv), _ip(vptr), _ip(ff), _ip(fptr),
            C.c_int(len(meshes)), _dp(pp), _dp(pq), _ub(still), _ip(qn), _ub(pin), C.c_int(n), _ip(eptr), _ip(enodes), _dp(xo),
            _dp(xn), _dp(uu), _dp(ww), _dp(mm), C.c_double(penalty), C.c_double(dt))
    outs = (_dp(x), _ip(hit), _ip(row), _dp(pt), _dp(nr), _dp(push), _dp(sl), _dp(sc))
    result = lambda: dict(x=x[:n], hit=hit[:n].astype(bool), row=row[:n], point=pt[:n], normal=nr[:n], push=push[:n],
                          slip=sl[:n], scale=sc[:n])
    if _carry is None:
        _chk(lib().aa_test_contact_friction(*head, *outs))
        return result()
    verts_prev, flags = _carry
    if len(verts_prev) != len(meshes) or len(flags) != len(meshes):
        raise ValueError("hook_contact_friction_carry: previous vertices and a carry flag per mesh")
    ps = [np.ascontiguousarray(vs[k] if P is None else P, np.float64).reshape(-1, 3) for k, P in enumerate(verts_prev)]
    if any(a.shape != b.shape for a, b in zip(ps, vs)):
        raise ValueError("hook_contact_friction_carry: the previous vertices differ in count from the mesh's")
    vp = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros((1, 3)))
    cf = np.ascontiguousarray(np.concatenate([np.asarray(flags, np.float64).reshape(-1), np.zeros(1)]), np.uint8)
    tri, b = np.zeros(k1, np.int32), np.zeros((k1, 3))
    _chk(lib().aa_test_contact_friction_carry(*head, _dp(vp), _ub(cf), *outs, _ip(tri), _dp(b)))
    out = result()
    out.update(tri=tri[:n], bary=b[:n])
    return out


def hook_contact_friction_carry(ctx: Context, obstacles, obstacles_prev, mu, meshes, x_old, x_new, u, w, m, penalty, dt,
                                verts_prev, carry, **kw):
    """The carry form of the pass's device function (aa_test_contact_friction_carry):
    hook_contact_friction's arguments plus, per mesh, the previous vertices (n, 3) (None = the mesh's
    own) and the carry flag. Also returns tri (the caller's triangle index of a mesh-row contact, -1
    otherwise) and bary (n, 3)."""
    return hook_contact_friction(ctx, obstacles, obstacles_prev, mu, meshes, x_old, x_new, u, w, m, penalty, dt,
                                 _carry=(verts_prev, carry), **kw)


def hook_mesh_sdf_deformed(ctx: Context, V, F, V_new, Q, pose=None, timings=False):
    """hook_mesh_sdf on the mesh built from (V, F) and refitted on the device to V_new. timings: a
    fourth result, the ms of (host prepare + upload of (V_new, F) from scratch, the device refit, the
    signed-distance kernel on the refitted tree, the same on a freshly built tree)."""
    v = np.ascontiguousarray(V, np.float64).reshape(-1)
    w = np.ascontiguousarray(V_new, np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("hook_mesh_sdf_deformed: V_new must have V's shape")
    f = np.ascontiguousarray(F, np.int32).reshape(-1)
    q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    n = q.shape[0]
    c, dx, tri, ms = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32), np.zeros(4)
    _chk(lib().aa_test_mesh_sdf_deformed(ctx.h, _dp(v), C.c_int(len(v) // 3), _ip(f), C.c_int(len(f) // 3), _dp(w),
                                         None if pose is None else _dp(_pose_arg(pose)), _dp(q), C.c_int(n), _dp(c), _dp(dx),
                                         _ip(tri), _dp(ms) if timings else None))
    return (c, dx, tri, ms) if timings else (c, dx, tri)


def hook_collision_prox(ctx: Context, obstacles, meshes, Q, poses=None):
    """Collision::prox of candidates Q (n, 3) against `obstacles` in insertion order: (type, params)
    pairs, a mesh as (AA_OBS_MESH, [m]) naming meshes[m] = (V, F). poses: one entry per mesh, (R, t)
    or 12 doubles, None for an unposed mesh."""
    rows = np.zeros((len(obstacles), 8))
    for k, (kind, prm) in enumerate(obstacles):
        a = np.asarray(prm, np.float64).reshape(-1)
        rows[k, 0] = kind
        rows[k, 1:1 + len(a)] = a
    vs = [np.ascontiguousarray(V, np.float64).reshape(-1, 3) for V, _ in meshes]
    fs = [np.ascontiguousarray(F, np.int32).reshape(-1, 3) for _, F in meshes]
    vptr = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int32)
    fptr = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int32)
    vv = np.ascontiguousarray(np.concatenate(vs) if vs else np.zeros((1, 3)))
    ff = np.ascontiguousarray(np.concatenate(fs) if fs else np.zeros((1, 3), np.int32))
    q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    out = np.zeros_like(q)
    if poses is not None:
        if len(poses) != len(meshes):
            raise ValueError("hook_collision_prox: one pose (or None) per mesh")
        pp = np.full((max(len(meshes), 1), 12), np.nan)   # a row of NaNs: that mesh unposed
        for m, p in enumerate(poses):
            if p is not None:
                pp[m] = _pose_arg(p)
        _chk(lib().aa_test_collision_prox_posed(ctx.h, _dp(rows), C.c_int(len(obstacles)), _dp(vv), _ip(vptr), _ip(ff),
                                                _ip(fptr), C.c_int(len(meshes)), _dp(pp), _dp(q), C.c_int(q.shape[0]),
                                                _dp(out)))
        return out
    _chk(lib().aa_test_collision_prox(ctx.h, _dp(rows), C.c_int(len(obstacles)), _dp(vv), _ip(vptr), _ip(ff), _ip(fptr),
                                      C.c_int(len(meshes)), _dp(q), C.c_int(q.shape[0]), _dp(out)))
    return out


# script entries of aa_test_direct_solve (include/aa_admm.h)
(AA_SOLVE_B0, AA_SOLVE_B1, AA_SOLVE_BOTH, AA_SOLVE_GATED_SKIP_B0, AA_SOLVE_GATED_SKIP_B1, AA_SOLVE_GATED_TAKE_B0,
 AA_SOLVE_GATED_TAKE_B1, AA_SOLVE_DONE_B0, AA_SOLVE_DONE_B1) = range(9)
SOLVE_SENTINEL = -1.2345678901234567e+123   # what the output buffers hold before every script entry

# DirectSolver::PlanSummary (csrc/direct_solve.hpp), field by field
SOLVE_PLAN_FIELDS = (
    "supernodes", "levels", "fused_subtrees", "fused_supernodes", "sub_u", "sub_x",
    "fwd_tasks", "bwd_tasks", "fwd_tiles", "bwd_tiles", "fwd_tile_w", "bwd_tile_w",
    "fwd_streams", "bwd_streams", "stream_all", "stream_gated", "branches", "packed", "nt", "nt_rows",
    "row_p_min", "row_p_max", "row_R_min", "row_R_max", "tile_p_min", "tile_p_max", "tile_R_min", "tile_R_max",
    "fwd_row_nodes", "fwd_tile_nodes", "bwd_row_nodes", "bwd_tile_nodes", "fwd_row_bwd_tile_nodes",
    "fwd_tile_bwd_row_nodes", "multi_block_fwd_nodes", "odd_p_nodes", "sub_block", "wave_p", "wave_r", "max_sets",
)


class DirectSolveResult:
    """x[k] = (first, second) output buffer of script entry k, each (n, 3) in the caller's ordering
    (SOLVE_SENTINEL where the entry wrote nothing); x_host = factor_solve_host of (b0, b1) with the
    same factor; plan = the PlanSummary as a dict; height / depth = per node, of its supernode."""

    def __init__(self, x, x_host, plan, height, depth):
        self.x, self.x_host, self.plan, self.height, self.depth = x, x_host, plan, height, depth


def test_direct_solve(ctx: Context, A, xyz, b0, b1=None, script=(AA_SOLVE_B0,), tree=None, leaf_size=8, top_rows=0,
                      wave_p=192, wave_r=384, max_sets=1, wide=False, default_branches=1, device_factor=False):
    """aa_test_direct_solve: the GPU triangular solves alone on the SPD matrix A (scipy CSR, full
    symmetric pattern with the diagonal stored). tree = (beg, end, parent): an explicit supernode
    tree in postorder with the identity permutation; None: the library's nested dissection with
    leaf_size / top_rows. The AA_SOLVE_* / AA_SUB_* / AA_FACTOR_NT* knobs are read from the
    environment on every call."""
    A = A.tocsr()
    A.sort_indices()
    n = A.shape[0]
    ptr = np.ascontiguousarray(A.indptr, np.int32)
    col = np.ascontiguousarray(A.indices, np.int32)
    val = np.ascontiguousarray(A.data, np.float64)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(n, 3)
    b0 = np.ascontiguousarray(b0, np.float64).reshape(n, 3)
    if b1 is not None:
        b1 = np.ascontiguousarray(b1, np.float64).reshape(n, 3)
    sc = np.ascontiguousarray(script, np.int32).reshape(-1)
    if tree is not None:
        tb, te, tp = (np.ascontiguousarray(a, np.int32) for a in tree)
        nt = len(tb)
    else:
        tb = te = tp = np.zeros(1, np.int32)
        nt = 0
    x = np.zeros((max(len(sc), 1), 2, n, 3))
    xh = np.zeros((2, n, 3))
    info = np.zeros((n, 2), np.int32)
    plan = np.zeros(len(SOLVE_PLAN_FIELDS), np.int32)
    cnt = C.c_int()
    _chk(lib().aa_test_direct_solve(
        ctx.h, C.c_int(n), _dp(xyz), _ip(ptr), _ip(col), _dp(val), C.c_int(nt), _ip(tb), _ip(te), _ip(tp),
        C.c_int(leaf_size), C.c_int(top_rows), C.c_int(wave_p), C.c_int(wave_r), C.c_int(max_sets), C.c_int(int(wide)),
        C.c_int(default_branches), C.c_int(int(device_factor)), _dp(b0), _dp(b1) if b1 is not None else None,
        C.c_int(len(sc)), _ip(sc), C.c_double(SOLVE_SENTINEL), _dp(x), _dp(xh), _ip(info), _ip(plan),
        C.c_int(len(plan)), C.byref(cnt)))
    if cnt.value != len(SOLVE_PLAN_FIELDS):
        raise RuntimeError(f"PlanSummary has {cnt.value} fields, the binding names {len(SOLVE_PLAN_FIELDS)}")
    return DirectSolveResult([(x[k, 0], x[k, 1]) for k in range(len(sc))], (xh[0], xh[1] if b1 is not None else None),
                             dict(zip(SOLVE_PLAN_FIELDS, (int(v) for v in plan))), info[:, 0].copy(), info[:, 1].copy())


# flags of aa_test_anderson_step (include/aa_admm.h)
AA_STEP_COPY_TO, AA_STEP_INPLACE, AA_STEP_NARROW, AA_STEP_ROWS = 1, 2, 4, 8
ANDERSON_CTL = ("aa_iter", "aa_col", "aa_skip", "aa_active", "done", "aa_mk", "aa_j", "aa_jn", "aa_first")


def hook_anderson_step(ctx: Context, state, G, nblocks=0, copy_to=None, out=None, inplace=False, narrow=True, rows=False):
    """aa_test_anderson_step: one launch_aa_reduce -> launch_aa_solve -> launch_aa_mix on the state.

    state: dict with m, na, nb, eff, cur (dim), dF (m, eff), dG (m, dim) -- row c = history column
    c --, the ANDERSON_CTL ints, scale (m), M (m, m) with M[r, c] the device's M[c * m + r], coef (m),
    aa_s and mask = (lo1, hi1, lo2, hi2). out / copy_to: what the buffers hold on entry (None with
    inplace / without the copy). Returns a dict: the same keys after the step, plus red (blocks,
    2 + 2 bucket), out, copy_to (None where not used), bucket, nblocks and cols (1 / 0 / -1)."""
    m, na, nb, eff = int(state["m"]), int(state["na"]), int(state["nb"]), int(state["eff"])
    dim = na + nb
    G = np.ascontiguousarray(G, np.float64).reshape(-1)
    cur = np.array(state["cur"], np.float64).reshape(-1)
    dF = np.array(state["dF"], np.float64, order="C")
    dG = np.array(state["dG"], np.float64, order="C")
    ok = m >= 1 and len(G) == dim and len(cur) == dim and 0 < eff <= dim and dF.shape == (m, eff) and dG.shape == (m, dim)
    if not ok:
        raise ValueError("hook_anderson_step: array shapes do not fit m, na, nb, eff")
    ctl = np.array([state[k] for k in ANDERSON_CTL], np.int32)
    scale = np.array(state["scale"], np.float64).reshape(m)
    M = np.array(np.asarray(state["M"], np.float64).reshape(m, m).T, order="C")   # device: column-major
    coef = np.array(state["coef"], np.float64).reshape(m)
    aa_s = C.c_double(float(state["aa_s"]))
    mask = np.array(state["mask"], np.int64).reshape(4)
    flags = ((AA_STEP_COPY_TO if copy_to is not None else 0) | (AA_STEP_INPLACE if inplace else 0)
             | (AA_STEP_NARROW if narrow else 0) | (AA_STEP_ROWS if rows else 0))
    o = None if inplace else np.array(out, np.float64).reshape(dim)
    cp = None if copy_to is None else np.array(copy_to, np.float64).reshape(dim)
    cap = (nblocks if nblocks > 0 else max(1, (dim + 63) // 64)) * 66   # blocks hold at least a wave's rows
    red = np.zeros(cap)
    info = np.zeros(3, np.int32)
    _chk(lib().aa_test_anderson_step(
        ctx.h, C.c_int(m), C.c_longlong(na), C.c_longlong(nb), C.c_longlong(eff), _dp(G), _dp(cur), _dp(dF), _dp(dG),
        _ip(ctl), _dp(scale), _dp(M), _dp(coef), C.byref(aa_s), mask.ctypes.data_as(C.POINTER(C.c_longlong)),
        C.c_int(nblocks), C.c_int(flags), _dp(red), C.c_longlong(cap), None if o is None else _dp(o),
        None if cp is None else _dp(cp), _ip(info)))
    bucket, nbl = int(info[0]), int(info[1])
    res = dict(m=m, na=na, nb=nb, eff=eff, cur=cur, dF=dF, dG=dG, scale=scale, M=np.array(M.T, order="C"), coef=coef,
               aa_s=aa_s.value, mask=tuple(int(v) for v in mask), red=red[:nbl * (2 + 2 * bucket)].reshape(nbl, 2 + 2 * bucket).copy(),
               out=o, copy_to=cp, bucket=bucket, nblocks=nbl, cols=int(info[2]))
    res.update({k: int(v) for k, v in zip(ANDERSON_CTL, ctl)})
    return res
