"""Host-side mirror of the C ABI in include/sfgpu.h (ctypes; numpy arrays in, numpy arrays out).

`FluidSolver.vel_step()` / `.dens_step()` are the two entry points BASELINE.json's north_star names;
field names follow docs/SPEC.md. All numerics run in libsfgpu.so (hand-written gfx950 HIP); this
module has no fallback: if the library is missing the import fails, and if no MI355X is visible
`FluidSolver(...)` raises SfError(SF_ERR_NO_DEVICE).
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("SF_LIB", "libsfgpu.so"))  # SF_LIB: experimental builds
if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
lib = C.CDLL(LIB_PATH)

SF_OK, SF_ERR_INVALID, SF_ERR_HIP, SF_ERR_RCCL, SF_ERR_HALO_EXCEEDED, SF_ERR_NO_DEVICE, SF_ERR_TRACER_OVERFLOW = range(7)
SF_F32, SF_F64 = 0, 1
FIELD_IDS = {"u": 0, "v": 1, "w": 2, "u0": 3, "v0": 4, "w0": 5, "dens": 6, "dens0": 7,
             "user0": 8, "user1": 9, "user2": 10, "user3": 11}
FIELD_NAMES = ("u", "v", "w", "u0", "v0", "w0", "dens", "dens0")
NCCL_ID_BYTES = 128
SF_FLAG_LOOPBACK_HALO, SF_FLAG_RCCL_SELF = 1, 2
SF_ADVECT_SEMI_LAGRANGIAN, SF_ADVECT_MACCORMACK = 0, 1
SF_RED_SUM, SF_RED_SUM_SQ, SF_RED_MIN, SF_RED_MAX, SF_RED_MAX_ABS, SF_RED_COUNT_NONFINITE = range(6)
REDUCE_OPS = {"sum": SF_RED_SUM, "sum_sq": SF_RED_SUM_SQ, "min": SF_RED_MIN, "max": SF_RED_MAX,
              "max_abs": SF_RED_MAX_ABS, "count_nonfinite": SF_RED_COUNT_NONFINITE}
SF_PRESSURE_JACOBI, SF_PRESSURE_CG = 0, 1
PRESSURE_SOLVERS = {"jacobi": SF_PRESSURE_JACOBI, "cg": SF_PRESSURE_CG}
SF_PRECOND_NONE, SF_PRECOND_JACOBI = 0, 1
PRECONDITIONERS = {"none": SF_PRECOND_NONE, "jacobi": SF_PRECOND_JACOBI}
SF_CG_CONVERGED, SF_CG_MAX_ITERS, SF_CG_BREAKDOWN = 0, 1, 2
CG_STATUS = ("converged", "max_iters", "breakdown")
TRANSPORTS = ("none", "copy", "rccl", "rccl-self", "loopback")

# every symbol include/sfgpu.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = (
    "sf_version", "sf_status_string", "sf_nccl_unique_id", "sf_create", "sf_destroy", "sf_upload",
    "sf_download", "sf_download_planes", "sf_upload_planes", "sf_owned_planes", "sf_stored_planes", "sf_fill", "sf_copy_field", "vel_step",
    "dens_step", "sf_add_source", "sf_set_bnd", "sf_lin_solve", "sf_diffuse", "sf_advect", "sf_project",
    "sf_set_iters", "sf_set_coefficients", "sf_sync", "sf_last_error", "sf_timer_start", "sf_timer_stop",
    "sf_measure_copy_bandwidth", "sf_layout_info", "sf_schedule_info", "sf_lin_solve_launches", "sf_snapshot", "sf_snapshot_read",
    "sf_tracers_set", "sf_tracers_advect", "sf_tracers_get", "sf_bind_sources", "sf_transport_info", "sf_snapshot_read_planes",
    "sf_tracers_owned", "sf_tracers_get_owned", "sf_tracers_set_capacity",
    "sf_set_vorticity_confinement", "sf_set_buoyancy", "sf_vorticity_magnitude", "sf_add_forces",
    "sf_set_advection", "sf_advect_maccormack",
    "sf_reduce", "sf_diagnostics_get",
    "sf_set_pressure_solver", "sf_project_cg", "sf_poisson_residual", "sf_pressure_info_get",
    "sf_set_pressure_sync", "sf_pressure_sync_get",
    "sf_set_pressure_preconditioner", "sf_pressure_preconditioner_get",
    "sf_set_pressure_multigrid", "sf_pressure_multigrid_get", "sf_precondition",
    "sf_set_obstacles", "sf_obstacles_get",
    "sf_set_obstacle_multigrid", "sf_obstacle_multigrid_get", "sf_precondition_masked",
    "sf_set_obstacle_transport", "sf_obstacle_transport_get", "sf_diffuse_masked", "sf_advect_masked",
    "sf_set_obstacle_maccormack", "sf_obstacle_maccormack_get", "sf_advect_maccormack_masked",
    "sf_set_obstacle_velocity", "sf_obstacle_velocity_get",
    "sf_render", "sf_render_read", "sf_light",
    "sf_render_view", "sf_render_view_read", "sf_view_frame",
    "sf_render_camera", "sf_camera_passes_get", "sf_camera_frame",
)


class SfParams(C.Structure):
    _fields_ = [("N", C.c_int), ("dtype", C.c_int), ("iters", C.c_int), ("dt", C.c_double),
                ("diff", C.c_double), ("visc", C.c_double), ("device", C.c_int), ("nslabs_local", C.c_int),
                ("rank", C.c_int), ("nranks", C.c_int), ("nccl_id", C.c_void_p), ("flags", C.c_int)]


class SfDiagnostics(C.Structure):
    """sf_diagnostics of include/sfgpu.h (docs/SPEC.md §10)."""
    _fields_ = [(n, C.c_double) for n in ("mass", "dens_min", "dens_max", "kinetic", "max_speed", "max_div",
                                          "cfl_x", "cfl_y", "cfl_z", "cfl")] + [("nonfinite", C.c_longlong)]


class SfPressureInfo(C.Structure):
    """sf_pressure_info of include/sfgpu.h (docs/SPEC.md §11)."""
    _fields_ = [("solver", C.c_int), ("status", C.c_int), ("iterations", C.c_int), ("rel_residual", C.c_double),
                ("solves_total", C.c_longlong), ("iterations_total", C.c_longlong)]


class SfPressureSync(C.Structure):
    """sf_pressure_sync of include/sfgpu.h (docs/SPEC.md §11)."""
    _fields_ = [("check_every", C.c_int), ("host_waits", C.c_int), ("host_waits_total", C.c_longlong)]


class SfPressurePreconditioner(C.Structure):
    """sf_pressure_preconditioner of include/sfgpu.h (docs/SPEC.md §11.2)."""
    _fields_ = [("kind", C.c_int), ("sweeps", C.c_int)]


class SfPressureMultigrid(C.Structure):
    """sf_pressure_multigrid of include/sfgpu.h (docs/SPEC.md §11.3)."""
    _fields_ = [("sweeps", C.c_int), ("max_levels", C.c_int), ("coarse_sweeps", C.c_int), ("levels", C.c_int)]


class SfObstacles(C.Structure):
    """sf_obstacles of include/sfgpu.h (docs/SPEC.md §15)."""
    _fields_ = [("enabled", C.c_int), ("fluid_cells", C.c_longlong)]


class SfRenderParams(C.Structure):
    """sf_render_params of include/sfgpu.h (docs/SPEC.md §12)."""
    _fields_ = [("axis", C.c_int), ("from_high", C.c_int), ("sigma", C.c_double), ("dens", C.c_int), ("emit", C.c_int)]


class SfViewParams(C.Structure):
    """sf_view_params of include/sfgpu.h (docs/SPEC.md §13)."""
    _fields_ = [("origin", C.c_double * 3), ("du", C.c_double * 3), ("dv", C.c_double * 3), ("step", C.c_double * 3),
                ("width", C.c_int), ("height", C.c_int), ("samples", C.c_int), ("sigma", C.c_double),
                ("dens", C.c_int), ("emit", C.c_int)]


class SfCameraParams(C.Structure):
    """sf_camera_params of include/sfgpu.h (docs/SPEC.md §14)."""
    _fields_ = [("view", SfViewParams), ("step_du", C.c_double * 3), ("step_dv", C.c_double * 3)]


SF_CAMERA_UP, SF_CAMERA_DOWN, SF_CAMERA_BOTH = 0, 1, 2
CAMERA_PASSES = ("up", "down", "both")

_ctx = C.c_void_p
lib.sf_version.restype = C.c_char_p
lib.sf_status_string.restype = C.c_char_p
lib.sf_status_string.argtypes = [C.c_int]
lib.sf_last_error.restype = C.c_char_p
lib.sf_last_error.argtypes = [_ctx]
lib.sf_nccl_unique_id.argtypes = [C.c_void_p]
lib.sf_create.argtypes = [C.POINTER(_ctx), C.POINTER(SfParams)]
lib.sf_destroy.argtypes = [_ctx]
lib.sf_destroy.restype = None
lib.sf_upload.argtypes = [_ctx, C.c_int, C.c_void_p]
lib.sf_download.argtypes = [_ctx, C.c_int, C.c_void_p]
lib.sf_download_planes.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p]
lib.sf_upload_planes.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p]
lib.sf_owned_planes.argtypes = [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.sf_stored_planes.argtypes = [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.sf_fill.argtypes = [_ctx, C.c_int, C.c_double]
lib.sf_copy_field.argtypes = [_ctx, C.c_int, C.c_int]
lib.vel_step.argtypes = [_ctx]
lib.dens_step.argtypes = [_ctx]
lib.sf_add_source.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_set_bnd.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_lin_solve.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
lib.sf_diffuse.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_double]
lib.sf_advect.argtypes = [_ctx] + [C.c_int] * 6
lib.sf_project.argtypes = [_ctx] + [C.c_int] * 5
lib.sf_vorticity_magnitude.argtypes = [_ctx] + [C.c_int] * 4
lib.sf_add_forces.argtypes = [_ctx] + [C.c_int] * 7
lib.sf_set_vorticity_confinement.argtypes = [_ctx, C.c_double]
lib.sf_set_buoyancy.argtypes = [_ctx, C.c_double, C.c_double, C.c_int]
lib.sf_set_advection.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_advect_maccormack.argtypes = [_ctx] + [C.c_int] * 6
lib.sf_reduce.argtypes = [_ctx, C.c_int, C.c_int, C.POINTER(C.c_double)]
lib.sf_diagnostics_get.argtypes = [_ctx, C.POINTER(SfDiagnostics)]
lib.sf_set_pressure_solver.argtypes = [_ctx, C.c_int, C.c_double, C.c_int]
lib.sf_project_cg.argtypes = [_ctx] + [C.c_int] * 5 + [C.c_double, C.c_int]
lib.sf_poisson_residual.argtypes = [_ctx, C.c_int, C.c_int, C.POINTER(C.c_double)]
lib.sf_pressure_info_get.argtypes = [_ctx, C.POINTER(SfPressureInfo)]
lib.sf_set_pressure_sync.argtypes = [_ctx, C.c_int]
lib.sf_pressure_sync_get.argtypes = [_ctx, C.POINTER(SfPressureSync)]
lib.sf_set_pressure_preconditioner.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_pressure_preconditioner_get.argtypes = [_ctx, C.POINTER(SfPressurePreconditioner)]
lib.sf_set_pressure_multigrid.argtypes = [_ctx, C.c_int, C.c_int, C.c_int]
lib.sf_pressure_multigrid_get.argtypes = [_ctx, C.POINTER(SfPressureMultigrid)]
lib.sf_precondition.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_set_obstacles.argtypes = [_ctx, C.c_int]
lib.sf_obstacles_get.argtypes = [_ctx, C.POINTER(SfObstacles)]
lib.sf_set_obstacle_multigrid.argtypes = [_ctx, C.c_int]
lib.sf_obstacle_multigrid_get.argtypes = [_ctx, C.POINTER(C.c_int)]
lib.sf_precondition_masked.argtypes = [_ctx, C.c_int, C.c_int]
lib.sf_set_obstacle_transport.argtypes = [_ctx, C.c_int]
lib.sf_obstacle_transport_get.argtypes = [_ctx, C.POINTER(C.c_int)]
lib.sf_diffuse_masked.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_double]
lib.sf_advect_masked.argtypes = [_ctx] + [C.c_int] * 6
lib.sf_set_obstacle_maccormack.argtypes = [_ctx, C.c_int]
lib.sf_obstacle_maccormack_get.argtypes = [_ctx, C.POINTER(C.c_int)]
lib.sf_set_obstacle_velocity.argtypes = [_ctx, C.c_int, C.c_int, C.c_int]
lib.sf_obstacle_velocity_get.argtypes = [_ctx, C.POINTER(C.c_int)]
lib.sf_advect_maccormack_masked.argtypes = [_ctx] + [C.c_int] * 6
lib.sf_render.argtypes = [_ctx, C.POINTER(SfRenderParams)]
lib.sf_render_read.argtypes = [_ctx, C.c_void_p, C.c_void_p]
lib.sf_light.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
lib.sf_render_view.argtypes = [_ctx, C.POINTER(SfViewParams)]
lib.sf_render_view_read.argtypes = [_ctx, C.c_void_p, C.c_void_p]
lib.sf_view_frame.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double,
                              C.c_double, C.POINTER(SfViewParams)]
lib.sf_render_camera.argtypes = [_ctx, C.POINTER(SfCameraParams)]
lib.sf_camera_passes_get.argtypes = [C.POINTER(SfCameraParams), C.c_int, C.POINTER(C.c_int)]
lib.sf_camera_frame.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(SfCameraParams)]
lib.sf_set_iters.argtypes = [_ctx, C.c_int]
lib.sf_set_coefficients.argtypes = [_ctx, C.c_double, C.c_double, C.c_double]
lib.sf_sync.argtypes = [_ctx]
lib.sf_timer_start.argtypes = [_ctx]
lib.sf_timer_stop.argtypes = [_ctx, C.POINTER(C.c_float)]
lib.sf_measure_copy_bandwidth.argtypes = [_ctx, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
lib.sf_lin_solve_launches.argtypes = [_ctx, C.c_int]
lib.sf_bind_sources.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_int]
lib.sf_snapshot.argtypes = [_ctx, C.POINTER(C.c_int), C.c_int]
lib.sf_snapshot_read.argtypes = [_ctx, C.c_int, C.c_void_p]
lib.sf_snapshot_read_planes.argtypes = [_ctx, C.c_int, C.c_int, C.c_int, C.c_void_p]
lib.sf_tracers_set.argtypes = [_ctx, C.c_int, C.c_void_p]
lib.sf_tracers_advect.argtypes = [_ctx]
lib.sf_tracers_get.argtypes = [_ctx, C.c_void_p, C.c_void_p, C.c_void_p]
lib.sf_tracers_owned.argtypes = [_ctx, C.POINTER(C.c_int)]
lib.sf_tracers_get_owned.argtypes = [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.sf_tracers_set_capacity.argtypes = [_ctx, C.c_int]
lib.sf_layout_info.argtypes = [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
lib.sf_schedule_info.argtypes = [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.sf_transport_info.argtypes = [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_long)]


class SfError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{lib.sf_status_string(status).decode()}: {message}")
        self.status = status


def version():
    return lib.sf_version().decode()


def nccl_unique_id():
    buf = C.create_string_buffer(NCCL_ID_BYTES)
    rc = lib.sf_nccl_unique_id(buf)
    if rc != SF_OK:
        raise SfError(rc, "ncclGetUniqueId failed")
    return buf.raw


def _fid(f):
    return FIELD_IDS[f] if isinstance(f, str) else int(f)


class FluidSolver:
    """One context of libsfgpu.so. Arrays are (N+2,N+2,N+2) numpy arrays indexed [k, j, i]
    (C order, i fastest), i.e. exactly the dense IX(i,j,k) layout of docs/SPEC.md."""

    def __init__(self, N, dtype="f32", iters=20, dt=0.1, diff=1e-4, visc=1e-4, device=0, nslabs_local=1,
                 rank=0, nranks=1, nccl_id=None, flags=0):
        self.N = int(N)
        self.np_dtype = np.float32 if dtype in ("f32", np.float32, SF_F32) else np.float64
        self._id_buf = C.create_string_buffer(nccl_id, NCCL_ID_BYTES) if nccl_id is not None else None
        p = SfParams(N=self.N, dtype=SF_F32 if self.np_dtype == np.float32 else SF_F64, iters=int(iters),
                     dt=float(dt), diff=float(diff), visc=float(visc), device=int(device),
                     nslabs_local=int(nslabs_local), rank=int(rank), nranks=int(nranks),
                     nccl_id=C.cast(self._id_buf, C.c_void_p) if self._id_buf is not None else None, flags=int(flags))
        self._h = _ctx()
        rc = lib.sf_create(C.byref(self._h), C.byref(p))
        if rc != SF_OK:
            self._h = None
            raise SfError(rc, lib.sf_last_error(None).decode())

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib.sf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc != SF_OK:
            raise SfError(rc, lib.sf_last_error(self._h).decode())

    # -- data ------------------------------------------------------------------------------
    @property
    def shape(self):
        return (self.N + 2,) * 3

    def upload(self, field, array):
        a = np.ascontiguousarray(array, dtype=self.np_dtype)
        if a.shape != self.shape:
            raise ValueError(f"expected shape {self.shape}, got {a.shape}")
        self._ck(lib.sf_upload(self._h, _fid(field), a.ctypes.data_as(C.c_void_p)))

    def download(self, field, out=None):
        if out is None:
            out = np.zeros(self.shape, self.np_dtype)
        assert out.dtype == self.np_dtype and out.shape == self.shape and out.flags.c_contiguous
        self._ck(lib.sf_download(self._h, _fid(field), out.ctypes.data_as(C.c_void_p)))
        return out

    def download_planes(self, field, k_begin, k_end):
        out = np.zeros((k_end - k_begin, self.N + 2, self.N + 2), self.np_dtype)
        self._ck(lib.sf_download_planes(self._h, _fid(field), int(k_begin), int(k_end),
                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def upload_planes(self, field, k_begin, array):
        a = np.ascontiguousarray(array, dtype=self.np_dtype)
        if a.ndim != 3 or a.shape[1:] != (self.N + 2, self.N + 2):
            raise ValueError(f"expected shape (nplanes,{self.N + 2},{self.N + 2}), got {a.shape}")
        self._ck(lib.sf_upload_planes(self._h, _fid(field), int(k_begin), int(k_begin) + a.shape[0],
                                      a.ctypes.data_as(C.c_void_p)))

    def stored_planes(self):
        """Global planes this context stores: its interior planes plus its ghost / shell planes."""
        kb, ke = C.c_int(), C.c_int()
        self._ck(lib.sf_stored_planes(self._h, C.byref(kb), C.byref(ke)))
        return kb.value, ke.value

    def owned_planes(self):
        kb, ke = C.c_int(), C.c_int()
        self._ck(lib.sf_owned_planes(self._h, C.byref(kb), C.byref(ke)))
        return kb.value, ke.value

    def fill(self, field, value):
        self._ck(lib.sf_fill(self._h, _fid(field), float(value)))

    def copy_field(self, dst, src):
        self._ck(lib.sf_copy_field(self._h, _fid(dst), _fid(src)))

    def bind_sources(self, su="user0", sv="user1", sw="user2", sd="user3"):
        ids = [(-1 if f is None else _fid(f)) for f in (su, sv, sw, sd)]
        self._ck(lib.sf_bind_sources(self._h, *ids))

    # -- the path --------------------------------------------------------------------------
    def vel_step(self):
        self._ck(lib.vel_step(self._h))

    def dens_step(self):
        self._ck(lib.dens_step(self._h))

    def add_source(self, x, s):
        self._ck(lib.sf_add_source(self._h, _fid(x), _fid(s)))

    def set_bnd(self, b, x):
        self._ck(lib.sf_set_bnd(self._h, int(b), _fid(x)))

    def lin_solve(self, b, x, x0, a, c, iters):
        self._ck(lib.sf_lin_solve(self._h, int(b), _fid(x), _fid(x0), float(a), float(c), int(iters)))

    def diffuse(self, b, x, x0, diff):
        self._ck(lib.sf_diffuse(self._h, int(b), _fid(x), _fid(x0), float(diff)))

    def advect(self, b, d, d0, u, v, w):
        self._ck(lib.sf_advect(self._h, int(b), _fid(d), _fid(d0), _fid(u), _fid(v), _fid(w)))

    def project(self, u, v, w, p, div):
        self._ck(lib.sf_project(self._h, _fid(u), _fid(v), _fid(w), _fid(p), _fid(div)))

    # -- external forces (docs/SPEC.md §8) ---------------------------------------------------
    def set_vorticity_confinement(self, eps):
        """Vorticity confinement strength applied by vel_step (0 = off, the default)."""
        self._ck(lib.sf_set_vorticity_confinement(self._h, float(eps)))

    def set_buoyancy(self, beta, ambient=0.0, axis=1):
        """Buoyancy beta*(dens - ambient) on velocity component `axis` (0 = u, 1 = v, 2 = w) in vel_step (beta 0 = off)."""
        self._ck(lib.sf_set_buoyancy(self._h, float(beta), float(ambient), int(axis)))

    def vorticity_magnitude(self, u, v, w, dst):
        self._ck(lib.sf_vorticity_magnitude(self._h, _fid(u), _fid(v), _fid(w), _fid(dst)))

    def add_forces(self, u, v, w, dens, su, sv, sw):
        self._ck(lib.sf_add_forces(self._h, _fid(u), _fid(v), _fid(w), _fid(dens), _fid(su), _fid(sv), _fid(sw)))

    # -- MacCormack advection (docs/SPEC.md §9) -----------------------------------------------
    def set_advection(self, velocity=SF_ADVECT_SEMI_LAGRANGIAN, density=SF_ADVECT_SEMI_LAGRANGIAN):
        """Advection scheme of vel_step / dens_step: SF_ADVECT_SEMI_LAGRANGIAN (the default) or SF_ADVECT_MACCORMACK."""
        self._ck(lib.sf_set_advection(self._h, int(velocity), int(density)))

    def advect_maccormack(self, b, d, d0, u, v, w):
        self._ck(lib.sf_advect_maccormack(self._h, int(b), _fid(d), _fid(d0), _fid(u), _fid(v), _fid(w)))

    # -- reductions and diagnostics (docs/SPEC.md §10) ----------------------------------------
    def reduce(self, op, field):
        """One deterministic reduction over the interior cells of a field slot, as a float (a double's bits are those
        of the SPEC for every decomposition). op: an SF_RED_* value or "sum", "sum_sq", "min", "max", "max_abs",
        "count_nonfinite". Collective on several ranks; synchronises."""
        out = C.c_double()
        self._ck(lib.sf_reduce(self._h, REDUCE_OPS[op] if isinstance(op, str) else int(op), _fid(field), C.byref(out)))
        return out.value

    def diagnostics(self):
        """State diagnostics of u, v, w, dens as a dict: mass, dens_min, dens_max, kinetic, max_speed, max_div, cfl_x,
        cfl_y, cfl_z, cfl (floats) and nonfinite (int). Collective on several ranks; synchronises."""
        d = SfDiagnostics()
        self._ck(lib.sf_diagnostics_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfDiagnostics._fields_}

    # -- conjugate-gradient projection (docs/SPEC.md §11) --------------------------------------
    def set_pressure_solver(self, solver="jacobi", tol=1e-3, max_iters=100):
        """What vel_step's two projections run: "jacobi" (the default: K sweeps, the §3 step exactly) or "cg" (until
        the recurrence residual is <= tol * its initial value, at most max_iters iterations)."""
        sid = PRESSURE_SOLVERS[solver] if isinstance(solver, str) else int(solver)
        self._ck(lib.sf_set_pressure_solver(self._h, sid, float(tol), int(max_iters)))

    def project_cg(self, u, v, w, p, div, tol=1e-3, max_iters=100):
        """SPEC §11 project_cg; returns pressure_info() of this solve. Collective on several ranks; synchronises."""
        self._ck(lib.sf_project_cg(self._h, _fid(u), _fid(v), _fid(w), _fid(p), _fid(div), float(tol), int(max_iters)))
        return self.pressure_info()

    def poisson_residual(self, p, div):
        """||div - A p|| / ||div|| of what either solver left in the slots p and div (0 for a zero div)."""
        out = C.c_double()
        self._ck(lib.sf_poisson_residual(self._h, _fid(p), _fid(div), C.byref(out)))
        return out.value

    def pressure_info(self):
        """The last projection of either kind: solver, status (SF_CG_*), iterations, rel_residual, and the totals."""
        d = SfPressureInfo()
        self._ck(lib.sf_pressure_info_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfPressureInfo._fields_}

    def set_pressure_sync(self, check_every=0):
        """Where a CG solve keeps alpha, beta and its stop tests: 0 (the default) on the host, two waits per iteration;
        m >= 1 on the device, the host reading the state once per m enqueued iterations. The same bits either way."""
        self._ck(lib.sf_set_pressure_sync(self._h, int(check_every)))

    @property
    def pressure_sync(self):
        """check_every, and the host waits of the last CG projection and of all of them (sf_pressure_sync_get)."""
        d = SfPressureSync()
        self._ck(lib.sf_pressure_sync_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfPressureSync._fields_}

    def set_pressure_preconditioner(self, kind="none", sweeps=0):
        """The preconditioner of the CG solve (SPEC §11.2): "none" (the default: §11 exactly) or "jacobi" with
        sweeps = m >= 1 undamped Jacobi sweeps from zero as z = M(r). An even m needs about sqrt(2 m) times fewer
        iterations; the stop test stays on r.r."""
        kid = PRECONDITIONERS[kind] if isinstance(kind, str) else int(kind)
        self._ck(lib.sf_set_pressure_preconditioner(self._h, kid, int(sweeps)))

    @property
    def pressure_preconditioner(self):
        """kind (SF_PRECOND_*) and sweeps as last set (sf_pressure_preconditioner_get)."""
        d = SfPressurePreconditioner()
        self._ck(lib.sf_pressure_preconditioner_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfPressurePreconditioner._fields_}

    def set_pressure_multigrid(self, sweeps, max_levels=0, coarse_sweeps=8):
        """The multigrid preconditioner of the CG solve (SPEC §11.3): sweeps = nu >= 1 puts one symmetric V-cycle per
        iteration in force (nu damped-Jacobi sweeps before and after each coarse-grid correction, coarse_sweeps on the
        coarsest level, at most max_levels levels; 0: as many as N allows); sweeps = 0 switches it off again and the
        setting of set_pressure_preconditioner, kept meanwhile, applies."""
        self._ck(lib.sf_set_pressure_multigrid(self._h, int(sweeps), int(max_levels), int(coarse_sweeps)))

    @property
    def pressure_multigrid(self):
        """sweeps, max_levels and coarse_sweeps as last set, and levels, the depth of the hierarchy for this N
        (sf_pressure_multigrid_get)."""
        d = SfPressureMultigrid()
        self._ck(lib.sf_pressure_multigrid_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfPressureMultigrid._fields_}

    def precondition(self, z, r):
        """z = M(r) with the preconditioner in force (the V-cycle of §11.3, else the Jacobi sweeps of §11.2): r is read
        on interior cells, z is written whole."""
        self._ck(lib.sf_precondition(self._h, _fid(z), _fid(r)))

    # -- solid obstacles (docs/SPEC.md §15) --------------------------------------------------------
    def set_obstacles(self, mask, slot="user3"):
        """Solid cells for the CG projection, vel_step and dens_step: an interior cell is solid iff its mask value is
        > 0. mask: None switches obstacles off; a field name or id takes the mask that slot holds; an (N+2)^3 array is
        uploaded into `slot` first, over what the slot holds (the slot is free again afterwards: the mask is read once,
        by this call; name a slot that is scratch at that moment where user3 is a bound source).
        Collective on several ranks; synchronises."""
        if mask is None:
            self._ck(lib.sf_set_obstacles(self._h, -1))
            return
        if isinstance(mask, (str, int)):
            slot = mask
        else:
            self.upload(slot, mask)
        self._ck(lib.sf_set_obstacles(self._h, _fid(slot)))

    def obstacles(self):
        """enabled (0 / 1) and fluid_cells, the fluid interior cells of the whole grid (sf_obstacles_get)."""
        d = SfObstacles()
        self._ck(lib.sf_obstacles_get(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in SfObstacles._fields_}

    # -- obstacle-aware multigrid (docs/SPEC.md §16) ------------------------------------------------
    def set_obstacle_multigrid(self, on):
        """on = True: a masked solve with the V-cycle in force runs the masked V-cycle of §16 (coarse cells solid iff all
        eight children are) instead of being refused; False (the default) keeps the refusal. Valid in any order with
        set_obstacles and set_pressure_multigrid. Collective on several ranks; synchronises."""
        self._ck(lib.sf_set_obstacle_multigrid(self._h, 1 if on else 0))

    def obstacle_multigrid(self):
        """The setting of set_obstacle_multigrid (sf_obstacle_multigrid_get)."""
        on = C.c_int(0)
        self._ck(lib.sf_obstacle_multigrid_get(self._h, C.byref(on)))
        return bool(on.value)

    def precondition_masked(self, z, r):
        """z = V_m(0, r), the masked V-cycle of §16 singly: needs obstacles, the V-cycle and set_obstacle_multigrid(True).
        r is read on interior cells (solid cells never), z is written whole."""
        self._ck(lib.sf_precondition_masked(self._h, _fid(z), _fid(r)))

    # -- mask-aware transport (docs/SPEC.md §17) ------------------------------------------------------
    def set_obstacle_transport(self, on):
        """on = True: with obstacles on, the diffuse and advect of vel_step and dens_step are the masked forms of §17
        (nothing leaks into a solid; dens_step no longer zeroes the solids at its end); False (the default) keeps the
        steps of §15. A step advected with MacCormack is refused while it is on. Valid in any order with
        set_obstacles. Collective on several ranks; synchronises."""
        self._ck(lib.sf_set_obstacle_transport(self._h, int(on) if isinstance(on, int) else (1 if on else 0)))

    def obstacle_transport(self):
        """The setting of set_obstacle_transport (sf_obstacle_transport_get)."""
        on = C.c_int(0)
        self._ck(lib.sf_obstacle_transport_get(self._h, C.byref(on)))
        return bool(on.value)

    def diffuse_masked(self, b, x, x0, diff):
        """diffuse under the mask (§17 diffuse_masked): needs obstacles and set_obstacle_transport(True)."""
        self._ck(lib.sf_diffuse_masked(self._h, int(b), _fid(x), _fid(x0), float(diff)))

    def advect_masked(self, b, d, d0, u, v, w):
        """advect under the mask (§17 advect_masked): needs obstacles and set_obstacle_transport(True)."""
        self._ck(lib.sf_advect_masked(self._h, int(b), _fid(d), _fid(d0), _fid(u), _fid(v), _fid(w)))

    # -- MacCormack under the mask (docs/SPEC.md §18) -------------------------------------------------
    def set_obstacle_maccormack(self, on):
        """on = True: with obstacles and set_obstacle_transport on, a step advected with MacCormack runs the masked
        MacCormack of §18 instead of being refused; False (the default) keeps the refusal. No effect without obstacles
        or without the transport setting. Valid in any order with set_obstacles, set_obstacle_transport and
        set_advection. Collective on several ranks; synchronises."""
        self._ck(lib.sf_set_obstacle_maccormack(self._h, int(on) if isinstance(on, int) else (1 if on else 0)))

    def obstacle_maccormack(self):
        """The setting of set_obstacle_maccormack (sf_obstacle_maccormack_get)."""
        on = C.c_int(0)
        self._ck(lib.sf_obstacle_maccormack_get(self._h, C.byref(on)))
        return bool(on.value)

    def advect_maccormack_masked(self, b, d, d0, u, v, w):
        """MacCormack advect under the mask (§18 advect_mc_masked): needs obstacles and set_obstacle_transport(True)."""
        self._ck(lib.sf_advect_maccormack_masked(self._h, int(b), _fid(d), _fid(d0), _fid(u), _fid(v), _fid(w)))

    # -- moving solids (docs/SPEC.md §19) -----------------------------------------------------------------
    def set_obstacle_velocity(self, us, vs, ws, slots=("user0", "user1", "user2")):
        """The velocity of the solids, one field per axis, of which only the values in interior solid cells are used.
        All three None switch it off; field names or ids take what those slots hold; (N+2)^3 arrays are uploaded into
        `slots` first, over what they hold: the default slots are the ones bind_sources binds by default, so name
        slots that are scratch at that moment (("u0", "v0", "w0") between steps) where sources are bound. The three
        fields are copied by this call, so the slots are free again afterwards. While it is set (and obstacles are on) project_cg, diffuse_masked, advect_masked and vel_step follow
        §19; vel_step then needs set_obstacle_transport(True) and a first-order velocity advection. Collective on
        several ranks; synchronises."""
        vals = (us, vs, ws)
        if all(v is None for v in vals):
            self._ck(lib.sf_set_obstacle_velocity(self._h, -1, -1, -1))
            return
        ids = []
        for v, slot in zip(vals, slots):
            if v is None:
                ids.append(-1)  # a mix of None and fields: the library refuses it
            elif isinstance(v, (str, int)):
                ids.append(_fid(v))
            else:
                self.upload(slot, v)
                ids.append(_fid(slot))
        self._ck(lib.sf_set_obstacle_velocity(self._h, *ids))

    def obstacle_velocity(self):
        """True while a solid velocity is set (sf_obstacle_velocity_get)."""
        on = C.c_int(0)
        self._ck(lib.sf_obstacle_velocity_get(self._h, C.byref(on)))
        return bool(on.value)

    # -- volume rendering and light marching (docs/SPEC.md §12) ---------------------------------
    def render(self, dens="dens", emit=None, axis=2, from_high=0, sigma=1.0):
        """One ray per pixel along axis (0: i, 1: j, 2: k), entering at index 1 (from_high = 0) or N (1), through the
        density slot `dens` with opacity sigma * h * dens per cell and the emission slot `emit` (None: none). Returns
        (colour, transmittance): two (N, N) arrays indexed [b - 1, a - 1] over the two remaining axes a < b, zeros
        where this context holds no pixel. Collective on several ranks; waits for the image."""
        p = SfRenderParams(axis=int(axis), from_high=int(from_high), sigma=float(sigma), dens=_fid(dens),
                           emit=-1 if emit is None else _fid(emit))
        self._ck(lib.sf_render(self._h, C.byref(p)))
        colour = np.zeros((self.N, self.N), self.np_dtype)
        trans = np.zeros((self.N, self.N), self.np_dtype)
        self._ck(lib.sf_render_read(self._h, colour.ctypes.data_as(C.c_void_p), trans.ctypes.data_as(C.c_void_p)))
        return colour, trans

    def light(self, dst, dens="dens", axis=1, from_high=1, sigma=1.0):
        """dst = the transmittance of the ray along axis in front of every cell (1 on the first cell visited), then
        set_bnd(0, dst): what render takes as `emit` for self-shadowed smoke. dst must not be dens."""
        self._ck(lib.sf_light(self._h, _fid(dst), _fid(dens), int(axis), int(from_high), float(sigma)))

    # -- orthographic volume rendering from any direction (docs/SPEC.md §13) ----------------------
    def view_frame(self, dir, up=(0.0, 0.0, 1.0), width=256, height=256, step=1.0, sigma=1.0):
        """The SfViewParams of sf_view_frame for this grid: a width x height image looking along `dir` ((x, y, z) =
        (i, j, k)) with `up` as the vertical, samples `step` cells apart, extinction `sigma` per unit length."""
        f = SfViewParams()
        st = lib.sf_view_frame(self.N, (C.c_double * 3)(*map(float, dir)), (C.c_double * 3)(*map(float, up)), int(width),
                               int(height), float(step), float(sigma), C.byref(f))
        if st != SF_OK:
            raise SfError(st, "sf_view_frame: a zero or non-finite dir, up parallel to dir, step not > 0 or too small, "
                              "sigma < 0, or width / height outside 1 .. 16384")
        return f

    def render_view(self, frame, dens="dens", emit=None):
        """One ray per pixel of the frame (an SfViewParams: view_frame, or filled by hand) through the density slot
        `dens` and the emission slot `emit` (None: none), trilinear samples composited front to back. Returns (colour,
        transmittance), each shaped (height, width); zeros where this context does not hold the image. Collective on
        several ranks; waits for the image."""
        p = SfViewParams.from_buffer_copy(frame)
        p.dens = _fid(dens)
        p.emit = -1 if emit is None else _fid(emit)
        self._ck(lib.sf_render_view(self._h, C.byref(p)))
        colour = np.zeros((p.height, p.width), self.np_dtype)
        trans = np.zeros((p.height, p.width), self.np_dtype)
        self._ck(lib.sf_render_view_read(self._h, colour.ctypes.data_as(C.c_void_p), trans.ctypes.data_as(C.c_void_p)))
        return colour, trans

    # -- perspective volume rendering (docs/SPEC.md §14) ------------------------------------------
    def camera_frame(self, eye, target, up=(0.0, 0.0, 1.0), fov_y_deg=40.0, width=256, height=256, step=1.0, sigma=1.0):
        """The SfCameraParams of sf_camera_frame for this grid: a pinhole camera at `eye` looking at `target` ((x, y, z)
        = (i, j, k), the centre of cell i at x = i) with `up` as the vertical and a vertical field of view of fov_y_deg
        degrees, samples `step` cells apart in depth, extinction `sigma` per cell length."""
        f = SfCameraParams()
        vec = lambda v: (C.c_double * 3)(*map(float, v))
        st = lib.sf_camera_frame(self.N, vec(eye), vec(target), vec(up), math.tan(math.radians(float(fov_y_deg)) / 2.0),
                                 int(width), int(height), float(step), float(sigma), C.byref(f))
        if st != SF_OK:
            raise SfError(st, "sf_camera_frame: eye == target, up parallel to the direction, a field of view or step not "
                              "> 0, the box behind the camera, too many samples, sigma < 0, or width / height outside "
                              "1 .. 16384")
        return f

    def camera_passes(self, frame):
        """Which chains render_camera runs for the frame in this context's dtype: "up", "down" or "both"."""
        out = C.c_int()
        p = SfCameraParams.from_buffer_copy(frame)
        st = lib.sf_camera_passes_get(C.byref(p), SF_F32 if self.np_dtype == np.float32 else SF_F64, C.byref(out))
        if st != SF_OK:
            raise SfError(st, "sf_camera_passes_get: a corner pixel's step vector or origin is not finite")
        return CAMERA_PASSES[out.value]

    def render_camera(self, frame, dens="dens", emit=None):
        """One ray per pixel of the frame (an SfCameraParams: camera_frame, or filled by hand), as render_view with a
        step vector per pixel. Returns (colour, transmittance), each shaped (height, width); zeros where this context
        does not hold the image. Collective on several ranks; waits for the image."""
        p = SfCameraParams.from_buffer_copy(frame)
        p.view.dens = _fid(dens)
        p.view.emit = -1 if emit is None else _fid(emit)
        self._ck(lib.sf_render_camera(self._h, C.byref(p)))
        colour = np.zeros((p.view.height, p.view.width), self.np_dtype)
        trans = np.zeros((p.view.height, p.view.width), self.np_dtype)
        self._ck(lib.sf_render_view_read(self._h, colour.ctypes.data_as(C.c_void_p), trans.ctypes.data_as(C.c_void_p)))
        return colour, trans

    def set_iters(self, iters):
        self._ck(lib.sf_set_iters(self._h, int(iters)))

    def set_coefficients(self, dt, diff, visc):
        self._ck(lib.sf_set_coefficients(self._h, float(dt), float(diff), float(visc)))

    def sync(self):
        self._ck(lib.sf_sync(self._h))

    # -- measurement -----------------------------------------------------------------------
    def timer_start(self):
        self._ck(lib.sf_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        self._ck(lib.sf_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def copy_bandwidth_gbps(self, nbytes=1 << 30, reps=5):
        g = C.c_double()
        self._ck(lib.sf_measure_copy_bandwidth(self._h, int(nbytes), int(reps), C.byref(g)))
        return g.value

    # -- asynchronous output / tracers ------------------------------------------------------
    def snapshot(self, fields):
        ids = (C.c_int * len(fields))(*[_fid(f) for f in fields])
        self._ck(lib.sf_snapshot(self._h, ids, len(fields)))

    def snapshot_read(self, index, out=None):
        if out is None:
            out = np.zeros(self.shape, self.np_dtype)
        rc = lib.sf_snapshot_read(self._h, int(index), out.ctypes.data_as(C.c_void_p))
        if rc != SF_OK:
            raise SfError(rc, "sf_snapshot_read failed")
        return out

    def snapshot_read_planes(self, index, k_begin, k_end):
        out = np.zeros((k_end - k_begin, self.N + 2, self.N + 2), self.np_dtype)
        rc = lib.sf_snapshot_read_planes(self._h, int(index), int(k_begin), int(k_end), out.ctypes.data_as(C.c_void_p))
        if rc != SF_OK:
            raise SfError(rc, "sf_snapshot_read_planes failed")
        return out

    def tracers_set(self, xyz):
        a = np.ascontiguousarray(xyz, dtype=self.np_dtype).reshape(-1, 3)
        self._ntr = a.shape[0]
        self._ck(lib.sf_tracers_set(self._h, self._ntr, a.ctypes.data_as(C.c_void_p)))

    def tracers_advect(self):
        self._ck(lib.sf_tracers_advect(self._h))

    def tracers_get(self, sample=True):
        n = getattr(self, "_ntr", 0)
        xyz = np.zeros((n, 3), self.np_dtype)
        dens = np.zeros(n, self.np_dtype)
        speed = np.zeros(n, self.np_dtype)
        self._ck(lib.sf_tracers_get(self._h, xyz.ctypes.data_as(C.c_void_p),
                                    dens.ctypes.data_as(C.c_void_p) if sample else None,
                                    speed.ctypes.data_as(C.c_void_p) if sample else None))
        return xyz, dens, speed

    def tracers_owned(self):
        """Tracers this context holds now (all of them on one slab or one rank)."""
        n = C.c_int()
        self._ck(lib.sf_tracers_owned(self._h, C.byref(n)))
        return n.value

    def tracers_get_owned(self, sample=True):
        """This context's tracers in ascending id order: (ids, xyz, dens, speed); dens / speed are zeros when
        sample is False."""
        n = self.tracers_owned()
        ids = np.zeros(n, np.int32)
        xyz = np.zeros((n, 3), self.np_dtype)
        dens = np.zeros(n, self.np_dtype)
        speed = np.zeros(n, self.np_dtype)
        self._ck(lib.sf_tracers_get_owned(self._h, ids.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p),
                                          dens.ctypes.data_as(C.c_void_p) if sample else None,
                                          speed.ctypes.data_as(C.c_void_p) if sample else None))
        return ids, xyz, dens, speed

    def tracers_set_capacity(self, per_direction):
        """Most tracers one slab may hand to one neighbour per tracers_advect (default: the tracer count)."""
        self._ck(lib.sf_tracers_set_capacity(self._h, int(per_direction)))

    def lin_solve_launches(self, iters):
        return int(lib.sf_lin_solve_launches(self._h, int(iters)))

    def schedule_info(self):
        trap, measured = C.c_int(), C.c_int()
        self._ck(lib.sf_schedule_info(self._h, C.byref(trap), C.byref(measured)))
        m = measured.value
        return {"trapezoid_pairs": trap.value, "measured": bool(m & 1), "fields_measured": bool(m & 2),
                "fields_per_launch": 3 if (m & 4) else 1}

    def transport_info(self):
        """Halo transport of this context and how many RCCL send/recv groups it has issued so far."""
        t, g = C.c_int(), C.c_long()
        self._ck(lib.sf_transport_info(self._h, C.byref(t), C.byref(g)))
        return {"transport": TRANSPORTS[t.value], "rccl_groups": g.value}

    def layout_info(self):
        pitch, planes, nbytes = C.c_int(), C.c_int(), C.c_size_t()
        self._ck(lib.sf_layout_info(self._h, C.byref(pitch), C.byref(planes), C.byref(nbytes)))
        return {"row_pitch": pitch.value, "planes_per_slab": planes.value, "bytes_per_field": nbytes.value}
