// sf_api.hip — the C ABI of include/sfgpu.h over the type-erased solver (sf_base.hpp). No exception crosses it: every
// entry point returns a status code and leaves the message in sf_last_error (the reference's convention is print +
// exit(1), FluidGPU.cuh:34-41; the driver does that with the code it gets back).
#include <cmath>
#include "sf_base.hpp"

using namespace sfi;

namespace {
thread_local std::string g_create_error;
}


struct sf_ctx {
    std::unique_ptr<SolverBase> impl;
    std::string err;
    std::string snap_err;  // sf_snapshot_read may run on another thread: it gets its own message buffer
};

namespace {

template <class F>
int guarded(sf_ctx* ctx, F&& body) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    try {
        body(*ctx->impl);
        return SF_OK;
    } catch (const Failure& f) {
        ctx->err = f.msg;
        return f.code;
    } catch (const std::exception& e) {
        ctx->err = e.what();
        return SF_ERR_INVALID;
    }
}

}  // namespace

extern "C" {

const char* sf_version(void) { return "sfgpu 0.1 gfx950 hip"; }

const char* sf_status_string(int status) {
    switch (status) {
        case SF_OK: return "SF_OK";
        case SF_ERR_INVALID: return "SF_ERR_INVALID";
        case SF_ERR_HIP: return "SF_ERR_HIP";
        case SF_ERR_RCCL: return "SF_ERR_RCCL";
        case SF_ERR_HALO_EXCEEDED: return "SF_ERR_HALO_EXCEEDED";
        case SF_ERR_NO_DEVICE: return "SF_ERR_NO_DEVICE";
        case SF_ERR_TRACER_OVERFLOW: return "SF_ERR_TRACER_OVERFLOW";
        default: return "SF_ERR_UNKNOWN";
    }
}

int sf_nccl_unique_id(void* out) {
    if (!out) return SF_ERR_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return SF_ERR_RCCL;
    std::memset(out, 0, SF_NCCL_ID_BYTES);
    std::memcpy(out, &id, sizeof id);
    return SF_OK;
}

int sf_create(sf_ctx** out, const sf_params* p) {
    if (!out) return SF_ERR_INVALID;
    *out = nullptr;
    if (!p) {
        g_create_error = "null params";
        return SF_ERR_INVALID;
    }
    try {
        std::unique_ptr<sf_ctx> ctx(new sf_ctx);
        if (p->dtype == SF_F32)
            ctx->impl.reset(make_solver_f32(*p));
        else if (p->dtype == SF_F64)
            ctx->impl.reset(make_solver_f64(*p));
        else
            throw Failure{SF_ERR_INVALID, "dtype must be SF_F32 or SF_F64"};
        *out = ctx.release();
        return SF_OK;
    } catch (const Failure& f) {
        g_create_error = f.msg;
        return f.code;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return SF_ERR_INVALID;
    }
}

void sf_destroy(sf_ctx* ctx) { delete ctx; }

int sf_upload(sf_ctx* ctx, int field, const void* host) {
    return guarded(ctx, [&](SolverBase& s) { s.upload(field, host); });
}
int sf_download(sf_ctx* ctx, int field, void* host) {
    return guarded(ctx, [&](SolverBase& s) { s.download(field, host); });
}
int sf_download_planes(sf_ctx* ctx, int field, int k_begin, int k_end, void* host) {
    return guarded(ctx, [&](SolverBase& s) { s.download_planes(field, k_begin, k_end, host); });
}
int sf_upload_planes(sf_ctx* ctx, int field, int k_begin, int k_end, const void* host) {
    return guarded(ctx, [&](SolverBase& s) { s.upload_planes(field, k_begin, k_end, host); });
}
int sf_stored_planes(const sf_ctx* ctx, int* k_begin, int* k_end) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    ctx->impl->stored_planes(k_begin, k_end);
    return SF_OK;
}
int sf_owned_planes(const sf_ctx* ctx, int* k_begin, int* k_end) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    ctx->impl->owned_planes(k_begin, k_end);
    return SF_OK;
}
int sf_fill(sf_ctx* ctx, int field, double value) {
    return guarded(ctx, [&](SolverBase& s) { s.fill(field, value); });
}
int sf_copy_field(sf_ctx* ctx, int dst, int src) {
    return guarded(ctx, [&](SolverBase& s) { s.copy_field(dst, src); });
}
int sf_bind_sources(sf_ctx* ctx, int su, int sv, int sw, int sd) {
    return guarded(ctx, [&](SolverBase& s) { s.bind_sources(su, sv, sw, sd); });
}
int vel_step(sf_ctx* ctx) {
    return guarded(ctx, [&](SolverBase& s) { s.vel_step(); });
}
int dens_step(sf_ctx* ctx) {
    return guarded(ctx, [&](SolverBase& s) { s.dens_step(); });
}
int sf_add_source(sf_ctx* ctx, int x, int src) {
    return guarded(ctx, [&](SolverBase& s) { s.add_source(x, src); });
}
int sf_set_bnd(sf_ctx* ctx, int b, int x) {
    return guarded(ctx, [&](SolverBase& s) { s.set_bnd(b, x); });
}
int sf_lin_solve(sf_ctx* ctx, int b, int x, int x0, double a, double c, int iters) {
    return guarded(ctx, [&](SolverBase& s) { s.lin_solve(b, x, x0, a, c, iters); });
}
int sf_diffuse(sf_ctx* ctx, int b, int x, int x0, double diff) {
    return guarded(ctx, [&](SolverBase& s) { s.diffuse(b, x, x0, diff); });
}
int sf_advect(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w) {
    return guarded(ctx, [&](SolverBase& s) { s.advect(b, d, d0, u, v, w); });
}
int sf_advect_maccormack(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w) {
    return guarded(ctx, [&](SolverBase& s) { s.advect_maccormack(b, d, d0, u, v, w); });
}
int sf_set_advection(sf_ctx* ctx, int velocity_scheme, int density_scheme) {
    return guarded(ctx, [&](SolverBase& s) { s.set_advection(velocity_scheme, density_scheme); });
}
int sf_project(sf_ctx* ctx, int u, int v, int w, int p, int div) {
    return guarded(ctx, [&](SolverBase& s) { s.project(u, v, w, p, div); });
}
int sf_vorticity_magnitude(sf_ctx* ctx, int u, int v, int w, int dst) {
    return guarded(ctx, [&](SolverBase& s) { s.vorticity_magnitude(u, v, w, dst); });
}
int sf_add_forces(sf_ctx* ctx, int u, int v, int w, int dens, int su, int sv, int sw) {
    return guarded(ctx, [&](SolverBase& s) { s.add_forces(u, v, w, dens, su, sv, sw); });
}
int sf_set_vorticity_confinement(sf_ctx* ctx, double eps) {
    return guarded(ctx, [&](SolverBase& s) { s.set_vorticity_confinement(eps); });
}
int sf_set_buoyancy(sf_ctx* ctx, double beta, double ambient, int axis) {
    return guarded(ctx, [&](SolverBase& s) { s.set_buoyancy(beta, ambient, axis); });
}
int sf_snapshot(sf_ctx* ctx, const int* fields, int nfields) {
    return guarded(ctx, [&](SolverBase& s) { s.snapshot(fields, nfields); });
}
int sf_snapshot_read(sf_ctx* ctx, int index, void* host) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    try {
        ctx->impl->snapshot_read(index, host);
        return SF_OK;
    } catch (const Failure& f) {
        ctx->snap_err = f.msg;
        return f.code;
    } catch (const std::exception& e) {  // e.g. std::bad_alloc: nothing may cross the C ABI
        ctx->snap_err = e.what();
        return SF_ERR_INVALID;
    }
}
int sf_snapshot_read_planes(sf_ctx* ctx, int index, int k_begin, int k_end, void* host) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    try {
        ctx->impl->snapshot_read_planes(index, k_begin, k_end, host);
        return SF_OK;
    } catch (const Failure& f) {
        ctx->snap_err = f.msg;
        return f.code;
    } catch (const std::exception& e) {
        ctx->snap_err = e.what();
        return SF_ERR_INVALID;
    }
}
int sf_tracers_set(sf_ctx* ctx, int n, const void* xyz) {
    return guarded(ctx, [&](SolverBase& s) { s.tracers_set(n, xyz); });
}
int sf_tracers_advect(sf_ctx* ctx) {
    return guarded(ctx, [&](SolverBase& s) { s.tracers_advect(); });
}
int sf_tracers_get(sf_ctx* ctx, void* xyz, void* dens_sample, void* speed_sample) {
    return guarded(ctx, [&](SolverBase& s) { s.tracers_get(xyz, dens_sample, speed_sample); });
}
int sf_tracers_owned(const sf_ctx* ctx, int* n_owned) {
    return guarded(const_cast<sf_ctx*>(ctx), [&](SolverBase& s) {
        const int n = s.tracers_owned();
        if (n_owned) *n_owned = n;
    });
}
int sf_tracers_get_owned(sf_ctx* ctx, int* ids, void* xyz, void* dens_sample, void* speed_sample) {
    return guarded(ctx, [&](SolverBase& s) { s.tracers_get_owned(ids, xyz, dens_sample, speed_sample); });
}
int sf_tracers_set_capacity(sf_ctx* ctx, int per_direction) {
    return guarded(ctx, [&](SolverBase& s) { s.tracers_set_capacity(per_direction); });
}
int sf_reduce(sf_ctx* ctx, int op, int field, double* out) {
    return guarded(ctx, [&](SolverBase& s) { s.reduce(op, field, out); });
}
int sf_diagnostics_get(sf_ctx* ctx, sf_diagnostics* out) {
    return guarded(ctx, [&](SolverBase& s) { s.diagnostics(out); });
}
int sf_set_pressure_solver(sf_ctx* ctx, int solver, double tol, int max_iters) {
    return guarded(ctx, [&](SolverBase& s) { s.set_pressure_solver(solver, tol, max_iters); });
}
int sf_project_cg(sf_ctx* ctx, int u, int v, int w, int p, int div, double tol, int max_iters) {
    return guarded(ctx, [&](SolverBase& s) { s.project_cg(u, v, w, p, div, tol, max_iters); });
}
int sf_poisson_residual(sf_ctx* ctx, int p, int div, double* rel) {
    return guarded(ctx, [&](SolverBase& s) { s.poisson_residual(p, div, rel); });
}
int sf_pressure_info_get(const sf_ctx* ctx, sf_pressure_info* out) {
    if (!ctx || !ctx->impl || !out) return SF_ERR_INVALID;
    ctx->impl->pressure_info(out);
    return SF_OK;
}
int sf_set_pressure_sync(sf_ctx* ctx, int check_every) {
    return guarded(ctx, [&](SolverBase& s) { s.set_pressure_sync(check_every); });
}
int sf_pressure_sync_get(const sf_ctx* ctx, sf_pressure_sync* out) {
    if (!ctx || !ctx->impl || !out) return SF_ERR_INVALID;
    ctx->impl->pressure_sync(out);
    return SF_OK;
}
int sf_set_pressure_preconditioner(sf_ctx* ctx, int kind, int sweeps) {
    return guarded(ctx, [&](SolverBase& s) { s.set_pressure_preconditioner(kind, sweeps); });
}
int sf_pressure_preconditioner_get(const sf_ctx* ctx, sf_pressure_preconditioner* out) {
    if (!ctx || !ctx->impl || !out) return SF_ERR_INVALID;
    ctx->impl->pressure_preconditioner(out);
    return SF_OK;
}
int sf_set_pressure_multigrid(sf_ctx* ctx, int sweeps, int max_levels, int coarse_sweeps) {
    return guarded(ctx, [&](SolverBase& s) { s.set_pressure_multigrid(sweeps, max_levels, coarse_sweeps); });
}
int sf_pressure_multigrid_get(const sf_ctx* ctx, sf_pressure_multigrid* out) {
    if (!ctx || !ctx->impl || !out) return SF_ERR_INVALID;
    ctx->impl->pressure_multigrid(out);
    return SF_OK;
}
int sf_precondition(sf_ctx* ctx, int z, int r) {
    return guarded(ctx, [&](SolverBase& s) { s.precondition(z, r); });
}
int sf_set_obstacles(sf_ctx* ctx, int mask_slot) {
    return guarded(ctx, [&](SolverBase& s) { s.set_obstacles(mask_slot); });
}
int sf_obstacles_get(const sf_ctx* ctx, sf_obstacles* out) {
    if (!ctx || !ctx->impl || !out) return SF_ERR_INVALID;
    ctx->impl->obstacles(out);
    return SF_OK;
}
int sf_set_obstacle_multigrid(sf_ctx* ctx, int on) {
    return guarded(ctx, [&](SolverBase& s) { s.set_obstacle_multigrid(on); });
}
int sf_obstacle_multigrid_get(const sf_ctx* ctx, int* on) {
    if (!ctx || !ctx->impl || !on) return SF_ERR_INVALID;
    ctx->impl->obstacle_multigrid(on);
    return SF_OK;
}
int sf_precondition_masked(sf_ctx* ctx, int z, int r) {
    return guarded(ctx, [&](SolverBase& s) { s.precondition_masked(z, r); });
}
int sf_set_obstacle_transport(sf_ctx* ctx, int on) {
    return guarded(ctx, [&](SolverBase& s) { s.set_obstacle_transport(on); });
}
int sf_obstacle_transport_get(const sf_ctx* ctx, int* on) {
    if (!ctx || !ctx->impl || !on) return SF_ERR_INVALID;
    ctx->impl->obstacle_transport(on);
    return SF_OK;
}
int sf_diffuse_masked(sf_ctx* ctx, int b, int x, int x0, double diff) {
    return guarded(ctx, [&](SolverBase& s) { s.diffuse_masked(b, x, x0, diff); });
}
int sf_advect_masked(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w) {
    return guarded(ctx, [&](SolverBase& s) { s.advect_masked(b, d, d0, u, v, w); });
}
int sf_set_obstacle_maccormack(sf_ctx* ctx, int on) {
    return guarded(ctx, [&](SolverBase& s) { s.set_obstacle_maccormack(on); });
}
int sf_obstacle_maccormack_get(const sf_ctx* ctx, int* on) {
    if (!ctx || !ctx->impl || !on) return SF_ERR_INVALID;
    ctx->impl->obstacle_maccormack(on);
    return SF_OK;
}
int sf_set_obstacle_velocity(sf_ctx* ctx, int su, int sv, int sw) {
    return guarded(ctx, [&](SolverBase& s) { s.set_obstacle_velocity(su, sv, sw); });
}
int sf_obstacle_velocity_get(const sf_ctx* ctx, int* on) {
    if (!ctx || !ctx->impl || !on) return SF_ERR_INVALID;
    ctx->impl->obstacle_velocity(on);
    return SF_OK;
}
int sf_advect_maccormack_masked(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w) {
    return guarded(ctx, [&](SolverBase& s) { s.advect_maccormack_masked(b, d, d0, u, v, w); });
}
int sf_render(sf_ctx* ctx, const sf_render_params* p) {
    return guarded(ctx, [&](SolverBase& s) { s.render(p); });
}
int sf_render_read(sf_ctx* ctx, void* colour, void* transmittance) {
    return guarded(ctx, [&](SolverBase& s) { s.render_read(colour, transmittance); });
}
int sf_light(sf_ctx* ctx, int dst, int dens, int axis, int from_high, double sigma) {
    return guarded(ctx, [&](SolverBase& s) { s.light(dst, dens, axis, from_high, sigma); });
}
int sf_render_view(sf_ctx* ctx, const sf_view_params* p) {
    return guarded(ctx, [&](SolverBase& s) { s.render_view(p); });
}
int sf_render_view_read(sf_ctx* ctx, void* colour, void* transmittance) {
    return guarded(ctx, [&](SolverBase& s) { s.render_view_read(colour, transmittance); });
}
// docs/SPEC.md §13: double arithmetic, + - * / sqrt only, bracketed as written (this file is compiled without contraction)
int sf_view_frame(int N, const double dir[3], const double up[3], int width, int height, double step, double sigma,
                  sf_view_params* out) {
    if (!dir || !up || !out || N < 1) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(dir[c]) || !std::isfinite(up[c])) return SF_ERR_INVALID;
    if (!std::isfinite(step) || !(step > 0.0) || !std::isfinite(sigma) || sigma < 0.0) return SF_ERR_INVALID;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return SF_ERR_INVALID;
    auto len = [](const double* v) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); };
    auto cross = [](const double* a, const double* b, double* o) {
        o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double d[3], r[3], u[3];
    const double ld = len(dir);
    if (!(ld > 0.0) || !std::isfinite(ld)) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c) d[c] = dir[c] / ld;
    cross(d, up, r);
    const double lr = len(r);
    if (!(lr > 0.0) || !std::isfinite(lr)) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c) r[c] = r[c] / lr;
    cross(r, d, u);
    const double L = std::sqrt(3.0) * N, pix = L / (width > height ? width : height), cen = (N + 1) / 2.0;
    if (!(L / step < 65536.0)) return SF_ERR_INVALID;  // samples would leave 1 .. 65536
    sf_view_params f{};
    for (int c = 0; c < 3; ++c) {
        f.du[c] = r[c] * pix;
        f.dv[c] = u[c] * pix;
        f.step[c] = d[c] * step;
        f.origin[c] = ((cen - d[c] * (L / 2)) - f.du[c] * ((width - 1) / 2.0)) - f.dv[c] * ((height - 1) / 2.0);
    }
    f.width = width, f.height = height;
    f.samples = (int)(L / step) + 1;
    f.sigma = sigma * step;
    f.dens = f.emit = -1;
    for (const double* v : {f.origin, f.du, f.dv, f.step})
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(v[c])) return SF_ERR_INVALID;
    if (!std::isfinite(f.sigma)) return SF_ERR_INVALID;
    *out = f;
    return SF_OK;
}
int sf_render_camera(sf_ctx* ctx, const sf_camera_params* p) {
    return guarded(ctx, [&](SolverBase& s) { s.render_camera(p); });
}
int sf_camera_passes_get(const sf_camera_params* p, int dtype, int* passes) {
    if (!p || !passes || (dtype != SF_F32 && dtype != SF_F64)) return SF_ERR_INVALID;
    if (p->view.width < 1 || p->view.width > 16384 || p->view.height < 1 || p->view.height > 16384) return SF_ERR_INVALID;
    for (const double* v : {p->view.origin, p->view.du, p->view.dv, p->view.step, p->step_du, p->step_dv})
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(v[c])) return SF_ERR_INVALID;
    int out = 0;
    const bool ok = dtype == SF_F32 ? camera_corner_rule<float>(*p, &out) : camera_corner_rule<double>(*p, &out);
    if (!ok) return SF_ERR_INVALID;
    *passes = out;
    return SF_OK;
}
// docs/SPEC.md §14: double arithmetic, + - * / sqrt only, bracketed as written
int sf_camera_frame(int N, const double eye[3], const double target[3], const double up[3], double tan_half_fov,
                    int width, int height, double step, double sigma, sf_camera_params* out) {
    if (!eye || !target || !up || !out || N < 1) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(eye[c]) || !std::isfinite(target[c]) || !std::isfinite(up[c])) return SF_ERR_INVALID;
    if (!std::isfinite(step) || !(step > 0.0) || !std::isfinite(sigma) || sigma < 0.0) return SF_ERR_INVALID;
    if (!std::isfinite(tan_half_fov) || !(tan_half_fov > 0.0)) return SF_ERR_INVALID;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return SF_ERR_INVALID;
    auto len = [](const double* v) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); };
    auto cross = [](const double* a, const double* b, double* o) {
        o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double f[3], d[3], r[3], u[3], e[3], q0[3];
    for (int c = 0; c < 3; ++c) f[c] = target[c] - eye[c];
    const double lf = len(f);
    if (!(lf > 0.0) || !std::isfinite(lf)) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c) d[c] = f[c] / lf;
    cross(d, up, r);
    const double lr = len(r);
    if (!(lr > 0.0) || !std::isfinite(lr)) return SF_ERR_INVALID;
    for (int c = 0; c < 3; ++c) r[c] = r[c] / lr;
    cross(r, d, u);
    const double R = std::sqrt(3.0) * N / 2.0, cen = (N + 1) / 2.0;
    for (int c = 0; c < 3; ++c) e[c] = cen - eye[c];
    const double dc = (e[0] * d[0] + e[1] * d[1]) + e[2] * d[2];
    double t0 = dc - R;
    if (!(t0 > 0.0)) t0 = 0.0;
    const double t1 = dc + R;
    if (!(t1 > t0)) return SF_ERR_INVALID;  // the box lies behind the camera
    if (!((t1 - t0) / step < 65536.0)) return SF_ERR_INVALID;  // samples would leave 1 .. 65536
    const double pp = (2.0 * tan_half_fov) / height;
    sf_camera_params k{};
    for (int c = 0; c < 3; ++c) {
        q0[c] = (d[c] - r[c] * (pp * ((width - 1) / 2.0))) - u[c] * (pp * ((height - 1) / 2.0));
        k.view.origin[c] = eye[c] + q0[c] * t0;
        k.view.du[c] = r[c] * (pp * t0);
        k.view.dv[c] = u[c] * (pp * t0);
        k.view.step[c] = q0[c] * step;
        k.step_du[c] = r[c] * (pp * step);
        k.step_dv[c] = u[c] * (pp * step);
    }
    k.view.width = width, k.view.height = height;
    k.view.samples = (int)((t1 - t0) / step) + 1;
    k.view.sigma = sigma;
    k.view.dens = k.view.emit = -1;
    for (const double* v : {k.view.origin, k.view.du, k.view.dv, k.view.step, k.step_du, k.step_dv})
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(v[c])) return SF_ERR_INVALID;
    *out = k;
    return SF_OK;
}
int sf_set_iters(sf_ctx* ctx, int iters) {
    return guarded(ctx, [&](SolverBase& s) { s.set_iters(iters); });
}
int sf_set_coefficients(sf_ctx* ctx, double dt, double diff, double visc) {
    return guarded(ctx, [&](SolverBase& s) { s.set_coefficients(dt, diff, visc); });
}
int sf_sync(sf_ctx* ctx) {
    return guarded(ctx, [&](SolverBase& s) { s.sync(); });
}
const char* sf_last_error(const sf_ctx* ctx) {
    if (!ctx) return g_create_error.c_str();
    return ctx->err.c_str();
}
int sf_timer_start(sf_ctx* ctx) {
    return guarded(ctx, [&](SolverBase& s) { s.timer_start(); });
}
int sf_timer_stop(sf_ctx* ctx, float* ms) {
    return guarded(ctx, [&](SolverBase& s) {
        const float t = s.timer_stop();
        if (ms) *ms = t;
    });
}
int sf_measure_copy_bandwidth(sf_ctx* ctx, size_t bytes, int reps, double* gbps) {
    return guarded(ctx, [&](SolverBase& s) {
        const double r = s.copy_bandwidth(bytes, reps);
        if (gbps) *gbps = r;
    });
}
int sf_lin_solve_launches(const sf_ctx* ctx, int iters) {
    if (!ctx || !ctx->impl || iters < 0) return -1;
    return ctx->impl->lin_solve_launches(iters);
}
int sf_layout_info(const sf_ctx* ctx, int* row_pitch, int* planes_per_slab, size_t* bytes_per_field) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    ctx->impl->layout_info(row_pitch, planes_per_slab, bytes_per_field);
    return SF_OK;
}
int sf_schedule_info(const sf_ctx* ctx, int* trapezoid_pairs, int* measured) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    ctx->impl->schedule_info(trapezoid_pairs, measured);
    return SF_OK;
}
int sf_transport_info(const sf_ctx* ctx, int* transport, long* rccl_groups) {
    if (!ctx || !ctx->impl) return SF_ERR_INVALID;
    ctx->impl->transport_info(transport, rccl_groups);
    return SF_OK;
}

}  // extern "C"
