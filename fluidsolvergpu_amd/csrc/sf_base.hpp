// sf_base.hpp — what the translation units of libsfgpu.so share: the error type and macros (those that need only the
// HIP runtime API come from sf_hip.hpp; SF_NCCL and whatever else needs rccl.h is here), the type-erased solver
// interface behind the C ABI (include/sfgpu.h) and the per-precision factories (sf_solver_f32.hip / sf_solver_f64.hip
// instantiate sfi::Solver<float> / <double> separately, so the two halves of the library compile in parallel).
#pragma once
#include "sf_hip.hpp"
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace sfi {

#define SF_NCCL(expr)                                                                              \
    do {                                                                                           \
        ncclResult_t _r = (expr);                                                                  \
        if (_r != ncclSuccess)                                                                     \
            throw Failure{SF_ERR_RCCL, std::string("RCCL error ") + ncclGetErrorString(_r) +       \
                                           " at line " + std::to_string(__LINE__) + " (" #expr ")"}; \
    } while (0)

inline int env_int(const char* name, int dflt) {
    const char* s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// The corner rule of docs/SPEC.md §14 in T (host arithmetic, compiled without contraction: the device's r_z in bits).
// r_z = (step_z + T(a) step_du_z) + T(b) step_dv_z is monotone in a and in b, so its extremes over the image lie at the
// four corner pixels: all >= 0 is one upward chain, all < 0 one downward chain, else both. False where a corner's step
// vector or origin is not finite in T (then *passes is not written).
template <class T>
inline bool camera_corner_rule(const sf_camera_params& p, int* passes) {
    int ups = 0;
    for (int corner = 0; corner < 4; ++corner) {
        const T a = (T)((corner & 1) ? p.view.width - 1 : 0), b = (T)((corner & 2) ? p.view.height - 1 : 0);
        T rz = T(0);
        for (int c = 0; c < 3; ++c) {
            const T r = ((T)p.view.step[c] + a * (T)p.step_du[c]) + b * (T)p.step_dv[c];
            const T o = ((T)p.view.origin[c] + a * (T)p.view.du[c]) + b * (T)p.view.dv[c];
            if (!std::isfinite(r) || !std::isfinite(o)) return false;
            rz = r;
        }
        ups += rz < T(0) ? 0 : 1;
    }
    *passes = ups == 4 ? SF_CAMERA_UP : ups == 0 ? SF_CAMERA_DOWN : SF_CAMERA_BOTH;
    return true;
}

class SolverBase {
public:
    virtual ~SolverBase() {}
    virtual void upload(int field, const void* host) = 0;
    virtual void download(int field, void* host) = 0;
    virtual void download_planes(int field, int kb, int ke, void* host) = 0;
    virtual void upload_planes(int field, int kb, int ke, const void* host) = 0;
    virtual void owned_planes(int* kb, int* ke) const = 0;
    virtual void stored_planes(int* kb, int* ke) const = 0;
    virtual void fill(int field, double value) = 0;
    virtual void copy_field(int dst, int src) = 0;
    virtual void bind_sources(int su, int sv, int sw, int sd) = 0;
    virtual void vel_step() = 0;
    virtual void dens_step() = 0;
    virtual void add_source(int x, int s) = 0;
    virtual void set_bnd(int b, int x) = 0;
    virtual void lin_solve(int b, int x, int x0, double a, double c, int iters) = 0;
    virtual void diffuse(int b, int x, int x0, double diff) = 0;
    virtual void advect(int b, int d, int d0, int u, int v, int w) = 0;
    virtual void advect_maccormack(int b, int d, int d0, int u, int v, int w) = 0;
    virtual void set_advection(int velocity_scheme, int density_scheme) = 0;
    virtual void project(int u, int v, int w, int p, int div) = 0;
    virtual void vorticity_magnitude(int u, int v, int w, int dst) = 0;
    virtual void add_forces(int u, int v, int w, int dens, int su, int sv, int sw) = 0;
    virtual void set_vorticity_confinement(double eps) = 0;
    virtual void set_buoyancy(double beta, double ambient, int axis) = 0;
    virtual void set_iters(int iters) = 0;
    virtual void set_coefficients(double dt, double diff, double visc) = 0;
    virtual void sync() = 0;
    virtual void timer_start() = 0;
    virtual float timer_stop() = 0;
    virtual double copy_bandwidth(size_t bytes, int reps) = 0;
    virtual void layout_info(int* pitch, int* planes, size_t* bytes) const = 0;
    virtual void schedule_info(int* trap, int* measured) const = 0;
    virtual void transport_info(int* transport, long* groups) const = 0;
    virtual int lin_solve_launches(int iters) const = 0;
    virtual void snapshot(const int* fields, int nfields) = 0;
    virtual void snapshot_read(int index, void* host) = 0;
    virtual void snapshot_read_planes(int index, int kb, int ke, void* host) = 0;
    virtual void tracers_set(int n, const void* xyz) = 0;
    virtual void tracers_advect() = 0;
    virtual void tracers_get(void* xyz, void* dens, void* speed) = 0;
    virtual void tracers_set_capacity(int per_direction) = 0;
    virtual int tracers_owned() = 0;
    virtual void tracers_get_owned(int* ids, void* xyz, void* dens, void* speed) = 0;
    virtual void reduce(int op, int field, double* out) = 0;
    virtual void diagnostics(sf_diagnostics* out) = 0;
    virtual void set_pressure_solver(int solver, double tol, int max_iters) = 0;
    virtual void project_cg(int u, int v, int w, int p, int div, double tol, int max_iters) = 0;
    virtual void poisson_residual(int p, int div, double* rel) = 0;
    virtual void pressure_info(sf_pressure_info* out) const = 0;
    virtual void set_pressure_sync(int check_every) = 0;
    virtual void pressure_sync(sf_pressure_sync* out) const = 0;
    virtual void set_pressure_preconditioner(int kind, int sweeps) = 0;
    virtual void pressure_preconditioner(sf_pressure_preconditioner* out) const = 0;
    virtual void set_pressure_multigrid(int sweeps, int max_levels, int coarse_sweeps) = 0;
    virtual void pressure_multigrid(sf_pressure_multigrid* out) const = 0;
    virtual void precondition(int z, int r) = 0;
    virtual void set_obstacles(int mask_slot) = 0;
    virtual void obstacles(sf_obstacles* out) const = 0;
    virtual void set_obstacle_multigrid(int on) = 0;
    virtual void obstacle_multigrid(int* on) const = 0;
    virtual void precondition_masked(int z, int r) = 0;
    virtual void set_obstacle_transport(int on) = 0;
    virtual void obstacle_transport(int* on) const = 0;
    virtual void diffuse_masked(int b, int x, int x0, double diff) = 0;
    virtual void advect_masked(int b, int d, int d0, int u, int v, int w) = 0;
    virtual void set_obstacle_maccormack(int on) = 0;
    virtual void obstacle_maccormack(int* on) const = 0;
    virtual void set_obstacle_velocity(int su, int sv, int sw) = 0;
    virtual void obstacle_velocity(int* on) const = 0;
    virtual void advect_maccormack_masked(int b, int d, int d0, int u, int v, int w) = 0;
    virtual void render(const sf_render_params* p) = 0;
    virtual void render_read(void* colour, void* transmittance) = 0;
    virtual void light(int dst, int dens, int axis, int from_high, double sigma) = 0;
    virtual void render_view(const sf_view_params* p) = 0;
    virtual void render_view_read(void* colour, void* transmittance) = 0;
    virtual void render_camera(const sf_camera_params* p) = 0;
};

SolverBase* make_solver_f32(const sf_params& p);
SolverBase* make_solver_f64(const sf_params& p);

}  // namespace sfi
