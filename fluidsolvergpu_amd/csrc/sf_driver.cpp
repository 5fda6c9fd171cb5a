// sf_driver.cpp — C++ host driver over the C ABI (include/sfgpu.h) and the VTK frame writer.
//
// Keeps the SHAPE of the reference's host loop (solver.cu:171-216, solver-unidyn.cu:313-573):
// per step print "t= <t>", bracket the device work with an event pair, print
// "done.\nElapsed kernel time: <ms> ms", and every <every> steps copy the fields back and write
// "anim_s<frame>.vtk" (naming of solver.cu:210 / solver-unidyn.cu:484). Errors follow the
// reference's CUDA_CHECK_RETURN convention (FluidGPU.cuh:34-41): print and exit(1).
// Unlike the reference (compile-time #defines, argv ignored — solver.cu:17-19,64) everything is a
// run-time option, and the grid solver behind vel_step/dens_step is the stable-fluids path of
// docs/SPEC.md, not the reference's SPH kernels.
//
// Output is asynchronous: at an output step the fields are snapshotted on the device and a
// writer thread downloads and encodes the frame while the main loop keeps stepping; the reference blocks on
// cudaDeviceSynchronize + cudaMemcpy + per-value sprintf instead (solver-unidyn.cu:475-487). With --tracers N a
// cloud of passive tracers is advected through the velocity field and written with write_point_mesh, the one
// writer call the reference really makes (solver-unidyn.cu:487: ASCII, two point scalars), on any decomposition: one
// file with every tracer in one process, one file per rank (its own tracers, tracers_s_GPU<rank>_<frame>.vtk) on several.
//
// Several GPUs: start one process per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT in the environment
// (e.g. `python -m torch.distributed.run --no-python --nproc-per-node 8 ./sf_driver ...`). Rank 0 creates the
// ncclUniqueId and hands it to the others through a file under /tmp keyed by MASTER_PORT (single node); every
// rank then owns one k-slab and writes its own frames as anim_s_GPU<rank>_<frame>.vtk — the per-device naming
// of solver-unidyn.cu:484-490 — as a rectilinear mesh carrying its z range.
//
//   sf_driver [--n 64] [--steps 20] [--iters 20] [--dtype f32|f64] [--every 10] [--out DIR]
//             [--binary] [--device 0] [--slabs 1] [--plumbing] [--quiet] [--sync-output] [--tracers 0]
//             [--vorticity EPS] [--buoyancy BETA] [--ambient A] [--buoyancy-axis 1] [--maccormack vel|dens|both]
//             [--monitor M] [--pressure jacobi|cg[:tol[:max_iters]]] [--pressure-sync M]
//             [--pressure-precond none|jacobi:M] [--pressure-mg NU[:LEVELS[:COARSE]]] [--render VIEW:SIGMA[:LIGHT]]
//             [--render-view DX,DY,DZ:WxH:SIGMA[:STEP]] [--render-camera EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]]]
//             [--obstacle box:I0,J0,K0:I1,J1,K1 | sphere:CX,CY,CZ:R]... [--obstacle-mg]
//             [--obstacle-transport] [--obstacle-maccormack] [--obstacle-velocity VX,VY,VZ] [--help]
// --vorticity / --buoyancy switch on the smoke forces of docs/SPEC.md §8 (vorticity confinement, buoyancy
// BETA*(dens - A) on velocity component --buoyancy-axis: 0 u, 1 v (the direction of the v0 source), 2 w).
// --maccormack advects the velocity, the density or both with the limited MacCormack scheme of docs/SPEC.md §9
// (default: first-order semi-Lagrangian for both, the §3 step).
// --monitor M: after every M-th step (t = 0, M, 2M, ... as --every counts) rank 0 prints one line
//   monitor step=<t> mass=<g> kinetic=<g> max_div=<g> cfl=<g> nonfinite=<n>
// from sf_diagnostics_get (docs/SPEC.md §10; %.17g, so the doubles read back exactly; every rank holds the same
// numbers). A state with nonfinite > 0 ends the run: an error naming the step, exit status 3. Without --monitor the
// driver issues exactly the calls it issued before the option existed.
// --pressure selects what vel_step's two projections run (docs/SPEC.md §11): jacobi (the default, --iters sweeps) or
// cg with a relative tolerance (default 1e-3) and an iteration limit (default 100). With --monitor a second line
//   pressure step=<t> solver=<jacobi|cg> status=<s> iterations=<n> rel_residual=<g> iterations_total=<n>
// follows each monitor line: the step's last projection (sf_pressure_info_get).
// --pressure-sync M (with --pressure cg): check_every of sf_set_pressure_sync. 0, the default: the host reads every inner
// product of a solve; M >= 1: the solve's scalars stay on the device and the host looks at them every M iterations. The
// frames and the monitor lines are the same bits either way.
// --pressure-precond none|jacobi:M (with --pressure cg): the preconditioner of the CG solve (docs/SPEC.md §11.2), M >= 1
// undamped Jacobi sweeps from zero per iteration. none, the default: §11 as it stands.
// --pressure-mg NU[:LEVELS[:COARSE]] (with --pressure cg): the multigrid V-cycle preconditioner of docs/SPEC.md §11.3 with
// NU >= 1 sweeps per level, at most LEVELS levels (0, the default: as many as the grid allows) and COARSE >= 1 sweeps on
// the coarsest (default 8). In force it takes the place of --pressure-precond.
// --obstacle box:I0,J0,K0:I1,J1,K1 | sphere:CX,CY,CZ:R (with --pressure cg, not with --pressure-mg; up to 16 times): solid
// cells of docs/SPEC.md §15, in cell indices: the cells of the inclusive index box, or those whose centre index lies
// within R of (CX, CY, CZ) — squared distance, in double, <= R^2. The union of all of them is the mask of sf_set_obstacles.
// --obstacle-mg: lets --obstacle go with --pressure-mg: the masked V-cycle of docs/SPEC.md §16 (sf_set_obstacle_multigrid).
// --obstacle-transport: diffusion and advection honour the obstacles too (docs/SPEC.md §17, sf_set_obstacle_transport);
// needs --obstacle and does not go with --maccormack.
// --obstacle-maccormack: lets --obstacle-transport go with --maccormack: the masked MacCormack advection of
// docs/SPEC.md §18 (sf_set_obstacle_maccormack); needs --obstacle-transport.
// --obstacle-velocity VX,VY,VZ: every --obstacle moves with this velocity (docs/SPEC.md §19, sf_set_obstacle_velocity),
// in domain units per unit time, the unit of the velocity fields: advect traces a cell back by dt0 * u = dt * N * u
// cells, so a solid of velocity V is displaced by V * t * N cells at time t = step * dt, and the solid velocity the
// solver is given is the constant V itself. Before each step the mask is rasterised afresh (the offset of a box rounded
// to whole cells, the centre of a sphere kept in double, both clipped to the interior) and set again with the velocity.
// This happens before the step's timer starts: the reported step times leave out the rasterisation, the upload and the
// two setters (docs/NEXT.md, "Moving solids", has their cost). Needs --obstacle-transport; does not go with
// --maccormack vel|both.
// --render VIEW:SIGMA[:LIGHT]: at every output step an image of the density (docs/SPEC.md §12) next to the frame,
// "render_<frame, 4 digits>.pgm" (several processes: "render_GPU<rank>_<frame>.pgm", each rank the pixel rows it holds).
// VIEW and LIGHT are one of i+ i- j+ j- k+ k-: the axis of the rays and the side they enter from (+: at index 1). SIGMA
// >= 0 is the extinction per unit length. With LIGHT the smoke is lit from that side first: sf_light writes the
// transmittance towards the light into a slot that is free at an output step — an SF_USER slot that is not a bound
// source, else SF_DENS0, which is scratch between steps while a density source is bound — and the view takes it as its
// emission. The file is binary PGM (P5), maxval 65535, big-endian, q = (int)(min(max(C, 0), 1) * 65535 + 0.5) with
// NaN -> 0, the row with the highest b first.
// --render-view DX,DY,DZ:WxH:SIGMA[:STEP]: at every output step a W x H image of the density seen along the direction
// (DX, DY, DZ) in (i, j, k) (docs/SPEC.md §13, the frame of sf_view_frame), "view_<frame, 4 digits>.pgm" in the same PGM
// format, written by the process that holds the image (the last rank for DZ >= 0, else rank 0). up is (0,0,1), or (0,1,0)
// when the direction is parallel to k. SIGMA >= 0 is the extinction per unit length, STEP > 0 the sample distance in
// cells (default 1).
// --render-camera EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]]: at every output step a W x H pinhole image of the density
// from the eye E towards the target T, both in (i, j, k) with the centre of cell i at i (docs/SPEC.md §14, the frame of
// sf_camera_frame), "camera_<frame, 4 digits>.pgm" in the same PGM format, written by the process that holds the image
// (the last rank if every ray climbs, sf_camera_passes_get; else rank 0). up is (0,0,1), or (0,1,0) for a camera that looks
// along k. FOV_DEG is the vertical field of view (default 40), STEP > 0 the sample distance in depth (default 1).
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <ctime>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "../../include/sf_visit_writer.h"
#include "../../include/sfgpu.h"

static sf_ctx* g_ctx = nullptr;

#define SF_CHECK_RETURN(value)                                                                  \
    {                                                                                           \
        int _m_stat = (value);                                                                  \
        if (_m_stat != SF_OK) {                                                                 \
            fprintf(stderr, "Error %s (%s) at line %d in file %s\n", sf_status_string(_m_stat), \
                    sf_last_error(g_ctx), __LINE__, __FILE__);                                  \
            exit(1);                                                                            \
        }                                                                                       \
    }

struct Options {
    int n = 64, steps = 20, iters = 20, every = 10, device = 0, slabs = 1, tracers = 0, monitor = 0;
    double vorticity = 0.0, buoyancy = 0.0, ambient = 0.0;
    int buoyancy_axis = 1;
    int advect_vel = SF_ADVECT_SEMI_LAGRANGIAN, advect_dens = SF_ADVECT_SEMI_LAGRANGIAN;
    int pressure = SF_PRESSURE_JACOBI, cg_max_iters = 100, cg_check_every = 0;
    int cg_precond = SF_PRECOND_NONE, cg_precond_sweeps = 0;
    int mg_sweeps = 0, mg_levels = 0, mg_coarse = 8;
    struct Obstacle {
        bool sphere;
        double a[6];  // box: i0, j0, k0, i1, j1, k1; sphere: cx, cy, cz, r
    };
    std::vector<Obstacle> obstacles;  // --obstacle (docs/SPEC.md §15)
    bool obstacle_mg = false;         // --obstacle-mg (docs/SPEC.md §16)
    bool obstacle_transport = false;  // --obstacle-transport (docs/SPEC.md §17)
    bool obstacle_mc = false;         // --obstacle-maccormack (docs/SPEC.md §18)
    bool obstacle_moving = false;     // --obstacle-velocity (docs/SPEC.md §19)
    double obstacle_vel[3] = {0.0, 0.0, 0.0};
    double cg_tol = 1e-3;
    int render_axis = -1, render_high = 0, light_axis = -1, light_high = 0;  // --render (axis -1: off / no light)
    double render_sigma = 0.0;
    bool view = false;  // --render-view
    double view_dir[3] = {0, 0, 1}, view_sigma = 0.0, view_step = 1.0;
    int view_w = 0, view_h = 0;
    bool camera = false;  // --render-camera
    double cam_eye[3] = {0, 0, 0}, cam_target[3] = {0, 0, 1}, cam_sigma = 0.0, cam_fov = 40.0, cam_step = 1.0;
    int cam_w = 0, cam_h = 0;
    bool f64 = false, binary = false, plumbing = false, quiet = false, sync_output = false, loopback = false;
    std::string out = ".";
    int rank = 0, world = 1, local_rank = 0;
};

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// Single-node exchange of the 128-byte ncclUniqueId: rank 0 writes it (atomically, via rename), the others poll.
// The file name is unique per launch — it carries the pid of the launching agent (torch.distributed.run starts every
// local rank as its child) besides the rendezvous port — so a file left by an earlier run can never be taken for
// this run's; rank 0 removes a stale one before it publishes, and removes its own once sf_create has returned (the
// communicator exists then, so every rank has read the id). SF_NCCL_ID_FILE names the file explicitly for launchers
// whose ranks do not share a parent.
static std::string nccl_id_path() {
    if (const char* f = getenv("SF_NCCL_ID_FILE")) return f;
    char path[256];
    snprintf(path, sizeof path, "/tmp/sf_ncclid_%d_%ld_%s.bin", env_int("MASTER_PORT", 29500), (long)getppid(),
             getenv("TORCHELASTIC_RUN_ID") ? getenv("TORCHELASTIC_RUN_ID") : "run");
    return path;
}

// Start of this process (seconds since the epoch), from /proc: files older than it cannot belong to this launch.
static time_t process_start_time() {
    struct stat st;
    return stat("/proc/self", &st) == 0 ? st.st_ctime : time(nullptr);
}

static void share_nccl_id(const Options& o, unsigned char* id) {
    const std::string path = nccl_id_path();
    if (o.rank == 0) {
        unlink(path.c_str());  // whatever is there is not ours
        if (sf_nccl_unique_id(id) != SF_OK) {
            fprintf(stderr, "Error: sf_nccl_unique_id failed\n");
            exit(1);
        }
        const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(id, 1, SF_NCCL_ID_BYTES, f) != SF_NCCL_ID_BYTES || fclose(f) != 0 ||
            rename(tmp.c_str(), path.c_str()) != 0) {
            fprintf(stderr, "Error: cannot publish the nccl id at %s\n", path.c_str());
            exit(1);
        }
    } else {
        // With SF_NCCL_ID_FILE the name is NOT unique per launch: a file older than this process was left by an
        // earlier (crashed) run — rank 0 of this run has not published yet — and is not taken.
        const time_t born = process_start_time();
        for (int tries = 0; tries < 1200; ++tries) {  // up to 120 s
            struct stat st;
            if (stat(path.c_str(), &st) == 0 && st.st_mtime + 1 >= born) {
                FILE* f = fopen(path.c_str(), "rb");
                if (f) {
                    const size_t n = fread(id, 1, SF_NCCL_ID_BYTES, f);
                    fclose(f);
                    if (n == SF_NCCL_ID_BYTES) return;
                }
            }
            usleep(100000);
        }
        fprintf(stderr, "Error: rank %d timed out waiting for %s\n", o.rank, path.c_str());
        exit(1);
    }
}

static void usage(FILE* to) {
    fprintf(to,
            "usage: sf_driver [--n 64] [--steps 20] [--iters 20] [--dtype f32|f64] [--every 10] [--out DIR]\n"
            "                 [--binary] [--device 0] [--slabs 1] [--plumbing] [--quiet] [--sync-output] [--tracers 0]\n"
            "                 [--vorticity EPS] [--buoyancy BETA] [--ambient A] [--buoyancy-axis 1]\n"
            "                 [--maccormack vel|dens|both] [--monitor M] [--pressure jacobi|cg[:tol[:max_iters]]]\n"
            "                 [--pressure-sync M] [--pressure-precond none|jacobi:M] [--pressure-mg NU[:LEVELS[:COARSE]]]\n"
            "                 [--render VIEW:SIGMA[:LIGHT]]   VIEW, LIGHT: i+ i- j+ j- k+ k- (+ enters at the low index)\n"
            "                 [--render-view DX,DY,DZ:WxH:SIGMA[:STEP]]   an image along any direction, STEP in cells (default 1)\n"
            "                 [--render-camera EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]]]   a pinhole camera at E looking at T\n"
            "                 [--obstacle box:I0,J0,K0:I1,J1,K1 | sphere:CX,CY,CZ:R]...   solid cells (with --pressure cg), up to 16\n"
            "                 [--obstacle-mg]   --obstacle together with --pressure-mg: the masked V-cycle\n"
            "                 [--obstacle-transport]   diffusion and advection honour --obstacle too (not with --maccormack)\n"
            "                 [--obstacle-maccormack]   --obstacle-transport together with --maccormack: masked MacCormack\n"
            "                 [--obstacle-velocity VX,VY,VZ]   every --obstacle moves: domain units per unit time, the unit of\n"
            "                      the velocity fields (advect traces back dt*N*u cells, so the solids are displaced by V*t*N\n"
            "                      cells); needs --obstacle-transport, not with --maccormack vel|both; the mask and the\n"
            "                      velocity are set again before each step, outside the reported step time\n"
            "                 [--loopback --rank R --world W] [--help]\n");
}

// "a,b,c" -> three finite numbers (integers only if `whole`)
static bool parse_triple(const std::string& s, bool whole, double* out) {
    size_t at = 0;
    for (int q = 0; q < 3; ++q) {
        const size_t c = q < 2 ? s.find(',', at) : std::string::npos;
        if (q < 2 && c == std::string::npos) return false;
        const std::string part = s.substr(at, c == std::string::npos ? c : c - at);
        char* end = nullptr;
        out[q] = strtod(part.c_str(), &end);
        if (part.empty() || *end != 0 || !std::isfinite(out[q])) return false;
        if (whole && (out[q] != std::floor(out[q]) || std::fabs(out[q]) > 1e6)) return false;
        at = c + 1;
    }
    return true;
}

// box:I0,J0,K0:I1,J1,K1 (whole indices, I0 <= I1 ...) | sphere:CX,CY,CZ:R (R >= 0)
static bool parse_obstacle(const std::string& spec, Options::Obstacle& ob) {
    const size_t c1 = spec.find(':'), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
    if (c2 == std::string::npos || spec.find(':', c2 + 1) != std::string::npos) return false;
    const std::string kind = spec.substr(0, c1), first = spec.substr(c1 + 1, c2 - c1 - 1), second = spec.substr(c2 + 1);
    if (kind == "box") {
        ob.sphere = false;
        if (!parse_triple(first, true, ob.a) || !parse_triple(second, true, ob.a + 3)) return false;
        return ob.a[0] <= ob.a[3] && ob.a[1] <= ob.a[4] && ob.a[2] <= ob.a[5];
    }
    if (kind == "sphere") {
        ob.sphere = true;
        if (!parse_triple(first, false, ob.a)) return false;
        char* end = nullptr;
        ob.a[3] = strtod(second.c_str(), &end);
        return !second.empty() && *end == 0 && std::isfinite(ob.a[3]) && ob.a[3] >= 0.0;
    }
    return false;
}

// "i+" .. "k-" -> axis 0..2 and from_high (+ enters at the low index)
static bool parse_view(const std::string& v, int& axis, int& high) {
    if (v.size() != 2 || (v[0] != 'i' && v[0] != 'j' && v[0] != 'k') || (v[1] != '+' && v[1] != '-')) return false;
    axis = v[0] - 'i';
    high = v[1] == '-' ? 1 : 0;
    return true;
}

// a whole string as a finite double
static bool parse_double(const std::string& v, double& out) {
    if (v.empty() || std::isspace((unsigned char)v[0])) return false;
    char* end = nullptr;
    out = strtod(v.c_str(), &end);
    return *end == 0 && std::isfinite(out);
}
// a whole string of 1 .. 5 digits as an int in 1 .. 16384
static bool parse_extent(const std::string& v, int& out) {
    if (v.empty() || v.size() > 5 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    out = (int)strtol(v.c_str(), nullptr, 10);
    return out >= 1 && out <= 16384;
}
// DX,DY,DZ:WxH:SIGMA[:STEP] into the view members of o
static bool parse_render_view(const std::string& spec, Options& o) {
    std::vector<std::string> part;
    for (size_t at = 0;;) {
        const size_t c = spec.find(':', at);
        part.push_back(spec.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    if (part.size() < 3 || part.size() > 4) return false;
    const size_t c1 = part[0].find(','), c2 = c1 == std::string::npos ? c1 : part[0].find(',', c1 + 1);
    if (c2 == std::string::npos || part[0].find(',', c2 + 1) != std::string::npos) return false;
    if (!parse_double(part[0].substr(0, c1), o.view_dir[0]) || !parse_double(part[0].substr(c1 + 1, c2 - c1 - 1), o.view_dir[1]) ||
        !parse_double(part[0].substr(c2 + 1), o.view_dir[2]))
        return false;
    if (o.view_dir[0] == 0.0 && o.view_dir[1] == 0.0 && o.view_dir[2] == 0.0) return false;
    const size_t x = part[1].find('x');
    if (x == std::string::npos || !parse_extent(part[1].substr(0, x), o.view_w) || !parse_extent(part[1].substr(x + 1), o.view_h))
        return false;
    if (!parse_double(part[2], o.view_sigma) || o.view_sigma < 0.0) return false;
    o.view_step = 1.0;
    if (part.size() == 4 && (!parse_double(part[3], o.view_step) || !(o.view_step > 0.0))) return false;
    return true;
}

// X,Y,Z as three finite doubles
static bool parse_triple(const std::string& v, double out[3]) {
    const size_t c1 = v.find(','), c2 = c1 == std::string::npos ? c1 : v.find(',', c1 + 1);
    if (c2 == std::string::npos || v.find(',', c2 + 1) != std::string::npos) return false;
    return parse_double(v.substr(0, c1), out[0]) && parse_double(v.substr(c1 + 1, c2 - c1 - 1), out[1]) &&
           parse_double(v.substr(c2 + 1), out[2]);
}
// the vertical of --render-camera: k, or j for a camera that looks along k
static void camera_up(const Options& o, double up[3]) {
    const bool along_k = o.cam_eye[0] == o.cam_target[0] && o.cam_eye[1] == o.cam_target[1];
    up[0] = 0.0, up[1] = along_k ? 1.0 : 0.0, up[2] = along_k ? 0.0 : 1.0;
}
// EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]] into the camera members of o
static bool parse_render_camera(const std::string& spec, Options& o) {
    std::vector<std::string> part;
    for (size_t at = 0;;) {
        const size_t c = spec.find(':', at);
        part.push_back(spec.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    if (part.size() < 4 || part.size() > 6) return false;
    if (!parse_triple(part[0], o.cam_eye) || !parse_triple(part[1], o.cam_target)) return false;
    if (o.cam_eye[0] == o.cam_target[0] && o.cam_eye[1] == o.cam_target[1] && o.cam_eye[2] == o.cam_target[2]) return false;
    const size_t x = part[2].find('x');
    if (x == std::string::npos || !parse_extent(part[2].substr(0, x), o.cam_w) || !parse_extent(part[2].substr(x + 1), o.cam_h))
        return false;
    if (!parse_double(part[3], o.cam_sigma) || o.cam_sigma < 0.0) return false;
    o.cam_fov = 40.0, o.cam_step = 1.0;
    if (part.size() >= 5 && (!parse_double(part[4], o.cam_fov) || !(o.cam_fov > 0.0) || !(o.cam_fov < 180.0))) return false;
    if (part.size() == 6 && (!parse_double(part[5], o.cam_step) || !(o.cam_step > 0.0))) return false;
    return true;
}

static Options parse(int argc, char** argv) {
    Options o;
    o.rank = env_int("RANK", 0);
    o.world = env_int("WORLD_SIZE", 1);
    o.local_rank = env_int("LOCAL_RANK", 0);
    bool rank_or_world_given = false;
    for (int a = 1; a < argc; ++a) {
        const std::string s = argv[a];
        auto next = [&]() -> const char* {
            if (a + 1 >= argc) {
                fprintf(stderr, "missing value after %s\n", s.c_str());
                exit(2);
            }
            return argv[++a];
        };
        if (s == "--n") o.n = atoi(next());
        else if (s == "--steps") o.steps = atoi(next());
        else if (s == "--iters") o.iters = atoi(next());
        else if (s == "--every") o.every = atoi(next());
        else if (s == "--device") o.device = atoi(next());
        else if (s == "--slabs") o.slabs = atoi(next());
        else if (s == "--out") o.out = next();
        else if (s == "--dtype") o.f64 = (std::string(next()) == "f64");
        else if (s == "--binary") o.binary = true;
        else if (s == "--plumbing") o.plumbing = true;
        else if (s == "--quiet") o.quiet = true;
        else if (s == "--sync-output") o.sync_output = true;
        else if (s == "--tracers") o.tracers = atoi(next());
        else if (s == "--vorticity") o.vorticity = atof(next());
        else if (s == "--buoyancy") o.buoyancy = atof(next());
        else if (s == "--ambient") o.ambient = atof(next());
        else if (s == "--buoyancy-axis") o.buoyancy_axis = atoi(next());
        else if (s == "--monitor") {
            o.monitor = atoi(next());
            if (o.monitor < 1) {
                fprintf(stderr, "--monitor takes a step count >= 1\n");
                exit(2);
            }
        }
        else if (s == "--pressure-sync") {
            const std::string ms = next();
            char* end = nullptr;
            const long m = strtol(ms.c_str(), &end, 10);
            if (ms.empty() || *end != 0 || m < 0 || m > 1000000) {
                fprintf(stderr, "--pressure-sync takes a count of iterations >= 0, not %s\n", ms.c_str());
                exit(2);
            }
            o.cg_check_every = (int)m;
        }
        else if (s == "--pressure-precond") {
            // none | jacobi:M
            const std::string spec = next();
            const size_t c = spec.find(':');
            bool ok = spec == "none";
            if (!ok && spec.substr(0, c) == "jacobi" && c != std::string::npos) {
                const std::string ms = spec.substr(c + 1);
                char* end = nullptr;
                const long m = strtol(ms.c_str(), &end, 10);
                ok = !ms.empty() && ms.find_first_not_of("0123456789") == std::string::npos && *end == 0 && m >= 1 &&
                     m <= 1000000;
                if (ok) {
                    o.cg_precond = SF_PRECOND_JACOBI;
                    o.cg_precond_sweeps = (int)m;
                }
            } else if (ok) {
                o.cg_precond = SF_PRECOND_NONE;
                o.cg_precond_sweeps = 0;
            }
            if (!ok) {
                fprintf(stderr, "--pressure-precond takes none or jacobi:M with M >= 1 sweeps, not %s\n", spec.c_str());
                exit(2);
            }
        }
        else if (s == "--pressure-mg") {
            // NU[:LEVELS[:COARSE]]: one to three counts, digits only
            const std::string spec = next();
            long val[3] = {0, 0, 8};
            int n = 0;
            bool ok = true;
            for (size_t at = 0; ok; ++n) {
                const size_t c = spec.find(':', at);
                const std::string part = spec.substr(at, c == std::string::npos ? c : c - at);
                ok = n < 3 && !part.empty() && part.size() <= 6 && part.find_first_not_of("0123456789") == std::string::npos;
                if (ok) val[n] = strtol(part.c_str(), nullptr, 10);
                if (c == std::string::npos) {
                    ++n;
                    break;
                }
                at = c + 1;
            }
            ok = ok && n >= 1 && val[0] >= 1 && val[2] >= 1;
            if (!ok) {
                fprintf(stderr, "--pressure-mg takes NU[:LEVELS[:COARSE]] with NU >= 1 sweeps, LEVELS >= 0 and COARSE >= 1, not %s\n",
                        spec.c_str());
                exit(2);
            }
            o.mg_sweeps = (int)val[0];
            o.mg_levels = (int)val[1];
            o.mg_coarse = (int)val[2];
        }
        else if (s == "--obstacle") {
            const std::string spec = next();
            Options::Obstacle ob{};
            if (!parse_obstacle(spec, ob)) {
                fprintf(stderr, "--obstacle takes box:I0,J0,K0:I1,J1,K1 (whole cell indices, low <= high) or sphere:CX,CY,CZ:R "
                                "(R >= 0), not %s\n", spec.c_str());
                exit(2);
            }
            if (o.obstacles.size() >= 16) {
                fprintf(stderr, "--obstacle may be given 16 times at most\n");
                exit(2);
            }
            o.obstacles.push_back(ob);
        }
        else if (s == "--obstacle-mg") o.obstacle_mg = true;
        else if (s == "--obstacle-transport") o.obstacle_transport = true;
        else if (s == "--obstacle-maccormack") o.obstacle_mc = true;
        else if (s == "--obstacle-velocity") {
            if (!parse_triple(next(), false, o.obstacle_vel)) {
                fprintf(stderr, "--obstacle-velocity takes VX,VY,VZ (finite numbers, domain units per unit time)\n");
                exit(2);
            }
            o.obstacle_moving = true;
        }
        else if (s == "--render") {
            // VIEW:SIGMA[:LIGHT]
            const std::string spec = next();
            const size_t c1 = spec.find(':'), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
            bool ok = c1 != std::string::npos && parse_view(spec.substr(0, c1), o.render_axis, o.render_high);
            if (ok) {
                const std::string ss = spec.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
                char* end = nullptr;
                o.render_sigma = strtod(ss.c_str(), &end);
                ok = !ss.empty() && *end == 0 && std::isfinite(o.render_sigma) && o.render_sigma >= 0.0;
            }
            o.light_axis = -1;
            if (ok && c2 != std::string::npos) ok = parse_view(spec.substr(c2 + 1), o.light_axis, o.light_high);
            if (!ok) {
                fprintf(stderr, "--render takes VIEW:SIGMA[:LIGHT] (VIEW, LIGHT one of i+ i- j+ j- k+ k-, SIGMA >= 0), not %s\n",
                        spec.c_str());
                exit(2);
            }
        }
        else if (s == "--render-view") {
            const std::string spec = next();
            sf_view_params probe;
            o.view = parse_render_view(spec, o);
            if (o.view) {  // (the frame depends on --n, which may follow: built when the run starts; here only what N cannot mend)
                const double upv[3] = {0.0, (o.view_dir[0] == 0.0 && o.view_dir[1] == 0.0) ? 1.0 : 0.0,
                                       (o.view_dir[0] == 0.0 && o.view_dir[1] == 0.0) ? 0.0 : 1.0};
                o.view = sf_view_frame(1, o.view_dir, upv, o.view_w, o.view_h, 1.0, o.view_sigma, &probe) == SF_OK;
            }
            if (!o.view) {
                fprintf(stderr, "--render-view takes DX,DY,DZ:WxH:SIGMA[:STEP] (a direction that is not zero, W and H in 1 .. 16384, "
                                "SIGMA >= 0, STEP > 0), not %s\n", spec.c_str());
                exit(2);
            }
        }
        else if (s == "--render-camera") {
            const std::string spec = next();
            o.camera = parse_render_camera(spec, o);  // (whether the box is in front of the camera depends on --n: when the run starts)
            if (!o.camera) {
                fprintf(stderr, "--render-camera takes EX,EY,EZ:TX,TY,TZ:WxH:SIGMA[:FOV_DEG[:STEP]] (an eye and a target that differ, W "
                                "and H in 1 .. 16384, SIGMA >= 0, 0 < FOV_DEG < 180, STEP > 0), not %s\n", spec.c_str());
                exit(2);
            }
        }
        else if (s == "--help") {
            usage(stdout);
            exit(0);
        }
        else if (s == "--maccormack") {
            const std::string which = next();
            if (which != "vel" && which != "dens" && which != "both") {
                fprintf(stderr, "--maccormack takes vel, dens or both, not %s\n", which.c_str());
                exit(2);
            }
            if (which != "dens") o.advect_vel = SF_ADVECT_MACCORMACK;
            if (which != "vel") o.advect_dens = SF_ADVECT_MACCORMACK;
        }
        else if (s == "--pressure") {
            // jacobi | cg | cg:tol | cg:tol:max_iters
            const std::string spec = next();
            const size_t c1 = spec.find(':'), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
            const std::string which = spec.substr(0, c1);
            bool ok = which == "jacobi" ? c1 == std::string::npos : which == "cg";
            if (ok && c1 != std::string::npos) {
                char* end = nullptr;
                const std::string ts = spec.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
                o.cg_tol = strtod(ts.c_str(), &end);
                ok = !ts.empty() && *end == 0 && std::isfinite(o.cg_tol) && o.cg_tol > 0.0;
                if (ok && c2 != std::string::npos) {
                    const std::string ms = spec.substr(c2 + 1);
                    const long m = strtol(ms.c_str(), &end, 10);
                    ok = !ms.empty() && *end == 0 && m >= 0 && m <= 1000000;
                    o.cg_max_iters = (int)m;
                }
            }
            if (!ok) {
                fprintf(stderr, "--pressure takes jacobi or cg[:tol[:max_iters]] (tol > 0, max_iters >= 0), not %s\n",
                        spec.c_str());
                exit(2);
            }
            o.pressure = which == "cg" ? SF_PRESSURE_CG : SF_PRESSURE_JACOBI;
        }
        // rehearsal of ONE rank's share on a one-GPU box: the geometry, buffers, launches and frame file of rank
        // --rank of --world, halo messages replaced by device-local copies (SF_FLAG_LOOPBACK_HALO), no communicator
        else if (s == "--loopback") o.loopback = true;
        else if (s == "--rank") { o.rank = atoi(next()); rank_or_world_given = true; }
        else if (s == "--world") { o.world = atoi(next()); rank_or_world_given = true; }
        else {
            fprintf(stderr, "unknown option %s\n", s.c_str());
            usage(stderr);
            exit(2);
        }
    }
    // --rank / --world override the launcher's environment only to rehearse one rank's share with local copies: without
    // --loopback a real communicator would wait 120 s for an id nobody publishes
    if (rank_or_world_given && !o.loopback) {
        fprintf(stderr, "--rank / --world need --loopback (ranks of a real run come from RANK / WORLD_SIZE)\n");
        exit(2);
    }
    if (!o.obstacles.empty() && (o.pressure != SF_PRESSURE_CG || (o.mg_sweeps > 0 && !o.obstacle_mg))) {
        fprintf(stderr, "--obstacle needs --pressure cg and does not go with --pressure-mg (docs/SPEC.md §15)\n");
        exit(2);
    }
    if (o.obstacle_transport && o.obstacles.empty()) {
        fprintf(stderr, "--obstacle-transport needs --obstacle (docs/SPEC.md §17)\n");
        exit(2);
    }
    if (o.obstacle_mc && !o.obstacle_transport) {
        fprintf(stderr, "--obstacle-maccormack needs --obstacle-transport (docs/SPEC.md §18)\n");
        exit(2);
    }
    if (o.obstacle_transport && !o.obstacle_mc &&
        (o.advect_vel == SF_ADVECT_MACCORMACK || o.advect_dens == SF_ADVECT_MACCORMACK)) {
        fprintf(stderr, "--obstacle-transport does not go with --maccormack (docs/SPEC.md §17)\n");
        exit(2);
    }
    if (o.obstacle_moving && !o.obstacle_transport) {
        fprintf(stderr, "--obstacle-velocity needs --obstacle-transport (docs/SPEC.md §19)\n");
        exit(2);
    }
    if (o.obstacle_moving && o.advect_vel == SF_ADVECT_MACCORMACK) {
        fprintf(stderr, "--obstacle-velocity does not go with --maccormack vel|both (docs/SPEC.md §19)\n");
        exit(2);
    }
    // frames go to <out>/: create it (the reference writes into the working directory, which always exists)
    if (o.every > 0) {
        std::error_code ec;
        std::filesystem::create_directories(o.out, ec);
    }
    return o;
}

// Analytic inputs of docs/SPEC.md §5, evaluated in double and rounded to T: ONE field on the global planes [kb, ke)
// this process stores (never the whole (N+2)^3 array: at 1024^3 that is 4.3 GB per field and rank).
// which: 0 u, 1 v, 2 w, 3 dens, 4 su, 5 sv, 6 sw, 7 sd.
template <class T>
static std::vector<T> make_input(int which, int N, int kb, int ke, double dt, bool plumbing) {
    const size_t S = (size_t)N + 2;
    std::vector<T> f(S * S * (size_t)(ke - kb), T(0));
    const double PI2 = 6.283185307179586476925286766559;
    const double A = 0.5 / (dt * N);
    auto at = [&](int i, int j, int k) -> T& { return f[(size_t)i + S * ((size_t)j + S * (size_t)(k - kb))]; };
    if (!plumbing && (which == 0 || which == 1 || which == 3)) {
        std::vector<double> sn(S), cs(S);
        for (int i = 1; i <= N; ++i) {
            sn[i] = std::sin(PI2 * (i - 0.5) / N);
            cs[i] = std::cos(PI2 * (i - 0.5) / N);
        }
        for (int k = std::max(kb, 1); k < std::min(ke, N + 1); ++k)
            for (int j = 1; j <= N; ++j)
                for (int i = 1; i <= N; ++i) {
                    if (which == 0) at(i, j, k) = (T)(A * sn[i] * cs[j]);
                    if (which == 1) at(i, j, k) = (T)(-A * cs[i] * sn[j]);
                    if (which == 3) at(i, j, k) = (T)(0.5 + 0.5 * sn[i] * sn[j] * sn[k]);
                }
    }
    const int c = N / 2 > 0 ? N / 2 : 1;
    if (c >= kb && c < ke) {
        if (which == 7) at(c, c, c) = T(100);
        if (which == 5) at(c, c, c) = plumbing ? T(5) : (T)A;
    }
    return f;
}

// The mask of --obstacle on the global planes [kb, ke): 1 in the cells of any obstacle, 0 elsewhere (docs/SPEC.md §15).
// time: every obstacle displaced by --obstacle-velocity * time * N cells (docs/SPEC.md §19; a box by whole cells).
template <class T>
static std::vector<T> make_mask(const Options& o, int kb, int ke, double time = 0.0) {
    const int N = o.n;
    const size_t S = (size_t)N + 2;
    std::vector<T> f(S * S * (size_t)(ke - kb), T(0));
    double sh[3], shw[3];
    for (int q = 0; q < 3; ++q) {
        sh[q] = o.obstacle_vel[q] * time * N;
        shw[q] = std::nearbyint(sh[q]);
    }
    for (const Options::Obstacle& ob : o.obstacles)
        for (int k = std::max(kb, 1); k < std::min(ke, N + 1); ++k)
            for (int j = 1; j <= N; ++j)
                for (int i = 1; i <= N; ++i) {
                    bool in;
                    if (ob.sphere) {
                        const double dx = i - (ob.a[0] + sh[0]), dy = j - (ob.a[1] + sh[1]), dz = k - (ob.a[2] + sh[2]);
                        in = (dx * dx + dy * dy) + dz * dz <= ob.a[3] * ob.a[3];
                    } else {
                        const double ci = i - shw[0], cj = j - shw[1], ck = k - shw[2];
                        in = ci >= ob.a[0] && ci <= ob.a[3] && cj >= ob.a[1] && cj <= ob.a[4] && ck >= ob.a[2] && ck <= ob.a[5];
                    }
                    if (in) f[(size_t)i + S * ((size_t)j + S * (size_t)(k - kb))] = T(1);
                }
    return f;
}

// One frame = the interior cells of global planes [kb, ke) (1-based k; the host arrays hold exactly those planes),
// density scalar + velocity vector, cell centred. Single process: the whole cube as a regular mesh "anim_s<frame>.vtk". Several processes: each rank
// writes its slab "anim_s_GPU<rank>_<frame>.vtk" as a rectilinear mesh whose z coordinates are its plane range.
template <class T>
static void write_frame(const Options& o, int frame, int kb, int ke, const std::vector<T>& dens,
                        const std::vector<T>& u, const std::vector<T>& v, const std::vector<T>& w) {
    const int N = o.n;
    const size_t S = (size_t)N + 2;
    const size_t ncell = (size_t)N * N * (size_t)(ke - kb);
    std::vector<float> d(ncell), vel(3 * ncell);
    size_t q = 0;
    for (int k = kb; k < ke; ++k)
        for (int j = 1; j <= N; ++j)
            for (int i = 1; i <= N; ++i, ++q) {
                const size_t s = (size_t)i + S * ((size_t)j + S * (size_t)(k - kb));  // buffers start at plane kb
                d[q] = (float)dens[s];
                vel[3 * q + 0] = (float)u[s];
                vel[3 * q + 1] = (float)v[s];
                vel[3 * q + 2] = (float)w[s];
            }
    std::ostringstream oss;
    int vardim[2] = {1, 3}, centering[2] = {0, 0};
    const char* names[2] = {"density", "velocity"};
    float* vars[2] = {d.data(), vel.data()};
    if (o.world == 1) {
        oss << o.out << "/anim_s" << frame << ".vtk";
        int dims[3] = {N + 1, N + 1, N + 1};  // point counts; cells = N^3 (visit_writer.cpp:901-905)
        write_regular_mesh(oss.str().c_str(), o.binary ? 1 : 0, dims, 2, vardim, centering, names, vars);
    } else {
        oss << o.out << "/anim_s_GPU" << o.rank << "_" << frame << ".vtk";  // solver-unidyn.cu:484
        int dims[3] = {N + 1, N + 1, ke - kb + 1};
        std::vector<float> xs(N + 1), zs(ke - kb + 1);
        for (int a = 0; a <= N; ++a) xs[a] = (float)a;
        for (int a = 0; a <= ke - kb; ++a) zs[a] = (float)(kb - 1 + a);
        write_rectilinear_mesh(oss.str().c_str(), o.binary ? 1 : 0, dims, xs.data(), xs.data(), zs.data(), 2, vardim,
                               centering, names, vars);
    }
}

// The image of one output step (docs/SPEC.md §12): the pixel rows [row_b, row_e) of colour this rank holds as binary PGM,
// 16 bits big-endian, the highest row first.
template <class T>
static void write_pgm(const std::string& path, const std::vector<T>& colour, int width, int row_b, int row_e) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "Error: cannot write %s\n", path.c_str());
        exit(1);
    }
    fprintf(f, "P5\n%d %d\n65535\n", width, row_e - row_b);
    std::vector<unsigned char> row(2 * (size_t)width);
    for (int b = row_e - 1; b >= row_b; --b) {
        for (int a = 0; a < width; ++a) {
            const double c = (double)colour[(size_t)a + (size_t)width * b];
            const double cl = c > 0.0 ? (c < 1.0 ? c : 1.0) : 0.0;  // NaN -> 0
            const int q = (int)(cl * 65535.0 + 0.5);
            row[2 * a] = (unsigned char)(q >> 8);
            row[2 * a + 1] = (unsigned char)(q & 255);
        }
        fwrite(row.data(), 1, row.size(), f);
    }
    fclose(f);
}
template <class T>
static void write_render(const Options& o, int frame, const std::vector<T>& colour, int row_b, int row_e) {
    char name[64];
    if (o.world == 1)
        snprintf(name, sizeof name, "/render_%04d.pgm", frame);
    else
        snprintf(name, sizeof name, "/render_GPU%d_%04d.pgm", o.rank, frame);
    write_pgm<T>(o.out + name, colour, o.n, row_b, row_e);
}

template <class T>
static int run(const Options& o) {
    const double dt = 0.1, diff = 1e-4, visc = 1e-4;
    sf_params p;
    std::memset(&p, 0, sizeof p);
    p.N = o.n;
    p.dtype = sizeof(T) == 4 ? SF_F32 : SF_F64;
    p.iters = o.iters;
    p.dt = dt;
    p.diff = diff;
    p.visc = visc;
    p.device = (o.world > 1 && !o.loopback) ? o.local_rank : o.device;
    p.flags = o.loopback ? SF_FLAG_LOOPBACK_HALO : 0;
    p.nslabs_local = o.slabs;
    p.rank = o.rank;
    p.nranks = o.world;
    unsigned char nccl_id[SF_NCCL_ID_BYTES];
    if (o.world > 1 && !o.loopback) {
        share_nccl_id(o, nccl_id);
        p.nccl_id = nccl_id;
    }
    int rc = sf_create(&g_ctx, &p);
    if (rc != SF_OK) {
        fprintf(stderr, "Error %s (%s) at line %d in file %s\n", sf_status_string(rc), sf_last_error(nullptr),
                __LINE__, __FILE__);
        exit(1);
    }
    if (o.world > 1 && !o.loopback && o.rank == 0) unlink(nccl_id_path().c_str());  // every rank has joined the communicator
    const bool talk = (o.rank == 0);
    if (talk)
        std::cout << sf_version() << "  N=" << o.n << " K=" << o.iters << " dtype=" << (sizeof(T) == 4 ? "f32" : "f64")
                  << " slabs=" << o.slabs * o.world << " ranks=" << o.world << "\n";
    int own_kb = 1, own_ke = o.n + 1;
    SF_CHECK_RETURN(sf_owned_planes(g_ctx, &own_kb, &own_ke));

    // inputs: only the planes this process stores, one field at a time (host memory per rank stays O(N^3 / ranks))
    int st_kb = 0, st_ke = o.n + 2;
    SF_CHECK_RETURN(sf_stored_planes(g_ctx, &st_kb, &st_ke));
    {
        const int slot[8] = {SF_U, SF_V, SF_W, SF_DENS, SF_USER0, SF_USER1, SF_USER2, SF_USER3};
        for (int q = 0; q < 8; ++q) {
            const std::vector<T> f = make_input<T>(q, o.n, st_kb, st_ke, dt, o.plumbing);
            SF_CHECK_RETURN(sf_upload_planes(g_ctx, slot[q], st_kb, st_ke, f.data()));
        }
    }
    for (int f : {SF_U, SF_V, SF_W}) SF_CHECK_RETURN(sf_set_bnd(g_ctx, f + 1, f));
    SF_CHECK_RETURN(sf_set_bnd(g_ctx, 0, SF_DENS));
    // --obstacle: the mask goes through a slot that is scratch before the first step (every SF_USER slot is bound below)
    // and is read there once
    if (!o.obstacles.empty()) {
        SF_CHECK_RETURN(sf_upload_planes(g_ctx, SF_DENS0, st_kb, st_ke, make_mask<T>(o, st_kb, st_ke).data()));
        SF_CHECK_RETURN(sf_set_obstacles(g_ctx, SF_DENS0));
        SF_CHECK_RETURN(sf_fill(g_ctx, SF_DENS0, 0.0));
        sf_obstacles ob{};
        SF_CHECK_RETURN(sf_obstacles_get(g_ctx, &ob));
        if (o.rank == 0) std::cout << "obstacles: " << o.obstacles.size() << ", fluid cells " << ob.fluid_cells << "\n";
    }
    // sources stay resident in HBM (SF_USER0..3) and are re-injected every step
    const int bound[4] = {SF_USER0, SF_USER1, SF_USER2, SF_USER3};
    SF_CHECK_RETURN(sf_bind_sources(g_ctx, bound[0], bound[1], bound[2], bound[3]));
    // --render with a light: the slot the transmittance towards the light is written to at an output step
    int light_slot = -1;
    if (o.render_axis >= 0 && o.light_axis >= 0) {
        for (int f = SF_USER0; f <= SF_USER3 && light_slot < 0; ++f)
            if (std::find(bound, bound + 4, f) == bound + 4) light_slot = f;
        if (light_slot < 0 && bound[3] >= 0) light_slot = SF_DENS0;  // scratch between steps: its source is bound
        if (light_slot < 0) {
            fprintf(stderr, "--render: no free slot for the light (every SF_USER slot is a bound source)\n");
            exit(2);
        }
    }
    // the pixel rows of the image this rank holds: those of its planes (i / j views), all on the rank a k view leaves from
    int img_b = own_kb - 1, img_e = own_ke - 1;
    if (o.render_axis == 2) {
        const bool mine = o.loopback || o.rank == (o.render_high ? 0 : o.world - 1);
        img_b = 0, img_e = mine ? o.n : 0;
    }
    std::vector<T> colour(o.render_axis >= 0 ? (size_t)o.n * o.n : 0);
    // --render-view: the frame for this N; the image ends on the rank that owns the last slab visited
    sf_view_params vp{};
    bool view_mine = false;
    if (o.view) {
        const bool along_k = o.view_dir[0] == 0.0 && o.view_dir[1] == 0.0;
        const double up[3] = {0.0, along_k ? 1.0 : 0.0, along_k ? 0.0 : 1.0};
        if (sf_view_frame(o.n, o.view_dir, up, o.view_w, o.view_h, o.view_step, o.view_sigma, &vp) != SF_OK) {
            fprintf(stderr, "--render-view: no frame for this direction, step and grid size\n");
            exit(2);
        }
        vp.dens = SF_DENS;
        view_mine = o.loopback || o.rank == ((sizeof(T) == 4 ? (double)(float)vp.step[2] : vp.step[2]) < 0.0 ? 0 : o.world - 1);
    }
    std::vector<T> view_colour(o.view ? (size_t)o.view_w * o.view_h : 0);
    // --render-camera: the frame for this N; the image ends on the rank sf_camera_passes_get names (up: the last, else 0)
    sf_camera_params cp{};
    bool camera_mine = false;
    if (o.camera) {
        double up[3];
        camera_up(o, up);
        int passes = SF_CAMERA_UP;
        if (sf_camera_frame(o.n, o.cam_eye, o.cam_target, up, std::tan(o.cam_fov * (M_PI / 360.0)), o.cam_w, o.cam_h, o.cam_step,
                            o.cam_sigma, &cp) != SF_OK ||
            sf_camera_passes_get(&cp, sizeof(T) == 4 ? SF_F32 : SF_F64, &passes) != SF_OK) {
            fprintf(stderr, "--render-camera: no frame for this camera, step and grid size (is the box behind the camera?)\n");
            exit(2);
        }
        cp.view.dens = SF_DENS;
        camera_mine = o.loopback || o.rank == (passes == SF_CAMERA_UP ? o.world - 1 : 0);
    }
    std::vector<T> camera_colour(o.camera ? (size_t)o.cam_w * o.cam_h : 0);
    // forces (SPEC §8): added by every vel_step to copies of the bound sources
    SF_CHECK_RETURN(sf_set_vorticity_confinement(g_ctx, o.vorticity));
    SF_CHECK_RETURN(sf_set_buoyancy(g_ctx, o.buoyancy, o.ambient, o.buoyancy_axis));
    SF_CHECK_RETURN(sf_set_advection(g_ctx, o.advect_vel, o.advect_dens));
    if (o.pressure != SF_PRESSURE_JACOBI) SF_CHECK_RETURN(sf_set_pressure_solver(g_ctx, o.pressure, o.cg_tol, o.cg_max_iters));
    if (o.cg_check_every > 0) SF_CHECK_RETURN(sf_set_pressure_sync(g_ctx, o.cg_check_every));
    if (o.cg_precond != SF_PRECOND_NONE)
        SF_CHECK_RETURN(sf_set_pressure_preconditioner(g_ctx, o.cg_precond, o.cg_precond_sweeps));
    if (o.mg_sweeps > 0) SF_CHECK_RETURN(sf_set_pressure_multigrid(g_ctx, o.mg_sweeps, o.mg_levels, o.mg_coarse));
    if (o.obstacle_mg) SF_CHECK_RETURN(sf_set_obstacle_multigrid(g_ctx, 1));
    if (o.obstacle_transport) SF_CHECK_RETURN(sf_set_obstacle_transport(g_ctx, 1));
    if (o.obstacle_mc) SF_CHECK_RETURN(sf_set_obstacle_maccormack(g_ctx, 1));

    // frame buffers: the planes this process owns, nothing else
    const size_t n = ((size_t)o.n + 2) * ((size_t)o.n + 2) * (size_t)(own_ke - own_kb);
    std::vector<T> hd, hu, hv, hw;
    if (o.every > 0) {
        hd.resize(n);
        hu.resize(n);
        hv.resize(n);
        hw.resize(n);
    }

    // tracers: a small lattice in the middle of the box, in grid-index coordinates (SPEC §6). Every rank seeds the
    // same global lattice; each keeps the tracers its slabs own (SPEC §6.1).
    std::vector<T> tpos, tdens, tspeed;
    if (o.tracers > 0) {
        int side = 1;
        while (side * side * side < o.tracers) ++side;
        for (int c = 0; c < side && (int)tpos.size() / 3 < o.tracers; ++c)
            for (int b = 0; b < side && (int)tpos.size() / 3 < o.tracers; ++b)
                for (int a = 0; a < side && (int)tpos.size() / 3 < o.tracers; ++a) {
                    tpos.push_back((T)(0.25 * o.n + 0.5 * o.n * (a + 0.5) / side));
                    tpos.push_back((T)(0.25 * o.n + 0.5 * o.n * (b + 0.5) / side));
                    tpos.push_back((T)(0.25 * o.n + 0.5 * o.n * (c + 0.5) / side));
                }
        tdens.resize(tpos.size() / 3);
        tspeed.resize(tpos.size() / 3);
        SF_CHECK_RETURN(sf_tracers_set(g_ctx, (int)(tpos.size() / 3), tpos.data()));
    }
    const int ntr = (int)(tpos.size() / 3);

    std::thread writer;  // at most one frame in flight
    // One process: all tracers in id order, "tracers_s<frame>.vtk". Several: each rank its own tracers in id order,
    // "tracers_s_GPU<rank>_<frame>.vtk" (the per-device naming of the grid frames, solver-unidyn.cu:484).
    int nout = ntr;  // tracers in the frame being written
    auto fetch_tracers = [&]() {
        if (o.world == 1) {
            SF_CHECK_RETURN(sf_tracers_get(g_ctx, tpos.data(), tdens.data(), tspeed.data()));
            nout = ntr;
            return;
        }
        SF_CHECK_RETURN(sf_tracers_owned(g_ctx, &nout));  // <= ntr: the host buffers hold the whole lattice
        SF_CHECK_RETURN(sf_tracers_get_owned(g_ctx, nullptr, tpos.data(), tdens.data(), tspeed.data()));
    };
    auto write_tracers = [&](int frame, int count) {
        std::vector<float> pts(3 * (size_t)count), m(count), sp(count);
        for (int q = 0; q < 3 * count; ++q) pts[q] = (float)tpos[q];
        for (int q = 0; q < count; ++q) {
            m[q] = (float)tdens[q];
            sp[q] = (float)tspeed[q];
        }
        std::ostringstream oss;
        if (o.world == 1)
            oss << o.out << "/tracers_s" << frame << ".vtk";
        else
            oss << o.out << "/tracers_s_GPU" << o.rank << "_" << frame << ".vtk";
        int vardims[2] = {1, 1};
        const char* names[2] = {"density", "speed"};
        float* arrays[2] = {m.data(), sp.data()};
        write_point_mesh(oss.str().c_str(), 0, count, pts.data(), 2, vardims, names, arrays);  // solver-unidyn.cu:487
    };

    double total_ms = 0;
    const auto wall0 = std::chrono::steady_clock::now();
    for (int t = 0; t < o.steps; t++) {
        if (!o.quiet && talk) std::cout << "t= " << t << "\n";
        float elapsedTime = 0.f;
        // --obstacle-velocity: the mask at this step's time and the solid velocity, through slots that are scratch
        // between steps while their sources are bound (SF_DENS0, SF_U0, SF_V0, SF_W0); each is read once, by its call
        if (o.obstacle_moving) {
            SF_CHECK_RETURN(sf_upload_planes(g_ctx, SF_DENS0, st_kb, st_ke, make_mask<T>(o, st_kb, st_ke, t * dt).data()));
            SF_CHECK_RETURN(sf_set_obstacles(g_ctx, SF_DENS0));
            SF_CHECK_RETURN(sf_fill(g_ctx, SF_DENS0, 0.0));
            const int vs[3] = {SF_U0, SF_V0, SF_W0};
            for (int q = 0; q < 3; ++q) SF_CHECK_RETURN(sf_fill(g_ctx, vs[q], o.obstacle_vel[q]));
            SF_CHECK_RETURN(sf_set_obstacle_velocity(g_ctx, SF_U0, SF_V0, SF_W0));
        }
        SF_CHECK_RETURN(sf_timer_start(g_ctx));
        SF_CHECK_RETURN(vel_step(g_ctx));  // sources are bound (sf_bind_sources above)
        SF_CHECK_RETURN(dens_step(g_ctx));
        if (ntr > 0) SF_CHECK_RETURN(sf_tracers_advect(g_ctx));
        SF_CHECK_RETURN(sf_timer_stop(g_ctx, &elapsedTime));
        total_ms += elapsedTime;
        if (!o.quiet && talk) std::cout << "done.\nElapsed kernel time: " << elapsedTime << " ms\n";

        if (o.monitor > 0 && t % o.monitor == 0) {
            sf_diagnostics d;
            SF_CHECK_RETURN(sf_diagnostics_get(g_ctx, &d));  // collective: every rank calls it, rank 0 talks
            if (talk) {
                printf("monitor step=%d mass=%.17g kinetic=%.17g max_div=%.17g cfl=%.17g nonfinite=%lld\n", t, d.mass,
                       d.kinetic, d.max_div, d.cfl, d.nonfinite);
                sf_pressure_info pi;
                SF_CHECK_RETURN(sf_pressure_info_get(g_ctx, &pi));
                static const char* const status[3] = {"converged", "max_iters", "breakdown"};
                printf("pressure step=%d solver=%s status=%s iterations=%d rel_residual=%.17g iterations_total=%lld\n", t,
                       pi.solver == SF_PRESSURE_CG ? "cg" : "jacobi", status[pi.status], pi.iterations, pi.rel_residual,
                       pi.iterations_total);
                fflush(stdout);
            }
            if (d.nonfinite > 0) {
                if (talk)
                    fprintf(stderr, "Error: %lld cells are not finite after step %d: the run has blown up\n", d.nonfinite, t);
                if (writer.joinable()) writer.join();
                exit(3);
            }
        }

        if (o.every > 0 && t % o.every == 0) {
            const int frame = t / o.every;
            if (writer.joinable()) writer.join();  // the previous frame must be out before its buffers are reused
            if (o.render_axis >= 0) {
                if (light_slot >= 0)
                    SF_CHECK_RETURN(sf_light(g_ctx, light_slot, SF_DENS, o.light_axis, o.light_high, o.render_sigma));
                const sf_render_params rp = {o.render_axis, o.render_high, o.render_sigma, SF_DENS, light_slot};
                SF_CHECK_RETURN(sf_render(g_ctx, &rp));
                SF_CHECK_RETURN(sf_render_read(g_ctx, colour.data(), nullptr));
                if (img_e > img_b) write_render<T>(o, frame, colour, img_b, img_e);
            }
            if (o.view) {
                SF_CHECK_RETURN(sf_render_view(g_ctx, &vp));
                SF_CHECK_RETURN(sf_render_view_read(g_ctx, view_colour.data(), nullptr));
                if (view_mine) {
                    char name[64];
                    snprintf(name, sizeof name, "/view_%04d.pgm", frame);
                    write_pgm<T>(o.out + name, view_colour, o.view_w, 0, o.view_h);
                }
            }
            if (o.camera) {
                SF_CHECK_RETURN(sf_render_camera(g_ctx, &cp));
                SF_CHECK_RETURN(sf_render_view_read(g_ctx, camera_colour.data(), nullptr));
                if (camera_mine) {
                    char name[64];
                    snprintf(name, sizeof name, "/camera_%04d.pgm", frame);
                    write_pgm<T>(o.out + name, camera_colour, o.cam_w, 0, o.cam_h);
                }
            }
            if (ntr > 0) fetch_tracers();
            if (o.sync_output) {
                SF_CHECK_RETURN(sf_sync(g_ctx));
                SF_CHECK_RETURN(sf_download_planes(g_ctx, SF_DENS, own_kb, own_ke, hd.data()));
                SF_CHECK_RETURN(sf_download_planes(g_ctx, SF_U, own_kb, own_ke, hu.data()));
                SF_CHECK_RETURN(sf_download_planes(g_ctx, SF_V, own_kb, own_ke, hv.data()));
                SF_CHECK_RETURN(sf_download_planes(g_ctx, SF_W, own_kb, own_ke, hw.data()));
                write_frame<T>(o, frame, own_kb, own_ke, hd, hu, hv, hw);
                if (ntr > 0) write_tracers(frame, nout);
            } else {
                const int fields[4] = {SF_DENS, SF_U, SF_V, SF_W};
                SF_CHECK_RETURN(sf_snapshot(g_ctx, fields, 4));
                writer = std::thread([&, frame, count = nout]() {
                    T* dst[4] = {hd.data(), hu.data(), hv.data(), hw.data()};
                    for (int q = 0; q < 4; ++q)
                        if (sf_snapshot_read_planes(g_ctx, q, own_kb, own_ke, dst[q]) != SF_OK) {
                            fprintf(stderr, "Error: snapshot read failed for frame %d\n", frame);
                            exit(1);
                        }
                    write_frame<T>(o, frame, own_kb, own_ke, hd, hu, hv, hw);
                    if (ntr > 0) write_tracers(frame, count);
                });
            }
        }
    }
    if (writer.joinable()) writer.join();
    SF_CHECK_RETURN(sf_sync(g_ctx));
    const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
    if (talk) std::cout << "wall time of the loop incl. output: " << wall_s << " s ("
              << (o.sync_output ? "synchronous" : "asynchronous") << " output)\n";
    const double cells = (double)o.n * o.n * o.n;
    if (o.steps > 0 && talk)
        std::cout << "mean step " << total_ms / o.steps << " ms, " << cells * o.steps / (total_ms * 1e-3) / 1e6
                  << " Mcells/s\n";
    sf_destroy(g_ctx);
    g_ctx = nullptr;
    return 0;
}

int main(int argc, char** argv) {
    const Options o = parse(argc, argv);
    return o.f64 ? run<double>(o) : run<float>(o);
}
