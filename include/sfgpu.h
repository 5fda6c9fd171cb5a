/* include/sfgpu.h — C ABI of libsfgpu.so: the MI355X (gfx950) stable-fluids hot path.
 *
 * What this replaces in the reference (robbergen/FluidSolverGPU): the reference has NO plugin /
 * FFI boundary — its host loop launches kernels with <<<>>> on raw device pointers inside one
 * program (kernel prototypes FluidGPU.cuh:417-419, FluidGPU-unidyn.cuh:537-544; host loop
 * solver.cu:171-216, solver-unidyn.cu:313-573) and owns every buffer in main() (solver.cu:74-106).
 * BASELINE.json's north_star asks for "dens_step / vel_step entry points ... host code in C++
 * calling HIP through a thin C-ABI"; this header is that boundary. Per entry point
 * the comment names the reference site whose role it takes.
 *
 * Conventions
 *   - Every function returns an sf_status (0 = SF_OK). No exception crosses the boundary.
 *     sf_last_error() gives the message; a driver prints it and exits, mirroring the reference's
 *     CUDA_CHECK_RETURN (FluidGPU.cuh:34-41).
 *   - Host arrays are dense (N+2)^3, x fastest: IX(i,j,k) = i + (N+2)*(j + (N+2)*k), element type
 *     float (SF_F32) or double (SF_F64). The caller owns host memory; the context owns all device
 *     memory, streams, events and the RCCL communicator. Device layout (pitched rows, ghost planes)
 *     is internal.
 *   - Step functions are asynchronous on the context's streams; sf_sync() waits and reports
 *     deferred errors. One context per host thread; contexts are independent.
 *   - Numerics are those of docs/SPEC.md, bit-for-bit.
 */
#ifndef SFGPU_H
#define SFGPU_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sf_ctx sf_ctx;

typedef enum sf_status {
    SF_OK = 0,
    SF_ERR_INVALID = 1,       /* bad argument */
    SF_ERR_HIP = 2,           /* a HIP runtime call failed (message has hipGetErrorString) */
    SF_ERR_RCCL = 3,          /* an RCCL call failed */
    SF_ERR_HALO_EXCEEDED = 4, /* advect back-traced beyond the slab's ghost plane (SPEC §4) */
    SF_ERR_NO_DEVICE = 5,     /* no usable gfx950 device: there is NO CPU fallback */
    SF_ERR_TRACER_OVERFLOW = 6 /* more tracers left a slab for one neighbour in one call than the capacity holds */
} sf_status;

typedef enum sf_dtype { SF_F32 = 0, SF_F64 = 1 } sf_dtype;

/* Field slots. p and div of project() alias SF_U0 and SF_V0 (SPEC §1). SF_USER0..3 are extra
 * resident slots (e.g. per-step sources kept in HBM), allocated on first use. */
typedef enum sf_field {
    SF_U = 0, SF_V = 1, SF_W = 2, SF_U0 = 3, SF_V0 = 4, SF_W0 = 5, SF_DENS = 6, SF_DENS0 = 7,
    SF_USER0 = 8, SF_USER1 = 9, SF_USER2 = 10, SF_USER3 = 11, SF_NUM_FIELDS = 12
} sf_field;

#define SF_NCCL_ID_BYTES 128

typedef struct sf_params {
    int N;            /* interior cells per axis (>= 1)                                         */
    int dtype;        /* sf_dtype                                                               */
    int iters;        /* Jacobi iterations K per lin_solve                                      */
    double dt, diff, visc;
    int device;       /* HIP device ordinal for this process                                    */
    int nslabs_local; /* logical k-slabs held by this context (>= 1); total = nranks * this     */
    int rank, nranks; /* this process / number of processes (one per GPU). nranks == 1: no RCCL */
    const void* nccl_id; /* SF_NCCL_ID_BYTES from sf_nccl_unique_id() of rank 0 when nranks > 1 */
    int flags;        /* 0, or SF_FLAG_* bits                                                   */
} sf_params;

/* Measurement aid: the context takes the geometry, streams and launch schedule of rank `rank` of `nranks`, but the
 * halo messages to ranks in other processes become device-local copies of its own planes of the same size and no
 * communicator is created (nccl_id may be NULL). Timing of one rank's share on a single GPU; the field values
 * next to the slab boundaries are then meaningless. */
#define SF_FLAG_LOOPBACK_HALO 1

/* Verification aid for the inter-process data plane on a ONE-GPU box (RCCL refuses two ranks on one device):
 * nranks == 1, nslabs_local >= 2, and the ghost planes of the logical slabs travel through a real single-rank RCCL
 * communicator as grouped ncclSend / ncclRecv to self — the same calls, counts, datatypes, buffer offsets, streams
 * and system-scope halo event as the multi-process exchange (whose role is that of the reference's 2-GPU buffer
 * exchange, solver-unidyn.cu:396-470) — instead of the device-local copy kernel. Results are bit-identical to the
 * copy transport and to the undecomposed solve; sf_create also runs the schedule measurement and its all-reduce
 * vote over that communicator, as a multi-process context does. */
#define SF_FLAG_RCCL_SELF 2

/* Library / build identification ("sfgpu <ver> gfx950 hip"). */
const char* sf_version(void);
const char* sf_status_string(int status);

/* Fills `out` (SF_NCCL_ID_BYTES) with a fresh ncclUniqueId; rank 0 calls it and ships the bytes to
 * the other ranks by any means (bench.py uses torch.distributed). */
int sf_nccl_unique_id(void* out);

/* Takes the role of the allocation block of solver.cu:74-106 / solver-unidyn.cu:90-114:
 * all fields, streams and (nranks > 1) the communicator. *out is NULL on failure; the message is
 * then available from sf_last_error(NULL). N must be divisible by nranks*nslabs_local. */
int sf_create(sf_ctx** out, const sf_params* p);
void sf_destroy(sf_ctx* ctx);

/* Host <-> device copies (cudaMemcpy sites solver.cu:131,151,168-169; solver-unidyn.cu:475).
 * `host` is the dense GLOBAL (N+2)^3 array; each context reads / writes only the planes of its own
 * slabs (download: planes it owns, plus the physical shell planes on the end slabs). Synchronous. */
int sf_upload(sf_ctx* ctx, int field, const void* host);
int sf_download(sf_ctx* ctx, int field, void* host);
/* Same for a run of whole planes: global k in [k_begin, k_end) must lie inside this context's
 * stored range; host points at plane k_begin ((N+2)^2 elements per plane). */
int sf_download_planes(sf_ctx* ctx, int field, int k_begin, int k_end, void* host);
int sf_upload_planes(sf_ctx* ctx, int field, int k_begin, int k_end, const void* host);
/* First / one-past-last global interior plane owned by this context (1-based k). sf_upload_planes
 * accepts any [k_begin, k_end) and copies the planes of it that this context STORES (its interior
 * planes and the ghost / shell plane either side), so a rank can upload just its own part. */
int sf_owned_planes(const sf_ctx* ctx, int* k_begin, int* k_end);
/* Global planes [k_begin, k_end) this context stores (owned planes plus its ghost / shell planes, clipped
 * to 0 .. N+2): the range a rank should fill with sf_upload_planes before the first step. */
int sf_stored_planes(const sf_ctx* ctx, int* k_begin, int* k_end);

/* Device-side helpers, asynchronous. */
int sf_fill(sf_ctx* ctx, int field, double value);        /* every stored entry = value           */
int sf_copy_field(sf_ctx* ctx, int dst, int src);         /* dst <- src (device to device)        */

/* The two entry points north_star names. They take the place of the per-step kernel sequence of the
 * reference loop (solver.cu:181-198; solver-unidyn.cu:324-393). Sources are whatever is currently in
 * SF_U0/V0/W0 (vel_step) and SF_DENS0 (dens_step); on return those slots hold scratch (SPEC §3). */
int vel_step(sf_ctx* ctx);
int dens_step(sf_ctx* ctx);

/* Resident sources. After sf_bind_sources(ctx, su, sv, sw, sd) every vel_step / dens_step behaves exactly as if
 * SF_U0, SF_V0, SF_W0 (vel_step) and SF_DENS0 (dens_step) had first been overwritten with copies of the bound
 * slots (normally SF_USER0..3) — same bits, one pass less over memory than sf_copy_field + the step. Pass -1 for
 * a source that stays "whatever is in the x0 slot"; sf_bind_sources(ctx, -1, -1, -1, -1) restores the default. */
int sf_bind_sources(sf_ctx* ctx, int su, int sv, int sw, int sd);

/* The operators of the path, exposed singly for parity tests and for timing the Jacobi sweep in
 * isolation. Field arguments are sf_field slots; `b` is the boundary mode 0..3. */
int sf_add_source(sf_ctx* ctx, int x, int s);
int sf_set_bnd(sf_ctx* ctx, int b, int x);
int sf_lin_solve(sf_ctx* ctx, int b, int x, int x0, double a, double c, int iters);
int sf_diffuse(sf_ctx* ctx, int b, int x, int x0, double diff);
int sf_advect(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w);
int sf_project(sf_ctx* ctx, int u, int v, int w, int p, int div);

/* External forces of docs/SPEC.md §8 (Fedkiw, Stam & Jensen, "Visual Simulation of Smoke", SIGGRAPH 2001).
 * With a non-zero coefficient, vel_step first adds the forces of the state at entry to its sources (the x0 slots, or
 * copies of the bound slots written into them), then runs as before; with both zero it is the §3 step exactly.
 * Coefficients are per context and, like sf_set_coefficients, must be the same on every rank.
 *   eps:  vorticity confinement strength (finite, >= 0; 0 = off, the default); the force is eps*h*(n x omega).
 *   beta: buoyancy beta*(dens - ambient) added to velocity component `axis` (0 = u, 1 = v, 2 = w); finite; 0 = off. */
int sf_set_vorticity_confinement(sf_ctx* ctx, double eps);
int sf_set_buoyancy(sf_ctx* ctx, double beta, double ambient, int axis);
/* The two passes singly. sf_vorticity_magnitude: dst = |curl(u, v, w)| on interior cells, then set_bnd(0, dst);
 * dst must not be u, v or w. sf_add_forces: su, sv, sw += the forces of (u, v, w, dens) on interior cells, with the
 * coefficients in force (a zero coefficient's term is not evaluated); all seven slots distinct. */
int sf_vorticity_magnitude(sf_ctx* ctx, int u, int v, int w, int dst);
int sf_add_forces(sf_ctx* ctx, int u, int v, int w, int dens, int su, int sv, int sw);

/* MacCormack advection of docs/SPEC.md §9 (Selle, Fedkiw, Kim, Liu & Rossignac, "An Unconditionally Stable MacCormack
 * Method", J. Sci. Comput. 2008): second order, built from two first-order advects and limited to the extrema of the
 * cells the back-trace interpolates; first order wherever a trace was clamped at a wall.
 * sf_set_advection selects the scheme vel_step uses for its three advects and dens_step for its one. Both default
 * to SF_ADVECT_SEMI_LAGRANGIAN, the §3 step exactly; any other value is SF_ERR_INVALID. The choice is per context
 * and, like sf_set_coefficients, must be the same on every rank. On a decomposed grid the condition of sf_advect
 * (|dt*N*w| < 1, else SF_ERR_HALO_EXCEEDED at the next sf_sync) holds for both traces. */
enum sf_advection { SF_ADVECT_SEMI_LAGRANGIAN = 0, SF_ADVECT_MACCORMACK = 1 };
int sf_set_advection(sf_ctx* ctx, int velocity_scheme, int density_scheme);
/* The operator singly: d = advect_mc(b, d0; u, v, w) with the context's dt, set_bnd(b, d) included. As with
 * sf_advect the output must not alias an input. */
int sf_advect_maccormack(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w);

/* Asynchronous frame output (the reference blocks on cudaDeviceSynchronize + cudaMemcpy +
 * per-value sprintf every output step, solver-unidyn.cu:475-487). sf_snapshot copies up to 4 fields into
 * context-owned snapshot buffers on the compute stream (device to device, ordered after everything issued
 * so far) and returns at once. sf_snapshot_read(index, host) waits for that copy only, then downloads snapshot
 * `index` as a dense global (N+2)^3 array on a separate copy stream. It may be called from ANOTHER host
 * thread while the owner keeps stepping; do not call sf_snapshot again before all reads have returned. */
int sf_snapshot(sf_ctx* ctx, const int* fields, int nfields);
int sf_snapshot_read(sf_ctx* ctx, int index, void* host);
/* The same for global planes [k_begin, k_end) only; `host` holds exactly those planes, dense (N+2)^2 each (what a
 * rank of a decomposed run needs for its own frame file: solver-unidyn.cu:484-490 writes one file per device). */
int sf_snapshot_read_planes(sf_ctx* ctx, int index, int k_begin, int k_end, void* host);

/* Tracer particles (docs/SPEC.md §6, §6.1; feeds the write_point_mesh call of solver-unidyn.cu:487). Positions are
 * x y z triples in grid-index coordinates, element type = the context's dtype. A tracer's id is its index in the
 * array given to sf_tracers_set; positions are kept raw (a set followed by a get returns the caller's values).
 * sf_tracers_advect moves them through SF_U/V/W by one dt; sf_tracers_get returns positions and, if the pointers
 * are non-NULL, the density and speed sampled at each tracer, all n in id order.
 * Decomposed contexts: each slab holds the tracers whose sample reads its planes and hands them to the neighbouring
 * slab when they cross into it; results are bit-identical to one slab. A tracer that moves past a neighbouring slab
 * in one call is reported by sf_sync as SF_ERR_HALO_EXCEEDED. On several ranks every rank passes the same global
 * array to sf_tracers_set, and sf_tracers_set and sf_tracers_advect are collective (every rank calls them, as with
 * vel_step); sf_tracers_get then fails with SF_ERR_INVALID: each rank reads its own with sf_tracers_get_owned. */
int sf_tracers_set(sf_ctx* ctx, int n, const void* xyz);
int sf_tracers_advect(sf_ctx* ctx);
int sf_tracers_get(sf_ctx* ctx, void* xyz, void* dens_sample, void* speed_sample);
/* Number of tracers this context holds now (all n on one slab). Synchronises. */
int sf_tracers_owned(const sf_ctx* ctx, int* n_owned);
/* This context's tracers in ascending id order: ids (int), positions and samples as in sf_tracers_get, each array
 * sized by sf_tracers_owned; any pointer may be NULL. What one rank writes into its own point-mesh file. */
int sf_tracers_get_owned(sf_ctx* ctx, int* ids, void* xyz, void* dens_sample, void* speed_sample);
/* The most tracers one slab may hand to one neighbour in one sf_tracers_advect (default: the tracer count, which
 * never overflows). Sizes the per-direction message buffers; must be the same on every rank. More migrants than
 * that are kept by the slab they leave and reported by sf_sync as SF_ERR_TRACER_OVERFLOW. */
int sf_tracers_set_capacity(sf_ctx* ctx, int per_direction);

/* Reductions and diagnostics of docs/SPEC.md §10: what the context can say about the state it holds without a
 * download. Every result is a double whose bits are fixed by the SPEC — interior cells only, a double accumulator, a
 * sum tree of row partials, plane partials and a total in global k order — so it is the same for every decomposition
 * (nslabs_local, nranks), transport and SF_* switch, and equals the numpy reference tests/diagnostics_ref.py bit for
 * bit. No float atomics anywhere.
 *   - Collective: with nranks > 1 every rank calls them (like vel_step); the ranks all-gather their per-plane records
 *     over the context's communicator and each folds all N of them, so every rank returns the same bits.
 *     SF_FLAG_RCCL_SELF contexts send their records through the same collective on their one-rank communicator (it
 *     counts as one group in sf_transport_info). SF_FLAG_LOOPBACK_HALO contexts have no communicator and reduce their
 *     own planes only: meaningless, like their fields.
 *   - Synchronising: both calls wait for the context's compute streams, like sf_timer_stop, and return the result to
 *     the host. They issue no halo exchange (ghost planes are current after every operator and upload), write no
 *     field, and change no later step by a bit. A step that never calls them issues exactly the launches it did.
 *   - A bad op, a slot out of range or a NULL pointer is SF_ERR_INVALID; an SF_USER slot not yet used is allocated
 *     (zeros) first, as elsewhere.
 * sf_reduce(op, field): SUM and SUM_SQ add x and x*x (each converted to double first); MIN, MAX and MAX_ABS select
 * among the FINITE cells only (NaN and +-inf are never taken) and return +inf, -inf and +0 when there is none — a zero
 * result is always +0; COUNT_NONFINITE is the number of NaN / +-inf cells, as a double. A sum over a field that holds a
 * NaN is a NaN (payload unspecified). */
enum sf_reduce_op { SF_RED_SUM = 0, SF_RED_SUM_SQ = 1, SF_RED_MIN = 2, SF_RED_MAX = 3,
                    SF_RED_MAX_ABS = 4, SF_RED_COUNT_NONFINITE = 5 };
int sf_reduce(sf_ctx* ctx, int op, int field, double* out);

/* One pass over SF_U, SF_V, SF_W, SF_DENS (docs/SPEC.md §10 "state diagnostics").
 *   mass       sum of dens
 *   dens_min, dens_max
 *   kinetic    0.5 * sum((u^2 + v^2) + w^2) / N^3, squares and adds in double
 *   max_speed  sqrt(max((u^2 + v^2) + w^2))
 *   max_div    max |c_div*(((u[i+1]-u[i-1]) + (v[j+1]-v[j-1])) + (w[k+1]-w[k-1]))| with c_div = -0.5/N: SPEC §3's own
 *              expression, evaluated in the context's precision, so it equals sf_reduce(SF_RED_MAX_ABS, div) of the div
 *              slot sf_project leaves when run on the same velocity. The physical divergence (central differences
 *              with h = 1/N) is max_div * N^2 in magnitude.
 *   cfl_x, cfl_y, cfl_z   max |dt*N*u|, |dt*N*v|, |dt*N*w|: the product advect forms, in cells per step. cfl_z < 1 is
 *              literally the condition of SPEC §4 under which a decomposed advect equals the undecomposed one (else
 *              SF_ERR_HALO_EXCEEDED): test it BEFORE the step instead of learning of it afterwards.
 *   cfl        the largest of the three
 *   nonfinite  interior cells where any of the four fields is NaN or +-inf. Minima and maxima skip terms that are not
 *              finite, so this count is how a blow-up shows. */
typedef struct sf_diagnostics { double mass, dens_min, dens_max, kinetic, max_speed, max_div,
                                cfl_x, cfl_y, cfl_z, cfl; long long nonfinite; } sf_diagnostics;
int sf_diagnostics_get(sf_ctx* ctx, sf_diagnostics* out);

/* Conjugate-gradient projection of docs/SPEC.md §11. K Jacobi sweeps do not solve the pressure equation on any grid of
 * interest (the long modes of an N^3 grid need ~N^2 sweeps); unpreconditioned CG on the same operator
 * A p = 6 p - (sum of the six neighbours), mirror shells of set_bnd(0, .), does in tens of iterations. Its inner
 * products are §10 sums, so the result has the same bits for every decomposition and transport and equals the numpy
 * reference tests/pressure_cg_ref.py.
 *   sf_project_cg(u, v, w, p, div, tol, max_iters): div and p = 0 as sf_project, CG on A p = div - mean(div) until the
 *       recurrence residual ||r|| <= tol * ||r0|| or max_iters iterations, then set_bnd(0, p) and the gradient
 *       subtraction of sf_project. Five distinct slots; the three work fields are the context's own.
 *   sf_set_pressure_solver(solver, tol, max_iters): what vel_step's two projections run. The default, SF_PRESSURE_JACOBI
 *       (tol and max_iters are then checked and kept but not used), is the §3 / §8 / §9 step exactly, with the same
 *       launches; sf_project is always the Jacobi operator. Per context and, like sf_set_coefficients, the same on
 *       every rank. With SF_PRESSURE_CG selected SF_W0 is scratch of the solve on return from vel_step: do not rely on it
 *       holding the pre-advect w.
 *   sf_poisson_residual(p, div, rel): sqrt(sum e.e / sum div.div), e = div - A p in the context's precision, both sums
 *       §10 sums; 0 when sum div.div == 0. No mean is removed: the honest comparison of what either solver left.
 *   sf_pressure_info_get: the last projection of either kind (sf_project, sf_project_cg, or the second one of vel_step).
 *       Jacobi: status SF_CG_MAX_ITERS, iterations = K, rel_residual = -1 (not computed). solves_total and
 *       iterations_total count every projection of the context since sf_create.
 * tol must be finite and > 0 and max_iters >= 0; anything else, an unknown solver, aliased slots or a NULL pointer is
 * SF_ERR_INVALID. Status: CONVERGED (also: zero right-hand side, 0 iterations), MAX_ITERS, or BREAKDOWN when a sum is
 * not finite or d.Ad is not > 0 (a NaN in the velocity; fp32 iterated far beyond its residual floor near 1e-4). A
 * breakdown is a status, not an error: the call returns SF_OK, the fields hold what the iterations left, and sf_sync
 * stays SF_OK. The calls are collective and synchronise on the host twice per iteration, unless sf_set_pressure_sync
 * has moved the scalars of the solve to the device (below). */
enum sf_pressure_solver { SF_PRESSURE_JACOBI = 0, SF_PRESSURE_CG = 1 };
enum sf_cg_status { SF_CG_CONVERGED = 0, SF_CG_MAX_ITERS = 1, SF_CG_BREAKDOWN = 2 };
typedef struct sf_pressure_info { int solver, status, iterations; double rel_residual;
                                  long long solves_total, iterations_total; } sf_pressure_info;
int sf_set_pressure_solver(sf_ctx* ctx, int solver, double tol, int max_iters);
int sf_project_cg(sf_ctx* ctx, int u, int v, int w, int p, int div, double tol, int max_iters);
int sf_poisson_residual(sf_ctx* ctx, int p, int div, double* rel);
int sf_pressure_info_get(const sf_ctx* ctx, sf_pressure_info* out);

/* Where the scalars of a CG solve are computed (docs/SPEC.md §11 "Where the scalars are computed").
 *   sf_set_pressure_sync(check_every): 0 (the default) — the host folds every inner product and passes alpha and beta
 *       to the next kernel by value: two host waits per iteration. m >= 1 — alpha, beta, the stop tests, status and the
 *       iteration count live in device memory; the host enqueues min(m, max_iters - n) iterations at a time and reads
 *       the state back once per batch. Iterations enqueued past the one that stops the solve change nothing, so p, u,
 *       v, w, iterations, status and rel_residual are the same bits for every check_every. Applies to sf_project_cg
 *       and to vel_step with SF_PRESSURE_CG; per context and the same on every rank (ranks that disagree issue
 *       different collectives: that hangs, it is not detected). Negative: SF_ERR_INVALID. The host first looks after a
 *       whole batch, so a solve that has nothing to do (a zero or non-finite right-hand side) or stops early still pays
 *       for the rest of its batch as empty launches and unchanged halo exchanges: m near max_iters suits solves that
 *       run to max_iters, a small m those that may stop at once.
 *   sf_pressure_sync_get: check_every, and how often the host blocked on a stream inside the last CG projection
 *       (host_waits: 2 + 2 * iterations with check_every = 0 for a solve that ends on the residual test; one per batch
 *       otherwise, a single one when check_every >= max_iters) and since sf_create (host_waits_total). */
typedef struct sf_pressure_sync { int check_every; int host_waits; long long host_waits_total; } sf_pressure_sync;
int sf_set_pressure_sync(sf_ctx* ctx, int check_every);
int sf_pressure_sync_get(const sf_ctx* ctx, sf_pressure_sync* out);

/* Preconditioner of the CG solve (docs/SPEC.md §11.2). Unpreconditioned CG needs on the order of N iterations.
 *   sf_set_pressure_preconditioner(kind, sweeps): SF_PRECOND_NONE (the default; sweeps is kept but not used) is §11
 *       exactly, with the same launches. SF_PRECOND_JACOBI with sweeps = m >= 1: z = M(r) is m undamped Jacobi sweeps
 *       on A z = r from z = 0 — §3's lin_solve(0, z, r, 1, 6, m) bit for bit, run by the kernels of sf_project — a
 *       symmetric polynomial in A that is positive on A's range. alpha = (r.z) / (d.Ad), beta = (r.z)' / (r.z),
 *       d = z + beta d; the stop test, rel_residual and sf_pressure_info stay on r.r, so tol means the same with and
 *       without a preconditioner. An even m cuts the iterations by about sqrt(2 m) (m = 4: about 2.8 x, m = 8: about
 *       4 x); an odd m is worse than the even one below it and m = 1 is a plain scaling (the iterations of NONE).
 *       m = 8 — two passes of the marching kernel on the grids it takes — is the measured optimum (docs/NEXT.md); m = 4
 *       runs as two pair passes and costs almost as much. BREAKDOWN also when r.z is not > 0. The first
 *       preconditioned solve allocates two more work fields per slab. Same bits for every decomposition, transport and
 *       check_every; per context and the same on every rank. An unknown kind, or JACOBI with sweeps < 1 (NONE with
 *       sweeps < 0): SF_ERR_INVALID, and the setting is unchanged.
 *   sf_pressure_preconditioner_get: {kind, sweeps} as last set. */
enum sf_pressure_precond { SF_PRECOND_NONE = 0, SF_PRECOND_JACOBI = 1 };
typedef struct sf_pressure_preconditioner { int kind; int sweeps; } sf_pressure_preconditioner;
int sf_set_pressure_preconditioner(sf_ctx* ctx, int kind, int sweeps);
int sf_pressure_preconditioner_get(const sf_ctx* ctx, sf_pressure_preconditioner* out);

/* Multigrid preconditioner of the CG solve (docs/SPEC.md §11.3): z = M(r) is one symmetric V-cycle of cell-centred
 * geometric multigrid on A, so the iteration count no longer grows with N (the Jacobi sweeps above cut it by sqrt(2 m)
 * only). Levels n_0 = N, n_{l+1} = n_l / 2 while n_l is even, n_l / 2 >= 4 and the depth allows; the smoother is damped
 * Jacobi (omega = 6/7), the restriction half the sum of the eight children's residuals, the prolongation the parent's
 * value; an N that does not coarsen (odd, < 8) runs coarse_sweeps sweeps on the fine grid.
 *   sf_set_pressure_multigrid(sweeps, max_levels, coarse_sweeps): sweeps = nu >= 1 puts the V-cycle in force for
 *       sf_project_cg and for vel_step with SF_PRESSURE_CG: nu sweeps before and after every coarse-grid correction,
 *       coarse_sweeps (>= 1) on the coarsest level, at most max_levels levels (0: as many as N allows). sweeps = 0 (the
 *       default) is off; max_levels and coarse_sweeps are then kept but not used, and a context that never enables it
 *       issues the launches it issued before. While the V-cycle is in force the kind and sweeps of
 *       sf_set_pressure_preconditioner are kept, reported unchanged by its getter and not used; sweeps = 0 again
 *       restores exactly the solve they describe. On a decomposed context every coarse level n_l (l >= 1) must be
 *       divisible by the number of slabs, so that no restriction crosses a slab (64 over 4 slabs: all five levels; over
 *       8: four; 40 over 2: three). Negative sweeps or max_levels, coarse_sweeps < 1 or such a decomposition:
 *       SF_ERR_INVALID, the message names the largest admissible max_levels, and the setting is unchanged. The first
 *       multigrid solve allocates the coarse levels (three fields each) and the two work fields of §11.2. Same bits for
 *       every admissible decomposition, transport and check_every; per context and the same on every rank.
 *   sf_pressure_multigrid_get: the three values as last set, and levels: the depth L of the hierarchy for this N.
 *   sf_precondition(z, r): the operator singly, z = M(r) with whatever preconditioner is in force (the V-cycle, or with
 *       SF_PRECOND_JACOBI lin_solve(0, z, r, 1, 6, m) from zero). r is read on interior cells; z is written whole,
 *       shells included. SF_ERR_INVALID if none is in force or if z == r. */
typedef struct sf_pressure_multigrid { int sweeps, max_levels, coarse_sweeps, levels; } sf_pressure_multigrid;
int sf_set_pressure_multigrid(sf_ctx* ctx, int sweeps, int max_levels, int coarse_sweeps);
int sf_pressure_multigrid_get(const sf_ctx* ctx, sf_pressure_multigrid* out);
int sf_precondition(sf_ctx* ctx, int z, int r);

/* Solid obstacles (docs/SPEC.md §15): a cell mask that the CG projection honours. An interior cell is solid iff its
 * mask value is > 0 (NaN, -0 and negatives are fluid; shell entries are ignored, shell cells are never solid). One rule
 * defines the divergence, the operator and the gradient: across a face that an interior solid cell closes, a fluid
 * cell reads itself (negated for the normal velocity) instead of the neighbour, as selects on loaded values, so nothing
 * stored in a solid cell (a NaN included) reaches a fluid cell. Solid cells end a projection with u = v = w = +0 and a
 * dens_step with dens = +0.
 *   sf_set_obstacles(mask_slot): reads the mask from field mask_slot once and turns it into per-cell face codes in a
 *       work field of the context (allocated by the first call); later writes to the slot change nothing until it is
 *       called again. From then on sf_project_cg, sf_poisson_residual and both projections of sf_vel_step are the masked
 *       forms of §15 and sf_dens_step zeroes the density of solid cells; sf_vel_step then needs SF_PRESSURE_CG
 *       (SF_ERR_INVALID otherwise), and a masked solve while the multigrid V-cycle is in force is SF_ERR_INVALID with
 *       a message unless sf_set_obstacle_multigrid(1) was called (below). sf_project and sf_precondition are never masked. mask_slot = -1 switches obstacles off and restores
 *       the launches of a context that never set any. With a mask without a solid cell every result has the bits of
 *       the unmasked call. Same bits for every decomposition, transport and check_every. Collective, the same on
 *       every rank; it synchronises (the fluid cells are counted as a §10 sum) and drops the graphs SF_GRAPH has
 *       cached. A slot outside -1 .. SF_NUM_FIELDS-1: SF_ERR_INVALID, and the setting is unchanged.
 *   sf_obstacles_get: enabled (0 / 1) and fluid_cells, the fluid interior cells of the whole grid (N^3 while off). */
typedef struct sf_obstacles { int enabled; long long fluid_cells; } sf_obstacles;
int sf_set_obstacles(sf_ctx* ctx, int mask_slot);
int sf_obstacles_get(const sf_ctx* ctx, sf_obstacles* out);

/* Obstacle-aware multigrid (docs/SPEC.md §16): the V-cycle of §11.3 with every level knowing the mask. A coarse cell
 * is solid iff all eight of its children are; smoother, residual and correction are the masked forms (a closed
 * neighbour reads as the cell itself, solid cells hold +0). A mask without a solid cell gives the bits of §11.3.
 *   sf_set_obstacle_multigrid(on): 0 (the default) keeps the refusal above, with its messages and launches; 1 makes a
 *       masked solve with the V-cycle in force run with z = V_m(0, r) where §15 says z = M(r). Valid in any order with
 *       sf_set_obstacles and sf_set_pressure_multigrid, each of which makes the next masked V-cycle build the face
 *       codes of the coarse levels afresh (one more field per coarse level, allocated by the first one). Same bits for
 *       every admissible decomposition, transport and check_every. Collective; it synchronises and drops the graphs
 *       SF_GRAPH has cached. on outside 0 / 1: SF_ERR_INVALID, and the setting is unchanged.
 *   sf_obstacle_multigrid_get: on as last set.
 *   sf_precondition_masked(z, r): the operator singly, z = V_m(0, r); r read on interior cells (what it stores in solid
 *       cells is never used), z written whole. SF_ERR_INVALID unless obstacles are on, the V-cycle is in force and the
 *       setting is on, or if z == r. sf_precondition stays unmasked. */
int sf_set_obstacle_multigrid(sf_ctx* ctx, int on);
int sf_obstacle_multigrid_get(const sf_ctx* ctx, int* on);
int sf_precondition_masked(sf_ctx* ctx, int z, int r);

/* Mask-aware transport (docs/SPEC.md §17): diffusion and advection that honour the mask of §15, so that nothing leaks
 * into a solid and has to be zeroed again. A Jacobi sweep reads a closed neighbour by set_bnd's mirror rule (the cell
 * itself, negated for the field's own velocity component: b = 0 no flux into a solid, b = 1, 2, 3 no flow through it
 * and free slip along it); advect replaces a sample that lies in a solid cell by the cell's own value (b = 0) or by 0
 * (b = 1, 2, 3). Solid cells hold +0 after either. All selects on loaded values: a NaN parked in a solid cell reaches
 * no fluid cell. A mask without a solid cell gives the bits of sf_diffuse / sf_advect. The back-trace is not stopped by
 * a solid: a path across a thin one samples the far side.
 *   sf_set_obstacle_transport(on): 0 (the default) keeps the steps of §15 with their launches; 1 makes, while obstacles
 *       are on, the three diffuse and advect of sf_vel_step and those of sf_dens_step the masked forms (sources are
 *       added first, bound ones copied into the x0 slots first: the same bits), and sf_dens_step no longer ends by
 *       zeroing the solids. A step whose fields are advected with SF_ADVECT_MACCORMACK is then SF_ERR_INVALID with a
 *       message, unless sf_set_obstacle_maccormack(1). Valid in any order with sf_set_obstacles; while the setting is on, sf_set_obstacles also zeroes the
 *       shell entries of the face codes and exchanges their ghost planes. Same bits for every decomposition and
 *       transport. Collective; it synchronises and drops the graphs SF_GRAPH has cached. on outside 0 / 1:
 *       SF_ERR_INVALID, and the setting is unchanged.
 *   sf_obstacle_transport_get: on as last set.
 *   sf_diffuse_masked(b, x, x0, diff), sf_advect_masked(b, d, d0, u, v, w): the operators singly, with the arguments,
 *       the aliasing rules and (advect) the halo condition of sf_diffuse / sf_advect. SF_ERR_INVALID unless obstacles
 *       are on and the setting is on. */
int sf_set_obstacle_transport(sf_ctx* ctx, int on);
int sf_obstacle_transport_get(const sf_ctx* ctx, int* on);
int sf_diffuse_masked(sf_ctx* ctx, int b, int x, int x0, double diff);
int sf_advect_masked(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w);

/* MacCormack under the mask (docs/SPEC.md §18): the second-order advection of §9 composed with the masked transport of
 * §17. Pass 1 is sf_advect_masked into a temporary; pass 2 is §9's limited correction with one more rule: a cell whose
 * forward or reverse trace was clamped at a wall, or sampled a solid cell at any of its sixteen sample cells, keeps the
 * first-order value. Solid cells hold +0. All selects on loaded values: a NaN parked in a solid cell reaches no fluid
 * cell. A mask without a solid cell gives the bits of sf_advect_maccormack. Neither trace is stopped by a solid.
 *   sf_set_obstacle_maccormack(on): 0 (the default) keeps the refusal of sf_set_obstacle_transport; 1 makes, while
 *       obstacles and the transport setting are on, a velocity advected with SF_ADVECT_MACCORMACK in sf_vel_step and a
 *       density so advected in sf_dens_step run this operator. Without obstacles or without the transport setting it has
 *       no effect. Valid in any order with sf_set_obstacles, sf_set_obstacle_transport and sf_set_advection. Same bits
 *       for every decomposition and transport. Collective; it synchronises and drops the graphs SF_GRAPH has cached.
 *       on outside 0 / 1: SF_ERR_INVALID, and the setting is unchanged.
 *   sf_obstacle_maccormack_get: on as last set.
 *   sf_advect_maccormack_masked(b, d, d0, u, v, w): the operator singly, with the arguments, the aliasing rules and the
 *       halo condition (both traces) of sf_advect_maccormack. SF_ERR_INVALID unless obstacles are on and
 *       sf_set_obstacle_transport(1); the setting above governs the steps only. */
int sf_set_obstacle_maccormack(sf_ctx* ctx, int on);
int sf_obstacle_maccormack_get(const sf_ctx* ctx, int* on);
int sf_advect_maccormack_masked(sf_ctx* ctx, int b, int d, int d0, int u, int v, int w);

/* Moving solids (docs/SPEC.md §19): obstacles with a velocity of their own, three fields us, vs, ws of which only the
 * values in interior solid cells are ever used (selects on loaded values: a NaN parked anywhere else reaches nothing).
 * On the axis of a velocity component the ghost value at a closed face becomes (xs[nb] + xs[nb]) - x[c], whose mean
 * with the cell is the solid's velocity, in the divergence of the projection and in the masked sweep; the tangential
 * axes stay free slip and b = 0 fields are §17's. The gradient subtraction writes us, vs, ws into solid cells instead
 * of +0, and the masked advect of b = 1, 2, 3 reads the solid's velocity at a solid SAMPLE cell instead of 0. The
 * operator A, CG, the preconditioners and §16 are unchanged. With us = vs = ws = +0 every output compares equal to
 * §15 / §17 (a -0 may come out as +0).
 *   sf_set_obstacle_velocity(su, sv, sw): the three slots are copied whole into internal fields (three more fields,
 *       allocated by the first call; ghost planes exchanged), so later writes to the slots change nothing until the
 *       next call. -1, -1, -1 switches it off and restores every launch of §15 - §18. A mix of -1 and slots, a slot
 *       out of range or two equal slots: SF_ERR_INVALID, and the setting is unchanged. Valid in any order with
 *       sf_set_obstacles and the other obstacle settings. While it is set and obstacles are on, sf_project_cg,
 *       sf_diffuse_masked, sf_advect_masked and sf_vel_step follow §19; sf_dens_step is §17's with the same launches.
 *       sf_vel_step is then SF_ERR_INVALID with a message without sf_set_obstacle_transport(1), and with a velocity
 *       advected by SF_ADVECT_MACCORMACK (whatever sf_set_obstacle_maccormack says; a MacCormack density is
 *       unaffected), and sf_advect_maccormack_masked with b = 1, 2, 3 is SF_ERR_INVALID with a message (b = 0 is
 *       §18's, unchanged): there is no MacCormack form under a solid velocity. Same bits for every decomposition and transport. Collective; it synchronises and drops the graphs
 *       SF_GRAPH has cached.
 *   sf_obstacle_velocity_get: 1 while a solid velocity is set, 0 otherwise. */
int sf_set_obstacle_velocity(sf_ctx* ctx, int su, int sv, int sw);
int sf_obstacle_velocity_get(const sf_ctx* ctx, int* on);

/* Axis-aligned volume rendering and light marching of docs/SPEC.md §12: an N x N image of the smoke from data that
 * already sits in device memory, instead of a (N+2)^3 frame over the bus. One ray per pixel runs along axis (0: i,
 * 1: j, 2: k) through the N interior cells of a line, entering at index 1 (from_high = 0) or N (from_high = 1). A cell
 * has the opacity a = clamp(sigma * h * dens, 0, 1) (NaN and negative densities are transparent) and, front to back,
 *     C = C + (Tr * a) * emit;  Tr = Tr * (1 - a)       from (C, Tr) = (0, 1); emit == -1: C = C + Tr * a.
 * The order along a ray is strictly sequential, so the bits are the same for every decomposition and transport and equal
 * the numpy reference tests/render_ref.py.
 *   sf_render: asynchronous; writes no field and changes no later step by a bit. Collective on several ranks: rays along
 *       k cross the slabs in order and each slab starts from the (C, Tr) image pair the one before it left; rays along i
 *       and j stay inside a plane. dens and emit are read on owned planes only (no halo exchange); emit == dens is allowed.
 *   sf_render_read: waits for the last sf_render, then writes the final C (colour) and Tr (transmittance) of every ray
 *       this context holds into dense N * N arrays of the context's dtype; either pointer may be NULL. The pixel of the
 *       ray at (a, b) — the two remaining axes in increasing order: (j, k), (i, k) or (i, j) — is at (a-1) + N*(b-1). A
 *       context writes the pixels it holds, as sf_download does for planes: for i and j views the pixel rows b = k of its
 *       owned planes, for a k view the whole image on the context that owns the plane the rays leave from and nothing
 *       elsewhere.
 *   sf_light: dst = the exclusive transmittance (the Tr of the ray before the cell is applied; exactly 1 on the first
 *       cell visited), then set_bnd(0, dst) and its ghost planes. Rendering with emit = dst and another axis gives
 *       self-shadowed smoke.
 * SF_ERR_INVALID: a NULL params pointer, an axis outside 0..2, from_high outside {0, 1}, a sigma that is negative or
 * not finite, a slot out of range, dst == dens, sf_render_read before any sf_render. An SF_USER slot not yet used is
 * allocated (zeros) first, as elsewhere. The image buffers are allocated by the first call. */
typedef struct sf_render_params { int axis, from_high; double sigma; int dens, emit; } sf_render_params; /* emit = -1: none */
int sf_render(sf_ctx* ctx, const sf_render_params* p);
int sf_render_read(sf_ctx* ctx, void* colour, void* transmittance);
int sf_light(sf_ctx* ctx, int dst, int dens, int axis, int from_high, double sigma);

/* Orthographic volume rendering from any direction (docs/SPEC.md §13): a width x height image of parallel rays. The
 * frame is in grid-index coordinates (the centre of cell i is at x = i), vectors ordered (x, y, z) = (i, j, k); every
 * double is converted to the context's dtype T once. Sample n (0 <= n < samples) of pixel (a, b) is at
 *     x = ((origin + T(a) * du) + T(b) * dv) + T(n) * step        per component, from n afresh,
 * and is visited iff 0.5 <= x <= N + 0.5 holds for all three components (a NaN component: not visited). The visited
 * samples of a pixel are composited front to back, in increasing n, with the recurrence of sf_render on the trilinear
 * sample of dens (and of emit) at the position and s = T(sigma) * h; a sample that is not visited leaves (C, Tr) alone,
 * so a ray that misses the box ends at exactly (+0, 1). The bits are the same for every decomposition, transport and
 * launch geometry and equal the numpy reference tests/render_view_ref.py.
 *   sf_render_view: asynchronous; writes no field and changes no later step by a bit; issues no halo exchange (ghost
 *       planes are current after every operator and upload). Collective on several ranks: each slab applies the samples
 *       whose lower plane k0 it owns and hands the (C, Tr) pair on, upwards if T(step[2]) >= 0 and downwards otherwise.
 *       The view has an image pair of its own: a view render does not touch the image of sf_render.
 *   sf_render_view_read: waits for the last sf_render_view or sf_render_camera (below; they share the image pair and the
 *       read returns the last image of either), then writes C (colour) and Tr (transmittance) into dense
 *       width * height arrays of T, pixel (a, b) at a + width * b; either pointer may be NULL. The whole image is on the
 *       context that owns the last slab visited; other contexts write nothing. A loopback context renders its own planes
 *       only.
 *   sf_view_frame: host only. The frame that looks along dir with up as the vertical, on an image plane that spans the
 *       box's bounding sphere: pixel pitch sqrt(3) N / max(width, height), samples `step` apart from the sphere's near
 *       side to its far side, sigma scaled by step (so sigma stays the extinction per cell length). dens and emit are
 *       left at -1 for the caller. All double arithmetic, bracketed as SPEC §13 writes it.
 * SF_ERR_INVALID: a NULL pointer, a double that is not finite, sigma < 0, width or height outside 1 .. 16384, samples
 * outside 1 .. 65536, a slot out of range, sf_render_view_read before any sf_render_view; in sf_view_frame also N < 1,
 * a zero dir, up parallel to dir, step not > 0, or a step that gives more than 65536 samples. An SF_USER slot not yet
 * used is allocated (zeros) first, as elsewhere. */
typedef struct sf_view_params { double origin[3], du[3], dv[3], step[3]; int width, height, samples;
                                double sigma; int dens, emit; } sf_view_params;   /* emit = -1: none */
int sf_render_view(sf_ctx* ctx, const sf_view_params* p);
int sf_render_view_read(sf_ctx* ctx, void* colour, void* transmittance);
int sf_view_frame(int N, const double dir[3], const double up[3], int width, int height, double step,
                  double sigma, sf_view_params* out);

/* Perspective volume rendering (docs/SPEC.md §14): the frame of sf_render_view plus two vectors that make the step a
 * function of the pixel, so that the rays of a pinhole camera fan out. Per component, in T,
 *     r = (view.step + T(a) * step_du) + T(b) * step_dv          the step vector of pixel (a, b)
 *     x = ((origin + T(a) * du) + T(b) * dv) + T(n) * r          sample n, from n afresh
 * with the visited predicate, the trilinear sample, the recurrence and the untouched unvisited sample of §13. view.sigma
 * is the extinction per cell length: the opacity scalar of a pixel is s = (T(sigma) * h) * sqrt((r_x r_x + r_y r_y) +
 * r_z r_z), so samples spaced differently along different rays absorb alike. With step_du = step_dv = 0 the positions
 * are sf_render_view's. The bits are the same for every decomposition, transport and launch geometry and equal the numpy
 * reference tests/render_camera_ref.py.
 *   sf_render_camera: asynchronous and collective, as sf_render_view; issues no halo exchange. A pixel is `down` iff
 *       T(r_z) < 0 and `up` otherwise. r_z is monotone along the rows and columns of the image, so the four corner pixels
 *       decide: all up or all down is one chain in that direction, as §13's; a mixed image takes an upward chain over all
 *       slabs that applies the up pixels and then a downward chain, starting from the pair the upward one left on the last
 *       slab, that applies the down pixels. It writes into the image pair of sf_render_view: sf_render_view_read returns
 *       the last image of either call, on the context that owns the last slab visited (mixed: slab 0). Nothing of it
 *       reaches the graph cache.
 *   sf_camera_passes_get: host only. The corner rule for dtype (SF_F32 / SF_F64): which chains sf_render_camera runs.
 *   sf_camera_frame: host only. A pinhole camera at eye looking at target, up as the vertical, tan_half_fov the tangent
 *       of half the vertical field of view. Sample n of every pixel lies at depth t0 + n * step along the viewing
 *       direction, from where the bounding sphere of the box begins (or the eye, inside it) to where it ends. All double
 *       arithmetic with + - * / sqrt only, bracketed as SPEC §14 writes it; sigma is passed through; dens and emit are
 *       left at -1.
 * SF_ERR_INVALID: what sf_render_view refuses; a corner pixel whose r or origin is not finite in T; a dtype that is
 * neither SF_F32 nor SF_F64; in sf_camera_frame N < 1, eye == target, up parallel to the direction, tan_half_fov or step
 * not > 0 (or not finite), a box behind the camera, more than 65536 samples. */
typedef struct sf_camera_params { sf_view_params view; double step_du[3], step_dv[3]; } sf_camera_params;
enum sf_camera_passes { SF_CAMERA_UP = 0, SF_CAMERA_DOWN = 1, SF_CAMERA_BOTH = 2 };
int sf_render_camera(sf_ctx* ctx, const sf_camera_params* p);
int sf_camera_passes_get(const sf_camera_params* p, int dtype, int* passes);
int sf_camera_frame(int N, const double eye[3], const double target[3], const double up[3], double tan_half_fov,
                    int width, int height, double step, double sigma, sf_camera_params* out);

/* Run-time parameters (the reference only has compile-time #defines, FluidGPU.cuh:1-31). */
int sf_set_iters(sf_ctx* ctx, int iters);
int sf_set_coefficients(sf_ctx* ctx, double dt, double diff, double visc);

/* Waits for all streams of the context; returns deferred errors (SF_ERR_HALO_EXCEEDED, SF_ERR_TRACER_OVERFLOW,
 * HIP faults).
 * Role of the cudaDeviceSynchronize calls of solver-unidyn.cu:369,380,403. */
int sf_sync(sf_ctx* ctx);
/* Message of the last failing call on ctx (ctx == NULL: of the last failing sf_create). */
const char* sf_last_error(const sf_ctx* ctx);

/* Device timers on the context's compute stream (the cudaEvent pair of solver.cu:175-197).
 * sf_timer_stop synchronises on the stop event and returns milliseconds between the two records. */
int sf_timer_start(sf_ctx* ctx);
int sf_timer_stop(sf_ctx* ctx, float* ms);

/* Measures a plain 16-byte-per-lane device copy of `bytes` bytes (read + write = 2*bytes of traffic)
 * on the context's device, `reps` times after one warm-up; returns the best rate in GB/s of
 * traffic. Used by bench.py to quote the achievable-HBM figure in the same run. */
int sf_measure_copy_bandwidth(sf_ctx* ctx, size_t bytes, int reps, double* gbps);

/* Number of kernel launches sf_lin_solve(..., iters) issues per field group on this context: sweeps are
 * fused in pairs where the layout allows (docs: DESIGN.md §4), so this is iters/2 (+1 if odd) or iters.
 * Lets a benchmark convert a lin_solve time into a per-launch time comparable with rocprof. */
int sf_lin_solve_launches(const sf_ctx* ctx, int iters);

/* Geometry of the internal layout, for reports: row pitch (elements), planes stored per slab,
 * bytes per field per slab. Any pointer may be NULL. */
int sf_layout_info(const sf_ctx* ctx, int* row_pitch, int* planes_per_slab, size_t* bytes_per_field);

/* Launch schedule of a decomposed lin_solve, for reports: pairs per trapezoid block (0 = boundary launch of fixed
 * size); `measured` bit 0: sf_create measured the depth on this machine (else default / SF_TRAP), bit 1: it also
 * measured "u,v,w one field at a time" against "three fields per launch", bit 2: the three-field form is in use. */
int sf_schedule_info(const sf_ctx* ctx, int* trapezoid_pairs, int* measured);

/* Which halo transport this context uses and how often it ran: *transport = 0 none (one slab), 1 device-local copy
 * kernel between logical slabs, 2 RCCL send/recv between processes, 3 RCCL send/recv to self (SF_FLAG_RCCL_SELF),
 * 4 loopback copies (SF_FLAG_LOOPBACK_HALO); *rccl_groups = ncclGroupEnd calls issued so far: halo
 * exchanges, tracer migrations and the record collectives of sf_reduce / sf_diagnostics_get (one each). */
int sf_transport_info(const sf_ctx* ctx, int* transport, long* rccl_groups);

#ifdef __cplusplus
}
#endif
#endif /* SFGPU_H */
