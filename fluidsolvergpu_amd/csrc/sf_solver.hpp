// sf_solver.hpp — host side of libsfgpu.so: contexts, slab decomposition, halo exchange, the step
// sequences of docs/SPEC.md §3 and the C ABI of include/sfgpu.h.
//
// Structure (MI355X-first, not a translation of the reference's host loop, solver.cu:171-216):
//   * one context = L logical k-slabs of one process on one GPU; P = nranks*L slabs in total.
//     Each slab has a compute stream and a halo stream. An operator is launched first on the two
//     slab-boundary planes, then on the interior planes; the halo stream ships the boundary planes
//     (device-to-device copy between slabs of the same process, RCCL send/recv grouped over xGMI
//     between processes) while the interior sweep runs. No collective reduction exists anywhere in
//     the step, only neighbour exchange; sf_reduce / sf_diagnostics_get (SPEC §10) are calls of
//     their own that the step never makes. The one exception is opt-in: with the conjugate-gradient pressure solver
//     selected (SPEC §11) the two projections of vel_step read their inner products on the host, or, with
//     sf_set_pressure_sync, fold them on the device and let the host read the solve's state once per batch.
//   * fields are named slots holding device pointers, so SPEC's "swap" is a pointer swap.
//   * there is NO CPU fallback: without a gfx950 device sf_create fails with SF_ERR_NO_DEVICE.
#pragma once
#include "sf_base.hpp"
#include "sf_kernels.hpp"

namespace sfi {

template <class T>
class Solver final : public SolverBase {
    static constexpr int W = sfk::VecT<T>::W;
    static constexpr int NSCRATCH = 3;
    // Internal slots: field[WORK_SLOT + f] aliases scratch[f] while an operator whose work field must be addressed by
    // slot is issued (exchange() and op_advect take slots). Invariant: one of these NSCRATCH slots is non-null only
    // while a ScratchAlias guard lives; guards do not nest; and nothing that swaps scratch pointers with slots (an
    // op_lin_solve without a partner of its own) runs under a guard. Every slot is a view, alias or not: own_ holds
    // what exists and frees it, the slots say where it is now, and nothing is ever freed through a slot.
    static constexpr int WORK_SLOT = SF_NUM_FIELDS;
    static constexpr int MAG_SLOT = WORK_SLOT;  // |curl u| of the forces (SPEC §8)
    static constexpr int HAT_SLOT = WORK_SLOT;  // + f: `hat`, the first-order result inside advect_mc (SPEC §9)
    static constexpr int CG_R = WORK_SLOT, CG_D = WORK_SLOT + 1, CG_Q = WORK_SLOT + 2;  // CG's r, d, q (SPEC §11)
    // z = M(r) of a preconditioned solve and the ping-pong partner of its sweeps (SPEC §11.2). No aliases: these two
    // slots have buffers of their own from the first preconditioned solve on (pcg_alloc).
    static constexpr int CG_Z = WORK_SLOT + NSCRATCH, CG_ZP = CG_Z + 1;
    // The coarse levels l >= 1 of the multigrid preconditioner (SPEC §11.3): z, its partner and the level's right-hand
    // side, three slots with buffers of their own per level from the first multigrid solve on (op_vcycle). Level 0 is
    // the z, the partner and the r of the solve itself.
    static constexpr int MG_MAXL = 12, MG_SLOT = CG_ZP + 1;
    static constexpr int mg_z(int l) { return MG_SLOT + 3 * (l - 1); }
    static constexpr int mg_zp(int l) { return mg_z(l) + 1; }
    static constexpr int mg_r(int l) { return mg_z(l) + 2; }
    // The face codes of the obstacles in force (SPEC §15): one slot with a buffer of its own from the first
    // sf_set_obstacles on, written by that call only.
    static constexpr int OBST_SLOT = MG_SLOT + 3 * (MG_MAXL - 1);
    // The face codes of the coarse levels l >= 1 under obstacles (SPEC §16): one owning slot per level, written when the
    // first masked V-cycle after sf_set_obstacles / sf_set_pressure_multigrid builds them. Level 0 is OBST_SLOT.
    static constexpr int mg_code(int l) { return OBST_SLOT + l; }
    // The solid velocity in force (SPEC §19): three owning slots (us, vs, ws) with buffers of their own from the first
    // sf_set_obstacle_velocity on, written by that call only (whole copies of the caller's slots, ghost planes current).
    static constexpr int OBSTV_SLOT = OBST_SLOT + MG_MAXL;

    // The geometry of the fields an operator runs on: the solver-wide one (lv0_, the default everywhere) or a coarse
    // level of the multigrid hierarchy, whose fields have n cells per axis, n / P planes per slab and one ghost plane.
    struct Level {
        int N = 0, nzl = 0, G = 1, np = 0, px = 0;
        long plane = 0, elems = 0, pad_front = 0, pad_back = 0;
    };

    struct Slab {
        int gid = 0;  // global slab index 0..P-1
        sfk::Geom geom{};
        T* field[SF_NUM_FIELDS + NSCRATCH + 2 + 3 * (MG_MAXL - 1) + 1 + (MG_MAXL - 1) + 3] = {};
        T* scratch[NSCRATCH] = {};
        T* snap[4] = {};               // snapshot buffers for asynchronous output
        hipStream_t os = nullptr;      // output (copy) stream
        hipEvent_t snap_done = nullptr;
        hipStream_t cs = nullptr;   // compute (interior planes, whole-field operators)
        hipStream_t bs = nullptr;   // boundary planes of a decomposed grid: runs beside the interior launch
        hipStream_t hs = nullptr;   // halo
        hipEvent_t cs_mark = nullptr;
        hipEvent_t boundary_done = nullptr;
        hipEvent_t halo_done = nullptr;
        int* d_flag = nullptr;
        // tracers of a decomposed context (SPEC §6.1): the owned list (a ping-pong pair and its two counts), the send
        // buffers towards slab gid - 1 / gid + 1 and, where that neighbour's records arrive as a message (another
        // process, loopback, SF_FLAG_RCCL_SELF), the receive buffers; tr_flag: overflow / skipped-slab bits
        sfk::TracerRec<T>* tr_list[2] = {};
        int* tr_cnt = nullptr;
        sfk::TracerRec<T>* tr_send[2] = {};
        sfk::TracerRec<T>* tr_recv[2] = {};
        int* tr_flag = nullptr;
        // reductions (SPEC §10), allocated by the first sf_reduce / sf_diagnostics_get: row records
        // [value][plane][rows_pad()] and plane records [plane][value]
        double* red_rows = nullptr;
        double* red_planes = nullptr;
        // rays (SPEC §12), allocated by the first sf_render [0] / sf_light [1]: the slab's (C, Tr) image pair, 2 N^2
        // values, and, where the pair of the slab a k-ray comes from arrives as a message, the buffer it arrives in.
        // [2]: the pair of sf_render_view (SPEC §13), 2 width height values, allocated afresh when the frame's size changes
        T* ray_img[3] = {};
        T* ray_in[3] = {};
    };

    // The first n internal slots of every slab alias its scratch buffers while this lives (invariant at WORK_SLOT). The
    // alias is taken afresh by every operator, because the solves in between swap scratch pointers with slots.
    struct ScratchAlias {
        std::vector<Slab>& slabs;
        const int n;
        ScratchAlias(std::vector<Slab>& s, int n_) : slabs(s), n(n_) {
            for (Slab& sl : slabs)
                for (int f = 0; f < n; ++f) SF_REQUIRE(!sl.field[WORK_SLOT + f], "internal: scratch alias already set");
            for (Slab& sl : slabs)
                for (int f = 0; f < n; ++f) sl.field[WORK_SLOT + f] = sl.scratch[f];
        }
        ~ScratchAlias() {
            for (Slab& sl : slabs)
                for (int f = 0; f < n; ++f) sl.field[WORK_SLOT + f] = nullptr;
        }
    };

    // One launch of an operator as for_planes issues it: planes [kb, ke) of slab sl on stream st (sl.cs or sl.bs).
    // The boundary launch of a decomposed grid covers the first and the last `split` interior planes in one grid:
    // its logical plane t sits at kb + t + (t >= split ? gap : 0) (sfk::TileMap). Other launches: split = INT_MAX,
    // gap = 0.
    struct Launch {
        Slab& sl;
        hipStream_t st;
        int kb, ke;
        int split = INT_MAX, gap = 0;
        bool is_split() const { return split != INT_MAX; }
    };

    // The SF_* environment switches, each read once, here, when the context is created (defaults = production).
    // SF_TRAP is read by the constructor (its default depends on the transport); SF_TRACE_SCHEDULE by trace_open().
    struct Switches {
        int nt = env_int("SF_NT", 2);           // non-temporal stores: 0 never, 1 always, 2 beyond the Infinity Cache
        int ishell = env_int("SF_ISHELL", 1);   // 0 every sweep reads and writes the i-shell, 1 implicit between
                                                // passes and left unwritten where nothing reads it, 2 implicit only
        bool fuse2 = env_int("SF_FUSE2", 1) != 0;  // 0 single sweeps, 1 fused sweeps
        int ghost = env_int("SF_GHOST", 4);     // most ghost planes per side of a slab
        int advect_row = env_int("SF_ADVECT_ROW", 1);  // 0 gather form always, 1 one cell per lane for the three
                                                       // velocity components, 2 / 3 always
        bool zero_skip = env_int("SF_ZERO_SKIP", 1) != 0;  // project's first pair loads no (zero) pressure
        bool split = env_int("SF_SPLIT", 1) != 0;  // boundary / interior launches of a slab on two streams
        int ovl = env_int("SF_OVL", 1);         // overlapped row mapping of the pair kernel (launch_fused2)
        int split_fields = env_int("SF_SPLIT_FIELDS", 1);  // 0 never, 1 when one field fits the Infinity Cache, 2 always
        bool fuse_src = env_int("SF_FUSE_SRC", 1) != 0;  // fold add_source (bound sources) into diffuse's first pass
        bool graph = env_int("SF_GRAPH", 0) != 0;
        int halo_stream = env_int("SF_HALO_STREAM", 0);
        bool autotune = env_int("SF_AUTOTUNE", 1) != 0;
        int march = env_int("SF_MARCH", 1);     // 0: the register-blocked pair kernel everywhere
        int march_minp = env_int("SF_MARCH_MINP", 12);
        // Smallest launch the marching kernel takes: 2.5 M cells (~136^3; 6 M until round 3) — with 16 thin waves per
        // workgroup it overtakes the pair kernel there (us per sweep of a 20-sweep solve, pair / marching: 128^3 4.4 /
        // 5.8, 144^3 9.0 / 6.0, 160^3 10.6 / 6.3, 176^3 13.4 / 7.1), slab interiors included (one rank's share of the
        // full step: 256^3 over 4 ranks 1.335 -> 1.147 ms, 384^3 over 8 ranks 1.806 -> 1.492).
        long march_min_cells = (long)env_int("SF_MARCH_MINCELLS_K", 2500) * 1000L;
        int sk_s = env_int("SF_SK_S", 4);       // most sweeps per marching pass
        bool sk_first = env_int("SF_SK_FIRST", 1) != 0;  // first pass of a solve through the marching kernel
    };

public:
    explicit Solver(const sf_params& p) : N_(p.N), K_(p.iters), device_(p.device), own_(p.device) {
        SF_REQUIRE(p.N >= 1, "N must be >= 1");
        SF_REQUIRE(p.iters >= 0, "iters must be >= 0");
        L_ = p.nslabs_local > 0 ? p.nslabs_local : 1;
        nranks_ = p.nranks > 0 ? p.nranks : 1;
        rank_ = p.rank;
        SF_REQUIRE(rank_ >= 0 && rank_ < nranks_, "rank out of range");
        P_ = nranks_ * L_;
        SF_REQUIRE(N_ % P_ == 0, "N must be divisible by nranks*nslabs_local");
        loopback_ = (p.flags & SF_FLAG_LOOPBACK_HALO) != 0;
        rccl_self_ = (p.flags & SF_FLAG_RCCL_SELF) != 0;
        SF_REQUIRE(!rccl_self_ || (nranks_ == 1 && L_ >= 2 && !loopback_),
                   "SF_FLAG_RCCL_SELF needs nranks == 1, nslabs_local >= 2 and no loopback flag");
        SF_REQUIRE(nranks_ == 1 || loopback_ || p.nccl_id != nullptr, "nccl_id required when nranks > 1");
        set_coefficients(p.dt, p.diff, p.visc);

        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw Failure{SF_ERR_NO_DEVICE, "no HIP device visible: libsfgpu has no CPU fallback"};
        SF_REQUIRE(device_ >= 0 && device_ < ndev, "device ordinal out of range");
        SF_HIP(hipSetDevice(device_));
        hipDeviceProp_t prop;
        SF_HIP(hipGetDeviceProperties(&prop, device_));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            throw Failure{SF_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName +
                                                ", this library is built for gfx950 only"};
        num_cu_ = prop.multiProcessorCount;

        // layout
        nzl_ = N_ / P_;
        lead_ = 128 / (int)sizeof(T);
        const int line = 128 / (int)sizeof(T);
        px_ = ceil_div(lead_ + N_ + 1 + W, line) * line;
        plane_ = (long)px_ * (N_ + 2);
        // two ghost planes per side let sweep pairs be fused across slab boundaries (one exchange per pair); grids
        // the fused kernel does not take (rows wider than 512 vectors, N not a multiple of W) keep one ghost plane
        // and exchange one plane per sweep
        const bool fusable = sw_.fuse2 && N_ % W == 0 && N_ / W <= fuse_maxvec_;
        G_ = (P_ > 1 && nzl_ >= 2 && fusable && sw_.ghost >= 2) ? 2 : 1;
        // three / four ghost planes where the marching kernel will run three / four sweeps per pass on the slab
        // interiors (one exchange per pass): the interior launch [2G, nzl) must be long and large enough for it.
        // (SF_ISHELL=0 — every sweep reads and writes the i-shell in memory — rules the marching kernel out in
        // march_takes(), hence march_fits() here: the deeper ghost zone is kept all the same and the solve then runs
        // pair launches of boundary depth pair_depth() on it, the schedule that K < 7 and remainders take by default)
        for (int gs = 3; gs <= 4; ++gs)  // S = gs sweeps per exchange need gs ghost planes
            if (G_ == gs - 1 && sw_.ghost >= gs && sw_.sk_s >= gs && sw_.split && march_fits(nzl_ - 2 * gs)) G_ = gs;
        nplanes_ = nzl_ + 2 * G_;
        field_elems_ = plane_ * nplanes_ + 256;  // slack so whole-vector accesses never leave the buffer
        field_elems_ = (field_elems_ + W - 1) / W * W;
        // Rows of padding before and after every field: the marching kernel addresses the rows of a workgroup's tile
        // without clamping them into the plane (sfk::jsk_step), so the tile of the first j-block reaches up to three
        // rows below the first plane and the tile of the last one up to NW x TJ rows beyond the last plane. Never
        // stored to, and what is loaded there only feeds rows that are not stored.
        pad_front_ = (sfk::SK_PAD_ROWS_FRONT * (long)px_ + 63) / 64 * 64;
        pad_back_ = sfk::SK_PAD_ROWS_BACK * (long)px_;
        lv0_.N = N_, lv0_.nzl = nzl_, lv0_.G = G_, lv0_.np = nplanes_, lv0_.px = px_;
        lv0_.plane = plane_, lv0_.elems = field_elems_, lv0_.pad_front = pad_front_, lv0_.pad_back = pad_back_;

        slabs_.resize(L_);
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            sl.gid = rank_ * L_ + s;
            sl.geom.N = N_;
            sl.geom.nzl = nzl_;
            sl.geom.G = G_;
            sl.geom.np = nplanes_;
            sl.geom.kg0 = sl.gid * nzl_ + 1 - G_;  // first interior k = gid*nzl + 1 is local plane G
            sl.geom.px = px_;
            sl.geom.lead = lead_;
            sl.geom.plane = plane_;
            sl.geom.wall_lo = (sl.gid == 0);
            sl.geom.wall_hi = (sl.gid == P_ - 1);
            sl.cs = own_.stream(hipStreamNonBlocking);
            sl.bs = own_.stream(hipStreamNonBlocking);
            // Events that only order kernels of THIS device against each other skip the system-scope fence of the
            // default event (a cache write-back + invalidate per record: ~12 us between consecutive sweeps of a
            // decomposed grid). halo_done keeps it when the ghost planes are written by another GPU through RCCL.
            const unsigned ev_local = hipEventDisableTiming | (unsigned)hipEventDisableSystemFence;
            const unsigned ev_halo = ((nranks_ > 1 && !loopback_) || rccl_self_) ? (unsigned)hipEventDisableTiming : ev_local;
            sl.cs_mark = own_.event(ev_local);
            {
                // One slab per process (production): every halo is an RCCL message, and the chain
                // boundary launch -> message -> next boundary launch is what limits a pair once the messages take as
                // long as the interior work. Issued on ONE stream that chain needs no cross-stream hand-over (each
                // costs ~10 us, tools/evgap.hip): the halo "stream" is then the boundary stream itself
                // (SF_HALO_STREAM=1 keeps a separate one). With several slabs per process the copies pull from the
                // neighbours' buffers and stay on their own stream (SF_HALO_STREAM=2 shares there too: used by the
                // parity tests to run the shared-stream ordering against the oracle). (A high-priority halo stream
                // was measured in round 1: with logical slabs on one GPU the copy kernel pre-empts the sweeps, 2x slower.)
                const int hmode = sw_.halo_stream;  // 0 as described, 1 always separate, 2 always shared
                const bool shared = (L_ == 1 && nranks_ > 1 && hmode == 0) || hmode == 2;
                sl.hs = shared ? sl.bs : own_.stream(hipStreamNonBlocking);
            }
            sl.boundary_done = own_.event(ev_local);
            sl.halo_done = own_.event(ev_halo);
            for (int f = 0; f < SF_USER0; ++f) sl.field[f] = alloc_field();
            for (int f = 0; f < NSCRATCH; ++f) sl.scratch[f] = alloc_field();
            sl.d_flag = own_.dev<int>(sizeof(int));
            SF_HIP(hipMemset(sl.d_flag, 0, sizeof(int)));
            SF_HIP(hipDeviceSynchronize());
        }
        t0_ = own_.event(hipEventDefault);  // the default flags: these two are timed
        t1_ = own_.event(hipEventDefault);
        if (nranks_ > 1 && !loopback_) {
            ncclUniqueId id;
            static_assert(sizeof(ncclUniqueId) <= SF_NCCL_ID_BYTES, "ncclUniqueId larger than ABI slot");
            std::memcpy(&id, p.nccl_id, sizeof id);
            SF_NCCL(ncclCommInitRank(&comm_.h, nranks_, id, rank_));
        } else if (rccl_self_) {
            // a real communicator of one rank: the logical slabs' ghost planes travel as grouped ncclSend / ncclRecv
            // to self (see exchange()), so the RCCL data plane runs on a one-GPU box
            ncclUniqueId id;
            SF_NCCL(ncclGetUniqueId(&id));
            SF_NCCL(ncclCommInitRank(&comm_.h, 1, id, 0));
        }
        ishell_skip_ = sw_.ishell != 0;
        dead_ishell_opt_ = sw_.ishell == 1;
        split_fields_ = sw_.split_fields;
        // Trapezoid blocks shorten the interior chain (no cross-stream wait) but lengthen the boundary chain
        // B(j) -> halo(j) -> B(j+1), because B grows by two planes per side and pair. With halos that are copies on
        // this GPU the interior chain is the critical one (default 5 pairs per block); with RCCL messages over xGMI
        // (2.4 MB per direction and pair at 512^2: tens of microseconds) the boundary chain is, so the default there
        // keeps B at its minimum size (0 = off) unless the measurement at the end of this constructor
        // (tune_schedule) says otherwise. SF_TRAP overrides and switches the measurement off.
        trap_m_ = env_int("SF_TRAP", (nranks_ > 1 || rccl_self_) ? 0 : 5);  // pairs per trapezoid block of a decomposed lin_solve (<= 1: off)
        graphs_ = sw_.graph && P_ == 1;
        sk2_min_cells_ = std::max(sw_.march_min_cells == 0 ? 0L : 60000000L, sw_.march_min_cells);  // ~390^3
        SF_HIP(hipDeviceSynchronize());
        if ((nranks_ > 1 || rccl_self_) && std::getenv("SF_TRAP") == nullptr && sw_.autotune) tune_schedule();
        trace_open();
    }

    // Which trapezoid depth suits THIS machine's halo latency (see the comment at trap_m_)? Times a 20-sweep
    // lin_solve on the (still zero) density slots for 0, 2 and 5 pairs per block and keeps the fastest, preferring
    // the shallower one unless the deeper is 3 % faster. Every rank runs the same sequence of exchanges whatever it
    // picks (the depth only moves planes between this rank's own two launches).
    void tune_schedule() {
        if (!(G_ >= 2 && can_fuse2()) || nzl_ <= 2 * (G_ + 2) + 2) return;
        const int x[1] = {SF_DENS}, x0[1] = {SF_DENS0}, b0[1] = {0};
        const T a = T(0.25), c = T(1) + T(6) * a;
        auto drain = [&] {
            join();
            for (Slab& sl : slabs_) {
                SF_HIP(hipStreamSynchronize(sl.cs));
                SF_HIP(hipStreamSynchronize(sl.bs));
                SF_HIP(hipStreamSynchronize(sl.hs));
            }
        };
        // The ranks measure TOGETHER: a one-word all-reduce lines them up before the clock starts (a rank that starts
        // its solves early would time its neighbours' set-up), and the time that counts is the slowest rank's — the
        // step runs at that pace — so every rank sees the same numbers and takes the same decision. (Round 2 timed each
        // rank by itself.) d_sync[0]: barrier word, d_sync[1]: the time in microseconds.
        long long* d_sync = nullptr;
        if (comm_) {
            d_sync = own_.dev<long long>(2 * sizeof(long long));
            SF_HIP(hipMemset(d_sync, 0, 2 * sizeof(long long)));
            SF_HIP(hipDeviceSynchronize());
        }
        auto line_up = [&] {
            if (!comm_) return;
            SF_NCCL(ncclAllReduce(d_sync, d_sync, 1, ncclInt64, ncclSum, comm_, slabs_[0].cs));
            SF_HIP(hipStreamSynchronize(slabs_[0].cs));
        };
        auto slowest = [&](double t) -> double {
            if (!comm_) return t;
            long long us = (long long)(t * 1e6);
            SF_HIP(hipMemcpy(d_sync + 1, &us, sizeof us, hipMemcpyHostToDevice));
            SF_NCCL(ncclAllReduce(d_sync + 1, d_sync + 1, 1, ncclInt64, ncclMax, comm_, slabs_[0].cs));
            SF_HIP(hipStreamSynchronize(slabs_[0].cs));
            SF_HIP(hipMemcpy(&us, d_sync + 1, sizeof us, hipMemcpyDeviceToHost));
            return (double)us * 1e-6;
        };
        const int cand[3] = {0, 2, 5};
        double best = 0;
        int best_m = 0;
        for (int q = 0; q < 3; ++q) {
            trap_m_ = cand[q];
            op_lin_solve<1>(x, x0, b0, a, c, 10, false);  // warm-up (first use of the communicator, caches)
            drain();
            line_up();
            const auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < 3; ++r) op_lin_solve<1>(x, x0, b0, a, c, 20, false);
            drain();
            const double t = slowest(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            if (q == 0 || t < 0.97 * best) {
                best = t;
                best_m = cand[q];
            }
        }
        trap_m_ = best_m;
        tuned_trap_ = best_m;
        // Same question for "u, v, w one field at a time" (Infinity-Cache resident, three small messages per pair)
        // against "three fields per launch" (one message of three times the size: the message latency is paid once):
        // the first wins when a pair is compute-bound, the second when the messages are the critical chain.
        if (std::getenv("SF_SPLIT_FIELDS") == nullptr && fits_ic(solve_bytes())) {
            const int vel[3] = {SF_U, SF_V, SF_W}, vel0[3] = {SF_U0, SF_V0, SF_W0}, b123[3] = {1, 2, 3};
            double t_split = 0;
            for (int q = 0; q < 2; ++q) {
                split_fields_ = q == 0 ? 1 : 0;
                op_lin_solve<3>(vel, vel0, b123, a, c, 4, false);
                drain();
                line_up();
                const auto t0 = std::chrono::steady_clock::now();
                for (int r = 0; r < 2; ++r) op_lin_solve<3>(vel, vel0, b123, a, c, 20, false);
                drain();
                const double t = slowest(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
                if (q == 0)
                    t_split = t;
                else if (!(t < 0.97 * t_split))
                    split_fields_ = 1;
            }
            // unlike the trapezoid depth this changes the sequence of exchanges, so the ranks must agree: they now compare
            // the same (slowest-rank) times, and the vote below stays as the guard that they really did
            if (comm_) {
                int vote = split_fields_ == 0 ? 1 : 0, sum = 0;
                int* d_vote = own_.dev<int>(sizeof(int));
                SF_HIP(hipMemcpy(d_vote, &vote, sizeof(int), hipMemcpyHostToDevice));
                SF_NCCL(ncclAllReduce(d_vote, d_vote, 1, ncclInt, ncclSum, comm_, slabs_[0].cs));
                SF_HIP(hipStreamSynchronize(slabs_[0].cs));
                SF_HIP(hipMemcpy(&sum, d_vote, sizeof(int), hipMemcpyDeviceToHost));
                own_.release(d_vote);
                split_fields_ = (sum == nranks_) ? 0 : 1;
            }
            tuned_split_ = split_fields_;
        }
        own_.release(d_sync);
    }

    // The graph executables and the trace file only: comm_ and own_ release the rest, in that order, as members.
    ~Solver() override {
        (void)hipSetDevice(device_);
        (void)hipDeviceSynchronize();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);
        if (trace_) std::fclose(trace_);
    }

    // ---- host <-> device ------------------------------------------------------------------
    void upload(int field, const void* host) override {
        join();
        check_field(field);
        SF_REQUIRE(host != nullptr, "null host pointer");
        (void)upload_range(field, 0, N_ + 2, static_cast<const T*>(host));  // the global array: every stored plane
    }

    void download(int field, void* host) override {
        join();
        check_field(field);
        SF_REQUIRE(host != nullptr, "null host pointer");
        (void)download_range(field, 0, N_ + 2, static_cast<T*>(host));  // the global array: every owned plane
    }

    void download_planes(int field, int kb, int ke, void* host) override {
        join();
        check_field(field);
        SF_REQUIRE(host != nullptr, "null host pointer");
        SF_REQUIRE(kb < ke, "empty plane range");
        SF_REQUIRE(download_range(field, kb, ke, static_cast<T*>(host)), "plane range not stored by this context");
    }

    void upload_planes(int field, int kb, int ke, const void* host) override {
        join();
        check_field(field);
        SF_REQUIRE(host != nullptr, "null host pointer");
        SF_REQUIRE(kb < ke, "empty plane range");
        SF_REQUIRE(upload_range(field, kb, ke, static_cast<const T*>(host)), "plane range not stored by this context");
    }

    void stored_planes(int* kb, int* ke) const override {
        if (kb) *kb = std::max(slabs_.front().geom.kg0, 0);
        if (ke) *ke = std::min(slabs_.back().geom.kg0 + nplanes_, N_ + 2);
    }

    void owned_planes(int* kb, int* ke) const override {
        if (kb) *kb = slabs_.front().geom.kg0 + G_;
        if (ke) *ke = slabs_.back().geom.kg0 + G_ + nzl_;
    }

    void fill(int field, double value) override {
        join();
        check_field(field);
        SF_HIP(hipSetDevice(device_));
        for (Slab& sl : slabs_) {
            T* dev = ensure(sl, field);
            const long nvec = field_elems_ / W;
            hipLaunchKernelGGL((sfk::fill_kernel<T>), dim3(stream_grid(nvec)), dim3(256), 0, sl.cs, dev,
                               (T)value, nvec);
        }
        SF_HIP(hipGetLastError());
    }

    void copy_field(int dst, int src) override {
        join();
        check_field(dst);
        check_field(src);
        SF_REQUIRE(dst != src, "copy_field: dst == src");
        SF_HIP(hipSetDevice(device_));
        for (Slab& sl : slabs_) {
            T* d = ensure(sl, dst);
            T* s = ensure(sl, src);
            SF_HIP(hipMemcpyAsync(d, s, (size_t)field_elems_ * sizeof(T), hipMemcpyDeviceToDevice, sl.cs));
        }
    }

    // ---- operators ------------------------------------------------------------------------
    void add_source(int x, int s) override {
        check_field(x);
        check_field(s);
        SF_HIP(hipSetDevice(device_));
        const int xs[1] = {x}, ss[1] = {s};
        op_add_source<1>(xs, ss);
    }

    void set_bnd(int b, int x) override {
        check_field(x);
        check_b(b);
        SF_HIP(hipSetDevice(device_));
        op_set_bnd(b, x, nullptr);
    }

    void lin_solve(int b, int x, int x0, double a, double c, int iters) override {
        check_field(x);
        check_field(x0);
        check_b(b);
        SF_REQUIRE(x != x0, "lin_solve: x and x0 must be different fields");
        SF_REQUIRE(iters >= 0, "iters must be >= 0");
        SF_HIP(hipSetDevice(device_));
        const int xs[1] = {x}, x0s[1] = {x0}, bs[1] = {b};
        op_lin_solve<1>(xs, x0s, bs, (T)a, (T)c, iters, false);
    }

    void diffuse(int b, int x, int x0, double diff) override {
        check_field(x);
        check_field(x0);
        check_b(b);
        SF_REQUIRE(x != x0, "diffuse: x and x0 must be different fields");
        SF_HIP(hipSetDevice(device_));
        const int xs[1] = {x}, x0s[1] = {x0}, bs[1] = {b};
        const T a = diffusion_a((T)diff);
        op_lin_solve<1>(xs, x0s, bs, a, T(1) + T(6) * a, K_, false);
    }

    void advect(int b, int d, int d0, int u, int v, int w) override {
        check_field(d);
        check_field(d0);
        check_field(u);
        check_field(v);
        check_field(w);
        check_b(b);
        SF_REQUIRE(d != d0 && d != u && d != v && d != w, "advect: output must not alias an input");
        SF_HIP(hipSetDevice(device_));
        const int ds[1] = {d}, d0s[1] = {d0}, bs[1] = {b};
        op_advect<1>(ds, d0s, bs, u, v, w, false);
    }

    // SPEC §9 advect_mc
    void advect_maccormack(int b, int d, int d0, int u, int v, int w) override {
        for (int f : {d, d0, u, v, w}) check_field(f);
        check_b(b);
        SF_REQUIRE(d != d0 && d != u && d != v && d != w, "advect_maccormack: output must not alias an input");
        SF_HIP(hipSetDevice(device_));
        const int ds[1] = {d}, d0s[1] = {d0}, bs[1] = {b};
        op_advect_mc<1>(ds, d0s, bs, u, v, w, false);
    }

    void set_advection(int velocity_scheme, int density_scheme) override {
        for (int s : {velocity_scheme, density_scheme})
            SF_REQUIRE(s == SF_ADVECT_SEMI_LAGRANGIAN || s == SF_ADVECT_MACCORMACK, "advection scheme must be 0 or 1");
        mc_vel_ = velocity_scheme;
        mc_dens_ = density_scheme;
    }

    void project(int u, int v, int w, int p, int div) override {
        check_distinct("project: fields must be distinct", {u, v, w, p, div});
        SF_HIP(hipSetDevice(device_));
        op_project(u, v, w, p, div);
    }

    // SPEC §8 vorticity into dst (set_bnd(0) and ghost planes included)
    void vorticity_magnitude(int u, int v, int w, int dst) override {
        for (int f : {u, v, w, dst}) check_field(f);
        SF_REQUIRE(dst != u && dst != v && dst != w, "vorticity_magnitude: dst must not be u, v or w");
        SF_HIP(hipSetDevice(device_));
        op_vorticity(u, v, w, dst);
    }

    // SPEC §8 add_forces, the sources updated in place
    void add_forces(int u, int v, int w, int dens, int su, int sv, int sw) override {
        check_distinct("add_forces: slots must be distinct", {u, v, w, dens, su, sv, sw});
        SF_HIP(hipSetDevice(device_));
        const int s[3] = {su, sv, sw};
        op_add_forces(u, v, w, dens, s, s);
    }

    void set_vorticity_confinement(double eps) override {
        SF_REQUIRE(std::isfinite(eps) && eps >= 0.0, "vorticity confinement: eps must be finite and >= 0");
        eps_ = (T)eps;
    }
    void set_buoyancy(double beta, double ambient, int axis) override {
        SF_REQUIRE(std::isfinite(beta) && std::isfinite(ambient), "buoyancy: beta and ambient must be finite");
        SF_REQUIRE(axis >= 0 && axis <= 2, "buoyancy: axis must be 0, 1 or 2");
        beta_ = (T)beta;
        amb_ = (T)ambient;
        axis_ = axis;
    }

    void bind_sources(int su, int sv, int sw, int sd) override {
        const int b[4] = {su, sv, sw, sd};
        for (int q = 0; q < 4; ++q) {
            SF_REQUIRE(b[q] >= -1 && b[q] < SF_NUM_FIELDS, "bind_sources: slot out of range");
            SF_REQUIRE(b[q] < 0 || b[q] >= SF_USER0, "bind_sources: sources must live in SF_USER0..3");
        }
        for (int q = 0; q < 4; ++q) bound_[q] = b[q];
    }

    // SF_GRAPH=1 (opt-in): the ~55 launches of a step are captured once into a hipGraph per distinct buffer arrangement
    // and replayed, so the host issues one graph launch instead of one launch per kernel. Single-slab contexts only.
    // Off by default: measured on MI355X it changes nothing (32^3: 0.31 ms/step, 64^3: 0.35, 128^3: 0.63 either
    // way) — small grids are bound by the ~5 us dependent-kernel boundary on the device, not by host launches.
    struct GraphEntry {
        int op;
        std::vector<T*> before, after;
        int K;
        T dt, diff, visc;
        T eps, beta, amb;  // forces (SPEC §8): their scalars are baked into the captured launches
        int axis;
        int mc_vel, mc_dens;  // advection schemes (SPEC §9): they decide which launches are captured
        int bound[4];
        hipGraphExec_t exec;
        // what the captured body noted of its projections (note_solve is host code: a replay has to say it again)
        sf_pressure_info info;
        long long solves, iterations;
    };
    std::vector<T*> pointer_state() const {
        std::vector<T*> st;
        const Slab& sl = slabs_[0];
        for (T* f : sl.field) st.push_back(f);
        for (T* f : sl.scratch) st.push_back(f);
        return st;
    }
    static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }
    void apply_state(const std::vector<T*>& st) {
        Slab& sl = slabs_[0];
        size_t q = 0;
        for (T*& f : sl.field) f = st[q++];
        for (T*& f : sl.scratch) f = st[q++];
    }
    template <class Body>
    void run_maybe_graphed(int op, Body body) {
        if (!graphs_ || P_ != 1) {
            body();
            return;
        }
        Slab& sl = slabs_[0];
        for (int q = 0; q < 4; ++q)
            if (bound_[q] >= 0) ensure(sl, bound_[q]);  // no allocation may happen inside a capture
        const std::vector<T*> before = pointer_state();
        for (GraphEntry& e : graph_cache_)
            if (e.op == op && e.K == K_ && e.dt == dt_ && e.diff == diff_ && e.visc == visc_ && same_bits(e.eps, eps_) &&
                same_bits(e.beta, beta_) && same_bits(e.amb, amb_) && e.axis == axis_ &&
                e.mc_vel == mc_vel_ && e.mc_dens == mc_dens_ &&
                std::equal(e.bound, e.bound + 4, bound_) && e.before == before) {
                SF_HIP(hipGraphLaunch(e.exec, sl.cs));
                apply_state(e.after);
                if (e.solves > 0) {  // sf_pressure_info: the step's last projection, and every projection counted
                    const long long solves = info_.solves_total + e.solves, iters = info_.iterations_total + e.iterations;
                    info_ = e.info;
                    info_.solves_total = solves;
                    info_.iterations_total = iters;
                }
                return;
            }
        hipGraph_t graph = nullptr;
        const sf_pressure_info info_before = info_;
        SF_HIP(hipStreamBeginCapture(sl.cs, hipStreamCaptureModeThreadLocal));
        try {
            body();
        } catch (...) {
            (void)hipStreamEndCapture(sl.cs, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            apply_state(before);
            info_ = info_before;
            throw;
        }
        SF_HIP(hipStreamEndCapture(sl.cs, &graph));
        GraphEntry e;
        e.op = op;
        e.before = before;
        e.after = pointer_state();
        e.K = K_;
        e.dt = dt_;
        e.diff = diff_;
        e.visc = visc_;
        e.eps = eps_;
        e.beta = beta_;
        e.amb = amb_;
        e.axis = axis_;
        e.mc_vel = mc_vel_;
        e.mc_dens = mc_dens_;
        std::copy(bound_, bound_ + 4, e.bound);
        e.info = info_;
        e.solves = info_.solves_total - info_before.solves_total;
        e.iterations = info_.iterations_total - info_before.iterations_total;
        SF_HIP(hipGraphInstantiate(&e.exec, graph, nullptr, nullptr, 0));
        SF_HIP(hipGraphDestroy(graph));
        graph_cache_.push_back(e);
        SF_HIP(hipGraphLaunch(e.exec, sl.cs));
    }

    void vel_step() override {
        SF_HIP(hipSetDevice(device_));
        if (pressure_ == SF_PRESSURE_CG)  // the CG solve reads its sums on the host: nothing to capture
            vel_step_body();
        else
            run_maybe_graphed(0, [&] { vel_step_body(); });
    }
    void dens_step() override {
        SF_HIP(hipSetDevice(device_));
        run_maybe_graphed(1, [&] { dens_step_body(); });
    }

    // SPEC §3 vel_step.
    void vel_step_body() {
        const int vel[3] = {SF_U, SF_V, SF_W}, vel0[3] = {SF_U0, SF_V0, SF_W0}, b123[3] = {1, 2, 3};
        const T a = diffusion_a(visc_);
        // Nobody reads the i-shell of the diffused velocity: project_div reads v and w at interior i only and mirrors u's
        // (b = 1), project_sub then rewrites all three shells from the corrected interior. Likewise the pressure of this
        // FIRST projection: its slot is overwritten by advect before anything else looks at it. Their solves therefore
        // leave the i-shell unwritten (no partial writes to HBM: a 512^3 last pass takes 441 instead of 520 us). K_ = 0
        // runs no sweep: the fields keep their caller-written shells and are read from memory as before.
        // (obstacles, SPEC §15: the masked project halves read every shell as stored, so nothing is left unwritten)
        SF_REQUIRE(!obst_on_ || pressure_ == SF_PRESSURE_CG,
                   "vel_step: obstacles need the CG pressure solver (SF_PRESSURE_CG)");
        SF_REQUIRE(!(obst_on_ && mg_nu_ > 0) || obst_mg_,
                   "vel_step: obstacles with the multigrid preconditioner in force are not supported");
        const bool dead = ishell_skip_ && K_ >= 1 && dead_ishell_opt_ && !obst_on_;
        // SPEC §17: diffuse and advect under the mask (sources added first; bound ones copied first: the same bits)
        const bool masked_tr = obst_on_ && obst_tr_;
        // SPEC §19: a solid velocity needs the masked transport and has no MacCormack form
        SF_REQUIRE(!obstv_on_ || obst_tr_,
                   "vel_step: a solid velocity (sf_set_obstacle_velocity) needs sf_set_obstacle_transport(1)");
        SF_REQUIRE(!(obstv_on_ && mc_vel_ == SF_ADVECT_MACCORMACK),
                   "vel_step: MacCormack advection of the velocity under a solid velocity (sf_set_obstacle_velocity) "
                   "is not supported");
        SF_REQUIRE(!(masked_tr && mc_vel_ == SF_ADVECT_MACCORMACK) || obst_mc_,
                   "vel_step: MacCormack advection of the velocity under sf_set_obstacle_transport(1) is not supported");
        // SPEC §8: with a force on, the sources (bound slots, or the x0 slots themselves) plus the forces go into the
        // x0 slots first, and the step continues as with unbound sources
        const bool forces = eps_ != T(0) || beta_ != T(0);
        if (forces) {
            int src[3];
            for (int q = 0; q < 3; ++q) src[q] = bound_[q] >= 0 ? bound_[q] : vel0[q];
            op_add_forces(SF_U, SF_V, SF_W, SF_DENS, src, vel0);
        }
        if (!masked_tr && !forces && bound_[0] >= 0 && bound_[1] >= 0 && bound_[2] >= 0) {
            const int src[3] = {bound_[0], bound_[1], bound_[2]};
            op_diffuse_src<3>(vel, vel0, b123, src, a, T(1) + T(6) * a, K_, dead);
        } else {
            for (int q = 0; q < 3; ++q)
                if (!forces && bound_[q] >= 0) copy_field(vel0[q], bound_[q]);
            op_add_source<3>(vel, vel0);
            swap_slots(SF_U0, SF_U);
            swap_slots(SF_V0, SF_V);
            swap_slots(SF_W0, SF_W);
            if (masked_tr)
                op_lin_solve_masked<3>(vel, vel0, b123, a, T(1) + T(6) * a, K_);
            else
                op_lin_solve<3>(vel, vel0, b123, a, T(1) + T(6) * a, K_, dead);
        }
        const bool cg = pressure_ == SF_PRESSURE_CG;
        if (cg)
            op_project_cg(SF_U, SF_V, SF_W, SF_U0, SF_V0, cg_tol_, cg_max_iters_, dead);
        else
            op_project(SF_U, SF_V, SF_W, SF_U0, SF_V0, dead, dead);
        swap_slots(SF_U0, SF_U);
        swap_slots(SF_V0, SF_V);
        swap_slots(SF_W0, SF_W);
        // the advected velocity goes straight into the second projection: same argument as for the diffused one
        if (masked_tr && mc_vel_ == SF_ADVECT_MACCORMACK)  // SPEC §18 (obst_mc_: required above)
            op_advect_mc_masked<3>(vel, vel0, b123, SF_U0, SF_V0, SF_W0);
        else if (masked_tr)
            op_advect_masked<3>(vel, vel0, b123, SF_U0, SF_V0, SF_W0);
        else if (mc_vel_ == SF_ADVECT_MACCORMACK)
            op_advect_mc<3>(vel, vel0, b123, SF_U0, SF_V0, SF_W0, dead);
        else
            op_advect<3>(vel, vel0, b123, SF_U0, SF_V0, SF_W0, dead);
        if (cg)
            op_project_cg(SF_U, SF_V, SF_W, SF_U0, SF_V0, cg_tol_, cg_max_iters_, dead);
        else
            op_project(SF_U, SF_V, SF_W, SF_U0, SF_V0, dead, false);
    }

    // SPEC §3 dens_step.
    void dens_step_body() {
        const int x[1] = {SF_DENS}, x0[1] = {SF_DENS0}, b0[1] = {0};
        const T a = diffusion_a(diff_);
        if (obst_on_ && obst_tr_) {  // SPEC §17: nothing enters a solid, so nothing is zeroed at the end
            SF_REQUIRE(mc_dens_ != SF_ADVECT_MACCORMACK || obst_mc_,
                       "dens_step: MacCormack advection of the density under sf_set_obstacle_transport(1) is not supported");
            if (bound_[3] >= 0) copy_field(SF_DENS0, bound_[3]);
            op_add_source<1>(x, x0);
            swap_slots(SF_DENS0, SF_DENS);
            op_lin_solve_masked<1>(x, x0, b0, a, T(1) + T(6) * a, K_);
            swap_slots(SF_DENS0, SF_DENS);
            if (mc_dens_ == SF_ADVECT_MACCORMACK)  // SPEC §18
                op_advect_mc_masked<1>(x, x0, b0, SF_U, SF_V, SF_W);
            else
                op_advect_masked<1>(x, x0, b0, SF_U, SF_V, SF_W);
            return;
        }
        if (bound_[3] >= 0) {
            const int src[1] = {bound_[3]};
            op_diffuse_src<1>(x, x0, b0, src, a, T(1) + T(6) * a, K_, false);
        } else {
            op_add_source<1>(x, x0);
            swap_slots(SF_DENS0, SF_DENS);
            op_lin_solve<1>(x, x0, b0, a, T(1) + T(6) * a, K_, false);
        }
        swap_slots(SF_DENS0, SF_DENS);
        if (mc_dens_ == SF_ADVECT_MACCORMACK)
            op_advect_mc<1>(x, x0, b0, SF_U, SF_V, SF_W, false);
        else
            op_advect<1>(x, x0, b0, SF_U, SF_V, SF_W, false);
        if (obst_on_) op_zero_solid(SF_DENS);
    }

    void set_iters(int iters) override {
        SF_REQUIRE(iters >= 0, "iters must be >= 0");
        K_ = iters;
    }
    void set_coefficients(double dt, double diff, double visc) override {
        dt_ = (T)dt;
        diff_ = (T)diff;
        visc_ = (T)visc;
    }

    void sync() override {
        join();
        SF_HIP(hipSetDevice(device_));
        for (Slab& sl : slabs_) {
            SF_HIP(hipStreamSynchronize(sl.cs));
            SF_HIP(hipStreamSynchronize(sl.bs));
            SF_HIP(hipStreamSynchronize(sl.hs));
        }
        if (P_ > 1) {
            bool exceeded = false;
            for (Slab& sl : slabs_) {
                int flag = 0;
                SF_HIP(hipMemcpy(&flag, sl.d_flag, sizeof(int), hipMemcpyDeviceToHost));
                if (flag) {
                    exceeded = true;
                    SF_HIP(hipMemset(sl.d_flag, 0, sizeof(int)));
                    SF_HIP(hipDeviceSynchronize());
                }
            }
            int tr_bits = 0;  // decomposed tracers: bit 0 overflow, bit 1 a tracer skipped a slab
            for (Slab& sl : slabs_) {
                if (!sl.tr_flag) continue;
                int flag = 0;
                SF_HIP(hipMemcpy(&flag, sl.tr_flag, sizeof(int), hipMemcpyDeviceToHost));
                if (flag) {
                    tr_bits |= flag;
                    SF_HIP(hipMemset(sl.tr_flag, 0, sizeof(int)));
                    SF_HIP(hipDeviceSynchronize());
                }
            }
            if (exceeded)
                throw Failure{SF_ERR_HALO_EXCEEDED,
                              "advect back-traced more than one plane across a slab boundary "
                              "(|dt*N*w| >= 1): results differ from the undecomposed solve"};
            if (tr_bits & 1)
                throw Failure{SF_ERR_TRACER_OVERFLOW,
                              "more tracers left a slab for one neighbour in one tracers_advect than the capacity "
                              "(sf_tracers_set_capacity) holds: the surplus stayed with the slab they left, and the "
                              "tracers are no longer those of the undecomposed run"};
            if (tr_bits & 2)
                throw Failure{SF_ERR_HALO_EXCEEDED,
                              "a tracer moved past a neighbouring slab in one tracers_advect (|dt*N*v_z| >= planes "
                              "per slab): it stayed with the slab it left, and the tracers are no longer those of "
                              "the undecomposed run"};
        }
    }

    void timer_start() override {
        join();
        SF_HIP(hipSetDevice(device_));
        SF_HIP(hipEventRecord(t0_, slabs_[0].cs));
    }
    float timer_stop() override {
        join();
        SF_HIP(hipEventRecord(t1_, slabs_[0].cs));
        SF_HIP(hipEventSynchronize(t1_));
        float ms = 0.f;
        SF_HIP(hipEventElapsedTime(&ms, t0_, t1_));
        return ms;
    }

    double copy_bandwidth(size_t bytes, int reps) override {
        join();
        SF_HIP(hipSetDevice(device_));
        bytes = (bytes + 4095) / 4096 * 4096;
        if (copy_bytes_ != bytes) {
            own_.release(copy_src_);
            own_.release(copy_dst_);
            copy_bytes_ = 0;
            copy_src_ = own_.dev<void>(bytes);
            copy_dst_ = own_.dev<void>(bytes);
            SF_HIP(hipMemset(copy_src_, 1, bytes));
            SF_HIP(hipMemset(copy_dst_, 0, bytes));
            SF_HIP(hipDeviceSynchronize());
            copy_bytes_ = bytes;
        }
        const long n = (long)(bytes / 16);
        hipStream_t st = slabs_[0].cs;
        double best_ms = 1e30;
        for (int r = 0; r <= reps; ++r) {
            SF_HIP(hipEventRecord(t0_, st));
            // one thread per 16 bytes, the grid in memory order: the shape that reaches 6.2-6.3 TB/s here
            // (tools/membench.hip); a grid-stride loop over a few thousand blocks stays at 5.0-5.9
            hipLaunchKernelGGL(sfk::copy16_kernel, dim3((unsigned)ceil_div(n, 256L)), dim3(256), 0, st,
                               (const float4*)copy_src_, (float4*)copy_dst_, n);
            SF_HIP(hipEventRecord(t1_, st));
            SF_HIP(hipEventSynchronize(t1_));
            float ms = 0.f;
            SF_HIP(hipEventElapsedTime(&ms, t0_, t1_));
            if (r > 0 && ms < best_ms) best_ms = ms;
        }
        return 2.0 * (double)bytes / (best_ms * 1e-3) / 1e9;
    }

    // ---- asynchronous output -----------------------------------------------------------------
    void snapshot(const int* fields, int nfields) override {
        join();
        SF_REQUIRE(fields != nullptr && nfields >= 1 && nfields <= 4, "snapshot takes 1..4 fields");
        SF_HIP(hipSetDevice(device_));
        for (int q = 0; q < nfields; ++q) check_field(fields[q]);
        for (Slab& sl : slabs_) {
            if (!sl.os) sl.os = own_.stream(hipStreamNonBlocking);
            if (!sl.snap_done) sl.snap_done = own_.event(hipEventDisableTiming);
            for (int q = 0; q < nfields; ++q) {
                if (!sl.snap[q]) sl.snap[q] = alloc_field();
                SF_HIP(hipMemcpyAsync(sl.snap[q], ensure(sl, fields[q]), (size_t)field_elems_ * sizeof(T),
                                      hipMemcpyDeviceToDevice, sl.cs));
            }
            SF_HIP(hipEventRecord(sl.snap_done, sl.cs));
        }
        snap_count_ = nfields;
    }

    // May run on another host thread: touches only the snapshot buffers, the output stream and snap_done.
    void snapshot_read(int index, void* host) override {
        SF_REQUIRE(host != nullptr, "null host pointer");
        // the planes this context is the owner of (shell planes on the end slabs), at their place in the GLOBAL array
        snapshot_read_planes(index, 0, N_ + 2, host);
    }

    // Planes [kb, ke) of snapshot `index` into a host array that holds exactly those planes (dense (N+2)^2 each).
    void snapshot_read_planes(int index, int kb, int ke, void* host) override {
        SF_REQUIRE(index >= 0 && index < snap_count_, "snapshot index out of range");
        SF_REQUIRE(host != nullptr, "null host pointer");
        SF_REQUIRE(kb < ke, "empty plane range");
        SF_HIP(hipSetDevice(device_));
        const size_t S = (size_t)N_ + 2;
        bool any = false;
        for (Slab& sl : slabs_) {
            SF_HIP(hipStreamWaitEvent(sl.os, sl.snap_done, 0));
            int ob, oe;
            owned_range(sl, ob, oe);
            const int b = std::max(kb, ob), e = std::min(ke, oe);
            if (b >= e) continue;
            any = true;
            copy_planes_out(sl, sl.snap[index], sl.os, b, e, static_cast<T*>(host) + (size_t)(b - kb) * S * S);
        }
        SF_REQUIRE(any, "plane range not stored by this context");
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.os));
    }

    // ---- tracers (SPEC §6; decomposed contexts §6.1) ------------------------------------------------------------
    void tracers_set(int n, const void* xyz) override {
        join();
        SF_REQUIRE(n >= 0 && (n == 0 || xyz != nullptr), "bad tracer array");
        SF_HIP(hipSetDevice(device_));
        tracers_free();
        tr_n_ = n;
        if (n == 0) return;
        tr_pos_ = own_.dev<T>((size_t)3 * n * sizeof(T));
        tr_dens_ = own_.dev<T>((size_t)n * sizeof(T));
        tr_speed_ = own_.dev<T>((size_t)n * sizeof(T));
        if (P_ == 1) {
            SF_HIP(hipMemcpyAsync(tr_pos_, xyz, (size_t)3 * n * sizeof(T), hipMemcpyHostToDevice, slabs_[0].cs));
            SF_HIP(hipStreamSynchronize(slabs_[0].cs));
            return;
        }
        // every rank gets the same global array and keeps the tracers its slabs own; the id is the index, positions
        // stay raw (unclamped) until the first tracers_advect
        const T* p = static_cast<const T*>(xyz);
        std::vector<std::vector<sfk::TracerRec<T>>> own(L_);
        for (int t = 0; t < n; ++t) {
            const int s = tracer_owner(p[3 * t + 2]) - rank_ * L_;
            if (s >= 0 && s < L_) own[s].push_back(sfk::TracerRec<T>{p[3 * t], p[3 * t + 1], p[3 * t + 2], t});
        }
        tr_ids_ = own_.dev<int>((size_t)n * sizeof(int));
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            for (auto*& l : sl.tr_list) l = own_.dev<sfk::TracerRec<T>>((size_t)n * sizeof(sfk::TracerRec<T>));
            sl.tr_cnt = own_.dev<int>(2 * sizeof(int));
            sl.tr_flag = own_.dev<int>(sizeof(int));
            const int cnt[2] = {(int)own[s].size(), 0}, zero = 0;
            if (!own[s].empty())
                SF_HIP(hipMemcpy(sl.tr_list[0], own[s].data(), own[s].size() * sizeof(sfk::TracerRec<T>),
                                 hipMemcpyHostToDevice));
            SF_HIP(hipMemcpy(sl.tr_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
            SF_HIP(hipMemcpy(sl.tr_flag, &zero, sizeof zero, hipMemcpyHostToDevice));
        }
        tr_cur_ = 0;
        tracers_alloc_messages();
    }

    void tracers_set_capacity(int per_direction) override {
        SF_REQUIRE(per_direction >= 1, "tracer capacity must be >= 1");
        join();
        SF_HIP(hipSetDevice(device_));
        tr_cap_req_ = per_direction;
        if (P_ > 1 && tr_n_ > 0) tracers_alloc_messages();
    }

    // One dt for every tracer. P > 1: per slab one kernel advects, classifies and compacts its tracers (keepers into
    // the other list of the pair, migrants into the send buffer of their direction); the send buffers then reach the
    // neighbours through the ghost-plane transports — read in place by a neighbour in this process, one grouped RCCL
    // send / receive per neighbouring process (all slabs in one group under SF_FLAG_RCCL_SELF), a local copy under
    // SF_FLAG_LOOPBACK_HALO — and a second kernel appends the arrivals. Nothing is read back to the host.
    void tracers_advect() override {
        join();
        if (tr_n_ == 0) return;
        SF_HIP(hipSetDevice(device_));
        if (P_ == 1) {
            Slab& sl = slabs_[0];
            hipLaunchKernelGGL((sfk::tracers_advect_kernel<T>), dim3((unsigned)ceil_div(tr_n_, 256)), dim3(256), 0,
                               sl.cs, sl.geom, tr_n_, tr_pos_, sl.field[SF_U], sl.field[SF_V], sl.field[SF_W],
                               dt_ * (T)N_);
            SF_HIP(hipGetLastError());
            return;
        }
        const int cur = tr_cur_, nxt = cur ^ 1;
        // the previous call's arrivals kernels of neighbours in this process read this slab's send buffers
        for (Slab& sl : slabs_) ev_record(sl, &Slab::cs_mark, sl.cs);
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            for (int d = 0; d < 2; ++d)
                if (tr_side(s, d) == TR_LOCAL) st_wait(sl, sl.cs, slabs_[s + (d ? 1 : -1)], &Slab::cs_mark);
            hipLaunchKernelGGL(sfk::tracers_reset_kernel, dim3(1), dim3(64), 0, sl.cs, sl.tr_cnt + nxt,
                               sl.tr_send[0] ? &sl.tr_send[0]->id : nullptr, sl.tr_send[1] ? &sl.tr_send[1]->id : nullptr);
            sfk::TracerMoveArgs<T> A;
            A.in = sl.tr_list[cur];
            A.n_in = sl.tr_cnt + cur;
            A.keep = sl.tr_list[nxt];
            A.n_keep = sl.tr_cnt + nxt;
            A.send[0] = sl.tr_send[0];
            A.send[1] = sl.tr_send[1];
            A.cap = tr_cap_;
            A.list_cap = tr_n_;
            A.gid = sl.gid;
            A.u = sl.field[SF_U];
            A.v = sl.field[SF_V];
            A.w = sl.field[SF_W];
            A.dt0 = dt_ * (T)N_;
            A.flag = sl.tr_flag;
            hipLaunchKernelGGL((sfk::tracers_move_kernel<T>), dim3(tracer_grid(tr_n_)), dim3(256), 0, sl.cs, sl.geom, A);
            SF_HIP(hipGetLastError());
            tr_whole("tracers_move", sl, {A.u, A.v, A.w, A.in},
                     {A.keep, sl.tr_send[0] ? (const void*)sl.tr_send[0] : A.keep,
                      sl.tr_send[1] ? (const void*)sl.tr_send[1] : A.keep});
        }
        for (Slab& sl : slabs_) ev_record(sl, &Slab::cs_mark, sl.cs);
        tracers_transport();
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            sfk::TracerArriveArgs<T> A;
            bool msg = false;
            for (int d = 0; d < 2; ++d) {
                const int side = tr_side(s, d);
                Slab* nb = side == TR_NONE ? nullptr : &slabs_[s + (d ? 1 : -1)];
                A.src[d] = side == TR_LOCAL ? nb->tr_send[1 - d] : (side == TR_MSG ? sl.tr_recv[d] : nullptr);
                if (side == TR_LOCAL) st_wait(sl, sl.cs, *nb, &Slab::cs_mark);
                if (side == TR_MSG && rccl_self_) st_wait(sl, sl.cs, *nb, &Slab::halo_done);
                msg = msg || side == TR_MSG;
            }
            if (msg) st_wait(sl, sl.cs, sl, &Slab::halo_done);
            A.cap = tr_cap_;
            A.list = sl.tr_list[nxt];
            A.n_list = sl.tr_cnt + nxt;
            A.list_cap = tr_n_;
            A.flag = sl.tr_flag;
            hipLaunchKernelGGL((sfk::tracers_arrive_kernel<T>), dim3(tracer_grid(tr_cap_), 2), dim3(256), 0, sl.cs, A);
            SF_HIP(hipGetLastError());
            tr_whole("tracers_arrive", sl, {A.src[0] ? (const void*)A.src[0] : A.list, A.src[1] ? (const void*)A.src[1] : A.list},
                     {A.list});
        }
        tr_cur_ = nxt;
    }

    void tracers_get(void* xyz, void* dens, void* speed) override {
        join();
        SF_REQUIRE(nranks_ == 1, "sf_tracers_get returns every tracer, but this context holds only its rank's: "
                                 "use sf_tracers_get_owned on a multi-rank context");
        if (tr_n_ == 0) return;
        SF_HIP(hipSetDevice(device_));
        Slab& sl = slabs_[0];
        if (P_ == 1) {
            if (dens || speed) {
                hipLaunchKernelGGL((sfk::tracers_sample_kernel<T>), dim3((unsigned)ceil_div(tr_n_, 256)), dim3(256), 0,
                                   sl.cs, sl.geom, tr_n_, tr_pos_, sl.field[SF_DENS], sl.field[SF_U], sl.field[SF_V],
                                   sl.field[SF_W], tr_dens_, tr_speed_);
                SF_HIP(hipGetLastError());
            }
        } else {
            // every slab scatters its tracers by id into the dense arrays (disjoint ids; read back after a host sync)
            for (Slab& s : slabs_) tracers_out(s, -1, dens || speed, false);
            for (Slab& s : slabs_) SF_HIP(hipStreamSynchronize(s.cs));
        }
        if (xyz) SF_HIP(hipMemcpyAsync(xyz, tr_pos_, (size_t)3 * tr_n_ * sizeof(T), hipMemcpyDeviceToHost, sl.cs));
        if (dens) SF_HIP(hipMemcpyAsync(dens, tr_dens_, (size_t)tr_n_ * sizeof(T), hipMemcpyDeviceToHost, sl.cs));
        if (speed) SF_HIP(hipMemcpyAsync(speed, tr_speed_, (size_t)tr_n_ * sizeof(T), hipMemcpyDeviceToHost, sl.cs));
        SF_HIP(hipStreamSynchronize(sl.cs));
    }

    int tracers_owned() override {
        join();
        SF_HIP(hipSetDevice(device_));
        if (P_ == 1 || tr_n_ == 0) return tr_n_;
        int total = 0;
        for (int c : tracer_counts()) total += c;
        return total;
    }

    // The tracers of this context in ascending id order (what one rank writes into its point-mesh file).
    void tracers_get_owned(int* ids, void* xyz, void* dens, void* speed) override {
        join();
        if (tr_n_ == 0) return;
        SF_HIP(hipSetDevice(device_));
        if (P_ == 1) {
            if (ids)
                for (int t = 0; t < tr_n_; ++t) ids[t] = t;
            if (xyz || dens || speed) tracers_get(xyz, dens, speed);
            return;
        }
        const std::vector<int> cnt = tracer_counts();
        int total = 0;
        for (int s = 0; s < L_; ++s) {
            tracers_out(slabs_[s], total, dens || speed, true);
            total += cnt[s];
        }
        total = std::min(total, tr_n_);
        for (Slab& s : slabs_) SF_HIP(hipStreamSynchronize(s.cs));
        std::vector<int> hid(total);
        std::vector<T> hpos((size_t)3 * total), hd(total), hs(total);
        if (total > 0) {
            SF_HIP(hipMemcpy(hid.data(), tr_ids_, (size_t)total * sizeof(int), hipMemcpyDeviceToHost));
            SF_HIP(hipMemcpy(hpos.data(), tr_pos_, (size_t)3 * total * sizeof(T), hipMemcpyDeviceToHost));
            if (dens || speed) {
                SF_HIP(hipMemcpy(hd.data(), tr_dens_, (size_t)total * sizeof(T), hipMemcpyDeviceToHost));
                SF_HIP(hipMemcpy(hs.data(), tr_speed_, (size_t)total * sizeof(T), hipMemcpyDeviceToHost));
            }
        }
        std::vector<int> order(total);
        for (int q = 0; q < total; ++q) order[q] = q;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return hid[a] < hid[b]; });
        for (int q = 0; q < total; ++q) {
            const int o = order[q];
            if (ids) ids[q] = hid[o];
            if (xyz)
                for (int c = 0; c < 3; ++c) static_cast<T*>(xyz)[3 * q + c] = hpos[3 * (size_t)o + c];
            if (dens) static_cast<T*>(dens)[q] = hd[o];
            if (speed) static_cast<T*>(speed)[q] = hs[o];
        }
    }

    // ---- reductions and diagnostics (SPEC §10) -------------------------------------------------------------------
    // Both calls: row records (one wave per row) and plane records (one workgroup per plane and value) on each slab's
    // compute stream, the plane records to pinned host memory, the fold over global k on the host. They synchronise.
    void reduce(int op, int field, double* out) override {
        SF_REQUIRE(out != nullptr, "null result pointer");
        SF_REQUIRE(op >= SF_RED_SUM && op <= SF_RED_COUNT_NONFINITE, "reduce: op out of range");
        check_field(field);
        join();
        SF_HIP(hipSetDevice(device_));
        records_alloc();
        auto go = [&](auto kernel) {
            launch_rows("reduce_rows", kernel, [&](Slab& sl) { return (const T*)ensure(sl, field); },
                        [&](Slab& sl) { return std::vector<Acc>{{sl.field[field], false, G_, G_ + nzl_}}; });
        };
        switch (op) {
            case SF_RED_SUM: go(sfk::reduce_rows_kernel<T, sfk::RED_SUM>); break;
            case SF_RED_SUM_SQ: go(sfk::reduce_rows_kernel<T, sfk::RED_SUM_SQ>); break;
            case SF_RED_MIN: go(sfk::reduce_rows_kernel<T, sfk::RED_MIN>); break;
            case SF_RED_MAX: go(sfk::reduce_rows_kernel<T, sfk::RED_MAX>); break;
            case SF_RED_MAX_ABS: go(sfk::reduce_rows_kernel<T, sfk::RED_MAX_ABS>); break;
            default: go(sfk::reduce_rows_kernel<T, sfk::RED_COUNT_NONFINITE>); break;
        }
        const bool sum = op == SF_RED_SUM || op == SF_RED_SUM_SQ || op == SF_RED_COUNT_NONFINITE;
        const int nsum = sum ? 1 : 0, nmin = op == SF_RED_MIN ? 1 : 0;
        double r[1];
        finish_records(1, nsum, nmin, r);
        *out = r[0];
    }

    void diagnostics(sf_diagnostics* out) override {
        SF_REQUIRE(out != nullptr, "null result pointer");
        join();
        SF_HIP(hipSetDevice(device_));
        records_alloc();
        launch_rows("diag_rows", sfk::diag_rows_kernel<T>, [&](Slab& sl) {
            sfk::DiagArgs<T> A;
            A.u = sl.field[SF_U];
            A.v = sl.field[SF_V];
            A.w = sl.field[SF_W];
            A.dens = sl.field[SF_DENS];
            A.c_div = T(-0.5) * (T(1) / (T)N_);
            A.dt0 = dt_ * (T)N_;
            return A;
        }, [&](Slab& sl) {
            return std::vector<Acc>{{sl.field[SF_U], false, G_, G_ + nzl_}, {sl.field[SF_V], false, G_, G_ + nzl_},
                                    {sl.field[SF_W], false, G_ - 1, G_ + nzl_ + 1}, {sl.field[SF_DENS], false, G_, G_ + nzl_}};
        });
        // record order of sfk::diag_rows_kernel: 0 mass, 1 kinetic sum, 2 nonfinite (sums), 3 dens_min (minimum),
        // 4 dens_max, 5 max speed^2, 6 max_div, 7..9 cfl_x, y, z (maxima)
        double r[sfk::DIAG_NV];
        finish_records(sfk::DIAG_NV, 3, 1, r);
        const double n3 = (double)N_ * (double)N_ * (double)N_;
        out->mass = r[0];
        out->kinetic = (0.5 * r[1]) / n3;
        out->nonfinite = (long long)r[2];
        out->dens_min = r[3];
        out->dens_max = r[4];
        out->max_speed = std::sqrt(r[5]);
        out->max_div = r[6];
        out->cfl_x = r[7];
        out->cfl_y = r[8];
        out->cfl_z = r[9];
        out->cfl = std::max(std::max(r[7], r[8]), r[9]);
    }

    // ---- conjugate-gradient projection (SPEC §11) ---------------------------------------------------------------
    static void check_cg(double tol, int max_iters) {
        SF_REQUIRE(std::isfinite(tol) && tol > 0.0, "pressure solver: tol must be finite and > 0");
        SF_REQUIRE(max_iters >= 0, "pressure solver: max_iters must be >= 0");
    }
    void set_pressure_solver(int solver, double tol, int max_iters) override {
        SF_REQUIRE(solver == SF_PRESSURE_JACOBI || solver == SF_PRESSURE_CG, "pressure solver must be 0 (Jacobi) or 1 (CG)");
        check_cg(tol, max_iters);
        pressure_ = solver;
        cg_tol_ = tol;
        cg_max_iters_ = max_iters;
    }
    void project_cg(int u, int v, int w, int p, int div, double tol, int max_iters) override {
        check_distinct("project_cg: fields must be distinct", {u, v, w, p, div});
        check_cg(tol, max_iters);
        SF_HIP(hipSetDevice(device_));
        op_project_cg(u, v, w, p, div, tol, max_iters);
    }
    void poisson_residual(int p, int div, double* rel) override {
        SF_REQUIRE(rel != nullptr, "null result pointer");
        check_field(p);
        check_field(div);
        SF_REQUIRE(p != div, "poisson_residual: p and div must be different fields");
        join();
        SF_HIP(hipSetDevice(device_));
        records_alloc();
        auto args = [&](Slab& sl) {
            sfk::CgArgs<T> A{};
            A.p = ensure(sl, p);
            A.div = ensure(sl, div);
            return A;
        };
        auto acc = [&](Slab& sl) {
            std::vector<Acc> a{{sl.field[p], false, G_ - 1, G_ + nzl_ + 1}, {sl.field[div], false, G_, G_ + nzl_}};
            if (obst_on_) a.push_back({sl.field[OBST_SLOT], false, G_, G_ + nzl_});
            return a;
        };
        if (obst_on_)
            launch_rows("poisson_residual_masked", sfk::cg_apply_dot_masked_kernel<T, true>,
                        [&](Slab& sl) { return sfk::CgMaskArgs<T>{args(sl), sl.field[OBST_SLOT]}; }, acc);
        else
            launch_rows("poisson_residual", sfk::cg_apply_dot_kernel<T, true>, args, acc);
        double r[2];
        finish_records(2, 2, 0, r);
        *rel = r[1] == 0.0 ? 0.0 : std::sqrt(r[0] / r[1]);
    }
    // SPEC §15: the mask of slot `mask_slot` becomes the face codes every masked kernel reads; -1: off
    void set_obstacles(int mask_slot) override {
        SF_REQUIRE(mask_slot >= -1 && mask_slot < SF_NUM_FIELDS, "set_obstacles: slot out of range (-1: off)");
        SF_HIP(hipSetDevice(device_));
        sync();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);  // a dens_step of the other form
        graph_cache_.clear();
        mg_codes_ok_ = false;
        if (mask_slot < 0) {
            obst_on_ = false;
            return;
        }
        records_alloc();
        for (Slab& sl : slabs_) {
            ensure(sl, mask_slot);
            if (!sl.field[OBST_SLOT]) sl.field[OBST_SLOT] = alloc_field();
        }
        launch_rows("face_code", sfk::face_code_kernel<T>,
                    [&](Slab& sl) { return sfk::FaceCodeArgs<T>{sl.field[mask_slot], sl.field[OBST_SLOT]}; },
                    [&](Slab& sl) {
                        return std::vector<Acc>{{sl.field[mask_slot], false, G_ - 1, G_ + nzl_ + 1},
                                                {sl.field[OBST_SLOT], true, G_, G_ + nzl_}};
                    });
        double n[1];
        finish_records(1, 1, 0, n);
        n_fluid_ = (long long)n[0];
        obst_on_ = true;
        if (obst_tr_) code_shells_publish();
    }
    void obstacles(sf_obstacles* out) const override {
        out->enabled = obst_on_ ? 1 : 0;
        out->fluid_cells = obst_on_ ? n_fluid_ : (long long)N_ * N_ * N_;
    }
    // SPEC §16: with obstacles on and the V-cycle in force, the masked V-cycle instead of the refusal
    void set_obstacle_multigrid(int on) override {
        SF_REQUIRE(on == 0 || on == 1, "obstacle multigrid: on must be 0 or 1");
        SF_HIP(hipSetDevice(device_));
        sync();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);
        graph_cache_.clear();
        obst_mg_ = on != 0;
    }
    void obstacle_multigrid(int* on) const override { *on = obst_mg_ ? 1 : 0; }
    void precondition_masked(int z, int r) override {
        check_distinct("precondition_masked: z and r must be different fields", {z, r});
        SF_REQUIRE(obst_on_ && mg_nu_ > 0 && obst_mg_,
                   "precondition_masked: needs obstacles (sf_set_obstacles), the multigrid preconditioner "
                   "(sf_set_pressure_multigrid) and sf_set_obstacle_multigrid(1)");
        SF_HIP(hipSetDevice(device_));
        pcg_alloc();
        records_alloc();
        for (Slab& sl : slabs_)
            for (int f : {z, r}) ensure(sl, f);
        join();
        op_precondition(mg_nu_, z, r, true);
    }
    // SPEC §17: with obstacles on, the diffuse and advect of both steps are the masked forms
    void set_obstacle_transport(int on) override {
        SF_REQUIRE(on == 0 || on == 1, "obstacle transport: on must be 0 or 1");
        SF_HIP(hipSetDevice(device_));
        sync();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);  // a step of the other form
        graph_cache_.clear();
        obst_tr_ = on != 0;
        if (obst_tr_ && obst_on_) code_shells_publish();
    }
    void obstacle_transport(int* on) const override { *on = obst_tr_ ? 1 : 0; }
    void diffuse_masked(int b, int x, int x0, double diff) override {
        check_field(x);
        check_field(x0);
        check_b(b);
        SF_REQUIRE(x != x0, "diffuse_masked: x and x0 must be different fields");
        SF_REQUIRE(obst_on_ && obst_tr_, "diffuse_masked: needs obstacles (sf_set_obstacles) and sf_set_obstacle_transport(1)");
        SF_HIP(hipSetDevice(device_));
        const int xs[1] = {x}, x0s[1] = {x0}, bs[1] = {b};
        const T a = diffusion_a((T)diff);
        op_lin_solve_masked<1>(xs, x0s, bs, a, T(1) + T(6) * a, K_);
    }
    void advect_masked(int b, int d, int d0, int u, int v, int w) override {
        for (int f : {d, d0, u, v, w}) check_field(f);
        check_b(b);
        SF_REQUIRE(d != d0 && d != u && d != v && d != w, "advect_masked: output must not alias an input");
        SF_REQUIRE(obst_on_ && obst_tr_, "advect_masked: needs obstacles (sf_set_obstacles) and sf_set_obstacle_transport(1)");
        SF_HIP(hipSetDevice(device_));
        const int ds[1] = {d}, d0s[1] = {d0}, bs[1] = {b};
        op_advect_masked<1>(ds, d0s, bs, u, v, w);
    }
    // SPEC §18: with obstacles and transport on, a MacCormack scheme runs advect_mc_masked instead of the refusal
    void set_obstacle_maccormack(int on) override {
        SF_REQUIRE(on == 0 || on == 1, "obstacle maccormack: on must be 0 or 1");
        SF_HIP(hipSetDevice(device_));
        sync();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);  // a step of the other form
        graph_cache_.clear();
        obst_mc_ = on != 0;
    }
    void obstacle_maccormack(int* on) const override { *on = obst_mc_ ? 1 : 0; }
    // SPEC §19: the slots su, sv, sw are copied whole into the three OBSTV slots; all -1: off
    void set_obstacle_velocity(int su, int sv, int sw) override {
        const bool off = su == -1 && sv == -1 && sw == -1;
        if (!off) {
            for (int f : {su, sv, sw})
                SF_REQUIRE(f >= 0 && f < SF_NUM_FIELDS,
                           "set_obstacle_velocity: slot out of range (three slots, or -1, -1, -1: off)");
            SF_REQUIRE(su != sv && su != sw && sv != sw, "set_obstacle_velocity: the three slots must be different fields");
        }
        SF_HIP(hipSetDevice(device_));
        sync();
        for (GraphEntry& e : graph_cache_) (void)hipGraphExecDestroy(e.exec);  // a step of the other form
        graph_cache_.clear();
        if (off) {
            obstv_on_ = false;
            return;
        }
        const int src[3] = {su, sv, sw}, dst[3] = {OBSTV_SLOT, OBSTV_SLOT + 1, OBSTV_SLOT + 2};
        for (Slab& sl : slabs_)
            for (int q = 0; q < 3; ++q) {
                ensure(sl, src[q]);
                if (!sl.field[dst[q]]) sl.field[dst[q]] = alloc_field();
                SF_HIP(hipMemcpyAsync(sl.field[dst[q]], sl.field[src[q]], (size_t)field_elems_ * sizeof(T),
                                      hipMemcpyDeviceToDevice, sl.cs));
                tr_whole("solid_velocity", sl, {sl.field[src[q]]}, {sl.field[dst[q]]});
            }
        obstv_on_ = true;
        if (P_ == 1) return;
        for (Slab& sl : slabs_) ev_record(sl, &Slab::boundary_done, sl.cs);
        exchange<3>(dst);
    }
    void obstacle_velocity(int* on) const override { *on = obstv_on_ ? 1 : 0; }
    void advect_maccormack_masked(int b, int d, int d0, int u, int v, int w) override {
        for (int f : {d, d0, u, v, w}) check_field(f);
        check_b(b);
        SF_REQUIRE(d != d0 && d != u && d != v && d != w, "advect_maccormack_masked: output must not alias an input");
        SF_REQUIRE(obst_on_ && obst_tr_,
                   "advect_maccormack_masked: needs obstacles (sf_set_obstacles) and sf_set_obstacle_transport(1)");
        // SPEC §19: there is no MacCormack form under a solid velocity; pass 1 would be the moving advect
        SF_REQUIRE(!(obstv_on_ && b != 0),
                   "advect_maccormack_masked: a velocity component (b = 1, 2, 3) under a solid velocity "
                   "(sf_set_obstacle_velocity) is not supported");
        SF_HIP(hipSetDevice(device_));
        const int ds[1] = {d}, d0s[1] = {d0}, bs[1] = {b};
        op_advect_mc_masked<1>(ds, d0s, bs, u, v, w);
    }
    void pressure_info(sf_pressure_info* out) const override { *out = info_; }
    void set_pressure_sync(int check_every) override {
        SF_REQUIRE(check_every >= 0, "pressure sync: check_every must be >= 0");
        check_every_ = check_every;
    }
    void set_pressure_preconditioner(int kind, int sweeps) override {
        SF_REQUIRE(kind == SF_PRECOND_NONE || kind == SF_PRECOND_JACOBI, "pressure preconditioner: unknown kind");
        SF_REQUIRE(sweeps >= (kind == SF_PRECOND_JACOBI ? 1 : 0),
                   "pressure preconditioner: sweeps must be >= 1 with SF_PRECOND_JACOBI (>= 0 with SF_PRECOND_NONE)");
        precond_ = kind;
        precond_sweeps_ = sweeps;
    }
    void pressure_preconditioner(sf_pressure_preconditioner* out) const override {
        out->kind = precond_;
        out->sweeps = precond_sweeps_;
    }
    void set_pressure_multigrid(int sweeps, int max_levels, int coarse_sweeps) override {
        SF_REQUIRE(sweeps >= 0, "pressure multigrid: sweeps must be >= 0 (0: off)");
        SF_REQUIRE(max_levels >= 0, "pressure multigrid: max_levels must be >= 0 (0: as deep as N allows)");
        SF_REQUIRE(coarse_sweeps >= 1, "pressure multigrid: coarse_sweeps must be >= 1");
        if (sweeps >= 1) {
            // every coarse level must split into whole planes per slab, so that no restriction crosses a slab
            const std::vector<int> n = mg_sizes(max_levels);
            int ok = 1;
            while (ok < (int)n.size() && n[ok] % P_ == 0) ++ok;
            if (ok < (int)n.size())
                throw Failure{SF_ERR_INVALID, "pressure multigrid: level " + std::to_string(ok) + " of N = " + std::to_string(N_) +
                                                  " has " + std::to_string(n[ok]) + " planes, not divisible by the " +
                                                  std::to_string(P_) + " slabs: the largest admissible max_levels is " +
                                                  std::to_string(ok)};
        }
        mg_nu_ = sweeps;
        mg_maxl_ = max_levels;
        mg_nuc_ = coarse_sweeps;
        mg_codes_ok_ = false;
    }
    void pressure_multigrid(sf_pressure_multigrid* out) const override {
        out->sweeps = mg_nu_;
        out->max_levels = mg_maxl_;
        out->coarse_sweeps = mg_nuc_;
        out->levels = (int)mg_sizes(mg_maxl_).size();
    }
    void precondition(int z, int r) override {
        check_distinct("precondition: z and r must be different fields", {z, r});
        const int pm = precond_sweeps_in_force();
        SF_REQUIRE(pm > 0, "precondition: no preconditioner is in force");
        SF_HIP(hipSetDevice(device_));
        pcg_alloc();
        for (Slab& sl : slabs_)
            for (int f : {z, r}) ensure(sl, f);
        join();
        op_precondition(pm, z, r);
    }
    // ---- volume rendering and light marching (SPEC §12) ----------------------------------------------------------
    static void check_rays(int axis, int from_high, double sigma) {
        SF_REQUIRE(axis >= 0 && axis <= 2, "ray axis must be 0 (i), 1 (j) or 2 (k)");
        SF_REQUIRE(from_high == 0 || from_high == 1, "from_high must be 0 or 1");
        SF_REQUIRE(std::isfinite(sigma) && sigma >= 0.0, "sigma must be finite and >= 0");
    }
    void render(const sf_render_params* p) override {
        SF_REQUIRE(p != nullptr, "null render params");
        check_rays(p->axis, p->from_high, p->sigma);
        check_field(p->dens);
        SF_REQUIRE(p->emit >= -1 && p->emit < SF_NUM_FIELDS, "emit must be a field id, or -1 for none");
        SF_HIP(hipSetDevice(device_));
        op_rays(p->emit >= 0 ? sfk::RAY_IMAGE_EMIT : sfk::RAY_IMAGE, p->axis, p->from_high, p->sigma, p->dens, p->emit, -1);
        ray_axis_ = p->axis;
        ray_high_ = p->from_high;
    }
    // Each slab's pixels go to pinned memory on its compute stream, so the copy waits for the render alone; then to the
    // caller's arrays at their place in the image.
    void render_read(void* colour, void* transmittance) override {
        SF_REQUIRE(ray_axis_ >= 0, "render_read before any render");
        SF_HIP(hipSetDevice(device_));
        const size_t NN = (size_t)N_ * N_;
        if (!ray_stage_) ray_stage_ = own_.pinned<T>(2 * NN * sizeof(T));
        std::vector<std::pair<size_t, size_t>> parts;  // pixels [first, second) held by this context
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            size_t b = (size_t)sl.gid * nzl_ * N_, e = b + (size_t)nzl_ * N_;  // i / j views: the rows of the owned planes
            if (ray_axis_ == 2) {
                if (!ray_leaves_here(s, ray_high_)) continue;
                b = 0, e = NN;  // k view: the whole image, on the slab the rays leave the grid from
            }
            for (size_t half : {(size_t)0, NN})
                SF_HIP(hipMemcpyAsync(ray_stage_ + half + b, sl.ray_img[0] + half + b, (e - b) * sizeof(T),
                                      hipMemcpyDeviceToHost, sl.cs));
            tr_op("render_out", sl, sl.cs, {{sl.ray_img[0], false, 0, nplanes_}});
            parts.push_back({b, e});
        }
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.cs));
        for (const auto& pr : parts) {
            const size_t bytes = (pr.second - pr.first) * sizeof(T);
            if (colour) std::memcpy(static_cast<T*>(colour) + pr.first, ray_stage_ + pr.first, bytes);
            if (transmittance) std::memcpy(static_cast<T*>(transmittance) + pr.first, ray_stage_ + NN + pr.first, bytes);
        }
    }
    // ---- orthographic volume rendering from any direction (SPEC §13) ----------------------------------------------
    void check_view(const sf_view_params* p) {
        SF_REQUIRE(p != nullptr, "null view params");
        for (const double* v : {p->origin, p->du, p->dv, p->step})
            for (int c = 0; c < 3; ++c) SF_REQUIRE(std::isfinite(v[c]), "the frame's vectors must be finite");
        SF_REQUIRE(std::isfinite(p->sigma) && p->sigma >= 0.0, "sigma must be finite and >= 0");
        SF_REQUIRE(p->width >= 1 && p->width <= 16384 && p->height >= 1 && p->height <= 16384,
                   "width and height must be in 1 .. 16384");
        SF_REQUIRE(p->samples >= 1 && p->samples <= 65536, "samples must be in 1 .. 65536");
        check_field(p->dens);
        SF_REQUIRE(p->emit >= -1 && p->emit < SF_NUM_FIELDS, "emit must be a field id, or -1 for none");
    }
    void render_view(const sf_view_params* p) override {
        check_view(p);
        SF_HIP(hipSetDevice(device_));
        op_view(*p);
    }
    // ---- perspective volume rendering (SPEC §14): into the image pair of §13, read by render_view_read --------------
    void render_camera(const sf_camera_params* p) override {
        SF_REQUIRE(p != nullptr, "null camera params");
        check_view(&p->view);
        for (const double* v : {p->step_du, p->step_dv})
            for (int c = 0; c < 3; ++c) SF_REQUIRE(std::isfinite(v[c]), "the frame's vectors must be finite");
        int passes = 0;
        SF_REQUIRE(camera_corner_rule<T>(*p, &passes), "a corner pixel's step vector or origin is not finite in the context's dtype");
        SF_HIP(hipSetDevice(device_));
        op_camera(*p, passes);
    }
    // The whole image is on the slab the rays leave the grid from (a loopback context: its own last slab); a context
    // without it writes nothing.
    void render_view_read(void* colour, void* transmittance) override {
        SF_REQUIRE(view_w_ > 0, "render_view_read before any render_view");
        SF_HIP(hipSetDevice(device_));
        const size_t WH = (size_t)view_w_ * view_h_;
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            if (!ray_leaves_here(s, view_high_)) continue;
            if (colour) SF_HIP(hipMemcpyAsync(colour, sl.ray_img[2], WH * sizeof(T), hipMemcpyDeviceToHost, sl.cs));
            if (transmittance)
                SF_HIP(hipMemcpyAsync(transmittance, sl.ray_img[2] + WH, WH * sizeof(T), hipMemcpyDeviceToHost, sl.cs));
            tr_op("render_view_out", sl, sl.cs, {{sl.ray_img[2], false, 0, nplanes_}});
            SF_HIP(hipStreamSynchronize(sl.cs));
        }
    }
    void light(int dst, int dens, int axis, int from_high, double sigma) override {
        check_rays(axis, from_high, sigma);
        check_distinct("light: dst and dens must be different fields", {dst, dens});
        SF_HIP(hipSetDevice(device_));
        op_rays(sfk::RAY_FIELD, axis, from_high, sigma, dens, -1, dst);
        op_set_bnd(0, dst, "light_set_bnd");
    }

    void pressure_sync(sf_pressure_sync* out) const override {
        out->check_every = check_every_;
        out->host_waits = host_waits_;
        out->host_waits_total = host_waits_total_;
    }

    int lin_solve_launches(int iters) const override {
        return (int)plan_solve(iters, false, false, false).size();
    }

    void schedule_info(int* trap, int* measured) const override {
        if (trap) *trap = trap_m_ > 1 ? trap_m_ : 0;
        if (measured) *measured = (tuned_trap_ >= 0 ? 1 : 0) | (tuned_split_ >= 0 ? 2 : 0) | (split_fields_ == 0 ? 4 : 0);
    }
    void transport_info(int* transport, long* groups) const override {
        if (transport)
            *transport = P_ == 1 ? 0 : (rccl_self_ ? 3 : (loopback_ ? 4 : (nranks_ > 1 ? 2 : 1)));
        if (groups) *groups = rccl_groups_;
    }
    void layout_info(int* pitch, int* planes, size_t* bytes) const override {
        if (pitch) *pitch = px_;
        if (planes) *planes = nplanes_;
        if (bytes) *bytes = (size_t)field_elems_ * sizeof(T);
    }

private:
    // ---- helpers --------------------------------------------------------------------------
    static void check_field(int f) { SF_REQUIRE(f >= 0 && f < SF_NUM_FIELDS, "field id out of range"); }
    static void check_b(int b) { SF_REQUIRE(b >= 0 && b <= 3, "boundary mode b must be 0..3"); }
    // every field valid (checked in order, each before it is compared) and no two the same: `what` is the message
    static void check_distinct(const char* what, std::initializer_list<int> fields) {
        for (const int* a = fields.begin(); a != fields.end(); ++a) {
            check_field(*a);
            for (const int* c = a + 1; c != fields.end(); ++c) SF_REQUIRE(*a != *c, what);
        }
    }

    // ---- decomposed tracers (SPEC §6.1) ------------------------------------------------------------------------
    // How the records of the neighbour below (d = 0) / above (d = 1) of local slab s reach it: no neighbour, read in
    // place from the neighbour's send buffer (same process), or a message into this slab's receive buffer.
    enum { TR_NONE = 0, TR_LOCAL = 1, TR_MSG = 2 };
    int tr_side(int s, int d) const {
        const int gid = slabs_[s].gid;
        if (d == 0 ? gid == 0 : gid == P_ - 1) return TR_NONE;
        const bool in_process = d == 0 ? s > 0 : s < L_ - 1;
        return (in_process && !rccl_self_) ? TR_LOCAL : TR_MSG;
    }
    // host twin of sfk::tracer_owner (same T arithmetic): the global slab whose planes the sample at height z reads
    int tracer_owner(T z) const {
        const T lo = T(0.5), hi = (T)N_ + T(0.5);
        if (z < lo) z = lo;
        if (z > hi) z = hi;
        int k0 = (z == z) ? (int)z : 0;
        k0 = k0 < 0 ? 0 : (k0 > N_ ? N_ : k0);
        return k0 == 0 ? 0 : (k0 - 1) / nzl_;
    }
    unsigned tracer_grid(int n) const {
        return (unsigned)std::max(1L, std::min(ceil_div((long)n, 256L), (long)num_cu_ * 8));
    }
    void tracers_free() {
        (void)hipDeviceSynchronize();  // earlier launches may still use the buffers
        own_.release(tr_pos_);
        own_.release(tr_dens_);
        own_.release(tr_speed_);
        own_.release(tr_ids_);
        for (Slab& sl : slabs_) {
            for (int q = 0; q < 2; ++q) {
                own_.release(sl.tr_list[q]);
                own_.release(sl.tr_send[q]);
                own_.release(sl.tr_recv[q]);
            }
            own_.release(sl.tr_cnt);
            own_.release(sl.tr_flag);
        }
        tr_n_ = 0;
    }
    // (Re)allocates the send / receive buffers for the capacity in force: a header record + tr_cap_ records each.
    void tracers_alloc_messages() {
        SF_HIP(hipDeviceSynchronize());
        tr_cap_ = tr_cap_req_ > 0 ? std::min(tr_cap_req_, tr_n_) : tr_n_;
        const size_t bytes = (size_t)(tr_cap_ + 1) * sizeof(sfk::TracerRec<T>);
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            for (int d = 0; d < 2; ++d) {
                own_.release(sl.tr_send[d]);
                own_.release(sl.tr_recv[d]);
                const int side = tr_side(s, d);
                if (side == TR_NONE) continue;
                sl.tr_send[d] = own_.dev<sfk::TracerRec<T>>(bytes);
                SF_HIP(hipMemset(sl.tr_send[d], 0, bytes));
                if (side == TR_MSG) {
                    sl.tr_recv[d] = own_.dev<sfk::TracerRec<T>>(bytes);
                    SF_HIP(hipMemset(sl.tr_recv[d], 0, bytes));
                }
            }
        }
        SF_HIP(hipDeviceSynchronize());
    }
    // The messages of one tracers_advect: issued on the halo streams after the move kernels (cs_mark), completion in
    // halo_done. Each message is the whole send buffer (header + capacity): the receiver cannot know the count on the
    // host without a sync.
    void tracers_transport() {
        const size_t bytes = (size_t)(tr_cap_ + 1) * sizeof(sfk::TracerRec<T>);
        if (rccl_self_) {
            // as exchange_rccl_self: every transfer is the pair (send from the owner, receive into the neighbour), all
            // slabs in one group
            for (int s = 0; s < L_; ++s) {
                Slab& sl = slabs_[s];
                st_wait(sl, sl.hs, sl, &Slab::cs_mark);
                if (s > 0) st_wait(sl, sl.hs, slabs_[s - 1], &Slab::cs_mark);
                if (s < L_ - 1) st_wait(sl, sl.hs, slabs_[s + 1], &Slab::cs_mark);
            }
            SF_NCCL(ncclGroupStart());
            for (int s = 0; s + 1 < L_; ++s) {
                Slab& lo = slabs_[s];
                Slab& hi = slabs_[s + 1];
                SF_NCCL(ncclSend(lo.tr_send[1], bytes, ncclUint8, 0, comm_, lo.hs));
                SF_NCCL(ncclRecv(hi.tr_recv[0], bytes, ncclUint8, 0, comm_, hi.hs));
                SF_NCCL(ncclSend(hi.tr_send[0], bytes, ncclUint8, 0, comm_, hi.hs));
                SF_NCCL(ncclRecv(lo.tr_recv[1], bytes, ncclUint8, 0, comm_, lo.hs));
            }
            SF_NCCL(ncclGroupEnd());
            ++rccl_groups_;
            for (int s = 0; s < L_; ++s) {
                Slab& sl = slabs_[s];
                if (trace_) {
                    std::vector<Acc> acc;
                    for (int d = 0; d < 2; ++d) {
                        if (!sl.tr_recv[d]) continue;
                        acc.push_back({sl.tr_send[d], false, 0, nplanes_});
                        acc.push_back({slabs_[s + (d ? 1 : -1)].tr_send[1 - d], false, 0, nplanes_});
                        acc.push_back({sl.tr_recv[d], true, 0, nplanes_});
                    }
                    tr_op("tracers_rccl_self", sl, sl.hs, acc);
                }
                ev_record(sl, &Slab::halo_done, sl.hs);
            }
            return;
        }
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            const bool m[2] = {tr_side(s, 0) == TR_MSG, tr_side(s, 1) == TR_MSG};
            if (!m[0] && !m[1]) continue;
            st_wait(sl, sl.hs, sl, &Slab::cs_mark);
            if (loopback_) {
                // SF_FLAG_LOOPBACK_HALO: the same bytes on the same stream, from this slab's own send buffers
                sfk::HaloCopyArgs H;
                H.nseg = 0;
                H.n16 = (long)(bytes / 16);
                for (int d = 0; d < 2; ++d)
                    if (m[d]) {
                        H.src[H.nseg] = reinterpret_cast<const float4*>(sl.tr_send[d]);
                        H.dst[H.nseg++] = reinterpret_cast<float4*>(sl.tr_recv[d]);
                    }
                const unsigned gx = (unsigned)std::max(1L, std::min((H.n16 + 255) / 256, 512L));
                hipLaunchKernelGGL(sfk::halo_copy_kernel, dim3(gx, H.nseg), dim3(256), 0, sl.hs, H);
                SF_HIP(hipGetLastError());
            } else {
                SF_NCCL(ncclGroupStart());
                for (int d = 0; d < 2; ++d)
                    if (m[d]) {
                        SF_NCCL(ncclSend(sl.tr_send[d], bytes, ncclUint8, rank_ + (d ? 1 : -1), comm_, sl.hs));
                        SF_NCCL(ncclRecv(sl.tr_recv[d], bytes, ncclUint8, rank_ + (d ? 1 : -1), comm_, sl.hs));
                    }
                SF_NCCL(ncclGroupEnd());
                ++rccl_groups_;
            }
            if (trace_) {
                std::vector<Acc> acc;
                for (int d = 0; d < 2; ++d)
                    if (m[d]) {
                        acc.push_back({sl.tr_send[d], false, 0, nplanes_});
                        acc.push_back({sl.tr_recv[d], true, 0, nplanes_});
                    }
                tr_op(loopback_ ? "tracers_loopback" : "tracers_rccl", sl, sl.hs, acc);
            }
            ev_record(sl, &Slab::halo_done, sl.hs);
        }
    }
    // Output kernel of one slab on its compute stream: scatter by id (offset < 0) or pack at offset, see
    // sfk::tracers_out_kernel. with_ids: also the ids (tr_ids_).
    void tracers_out(Slab& sl, int offset, bool sample, bool with_ids) {
        sfk::TracerOutArgs<T> A;
        A.list = sl.tr_list[tr_cur_];
        A.n_list = sl.tr_cnt + tr_cur_;
        A.list_cap = tr_n_;
        A.dens = sample ? ensure(sl, SF_DENS) : nullptr;
        A.u = sl.field[SF_U];
        A.v = sl.field[SF_V];
        A.w = sl.field[SF_W];
        A.n_out = tr_n_;
        A.offset = offset;
        A.pos = tr_pos_;
        A.dens_out = tr_dens_;
        A.speed_out = tr_speed_;
        A.id_out = with_ids ? tr_ids_ : nullptr;
        hipLaunchKernelGGL((sfk::tracers_out_kernel<T>), dim3(tracer_grid(tr_n_)), dim3(256), 0, sl.cs, sl.geom, A);
        SF_HIP(hipGetLastError());
        // (the dense output arrays are written at disjoint indices by the slabs and read after a host sync: not traced)
        tr_whole("tracers_out", sl, {A.list, A.u, A.v, A.w, sample ? (const void*)A.dens : A.list}, {});
    }
    // Tracers held per local slab now (synchronises).
    std::vector<int> tracer_counts() {
        std::vector<int> c(L_, 0);
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            SF_HIP(hipStreamSynchronize(sl.cs));
            SF_HIP(hipMemcpy(&c[s], sl.tr_cnt + tr_cur_, sizeof(int), hipMemcpyDeviceToHost));
            c[s] = std::max(0, std::min(c[s], tr_n_));
        }
        return c;
    }

    T* alloc_field(const Level* lv = nullptr) {
        const Level& h = lv ? *lv : lv0_;
        const size_t total = (size_t)(h.pad_front + h.elems + h.pad_back) * sizeof(T);
        T* p = own_.dev<T>(total);
        SF_HIP(hipMemset(p, 0, total));
        // hipMemset on device memory may return before the fill has run, and the context's streams are
        // non-blocking (they do not order against the null stream): wait here.
        SF_HIP(hipDeviceSynchronize());
        return p + h.pad_front;
    }
    T* ensure(Slab& sl, int f) {
        if (!sl.field[f]) {
            // allocation is synchronous with respect to the device; fine for the lazily created user slots
            sl.field[f] = alloc_field();
        }
        return sl.field[f];
    }
    void swap_slots(int a, int b) {
        for (Slab& sl : slabs_) std::swap(sl.field[a], sl.field[b]);
    }
    T diffusion_a(T coeff) const {
        const T Nf = (T)N_;
        return ((dt_ * coeff) * Nf) * Nf;
    }
    unsigned stream_grid(long nvec) const {
        long blocks = (nvec + 255) / 256;
        const long cap = (long)num_cu_ * 8;
        return (unsigned)std::max(1L, std::min(blocks, cap));
    }

    // the planes of the global array that slab sl is the owner of: its interior, and the shell plane on a wall slab
    void owned_range(const Slab& sl, int& kb, int& ke) const {
        kb = sl.geom.kg0 + G_ - (sl.geom.wall_lo ? 1 : 0);
        ke = sl.geom.kg0 + G_ + nzl_ + (sl.geom.wall_hi ? 1 : 0);
    }
    // global planes [kb, ke) of buffer src of slab sl into dense (N+2)^2 planes at dst, on stream st
    void copy_planes_out(const Slab& sl, const T* src, hipStream_t st, int kb, int ke, T* dst) const {
        const size_t S = (size_t)N_ + 2;
        const int klb = kb - sl.geom.kg0;
        SF_REQUIRE(klb >= 0 && ke - sl.geom.kg0 <= nplanes_, "plane range outside slab");
        SF_HIP(hipMemcpy2DAsync(dst, S * sizeof(T), src + (size_t)klb * plane_ + (lead_ - 1), (size_t)px_ * sizeof(T),
                                S * sizeof(T), S * (size_t)(ke - kb), hipMemcpyDeviceToHost, st));
    }
    // Planes [kb, ke) of a field from / to a host array that holds exactly those planes: every slab takes the ones it
    // stores (upload: ghost planes included) / is the owner of (download). False: no slab has any of them.
    bool upload_range(int field, int kb, int ke, const T* host) {
        SF_HIP(hipSetDevice(device_));
        const size_t S = (size_t)N_ + 2;
        bool any = false;
        for (Slab& sl : slabs_) {
            T* dev = ensure(sl, field);
            const int b = std::max(std::max(kb, sl.geom.kg0), 0);
            const int e = std::min(std::min(ke, sl.geom.kg0 + nplanes_), N_ + 2);
            if (b >= e) continue;
            any = true;
            SF_HIP(hipMemcpy2DAsync(dev + (size_t)(b - sl.geom.kg0) * plane_ + (lead_ - 1), (size_t)px_ * sizeof(T),
                                    host + (size_t)(b - kb) * S * S, S * sizeof(T), S * sizeof(T), S * (size_t)(e - b),
                                    hipMemcpyHostToDevice, sl.cs));
        }
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.cs));
        return any;
    }
    bool download_range(int field, int kb, int ke, T* host) {
        SF_HIP(hipSetDevice(device_));
        const size_t S = (size_t)N_ + 2;
        bool any = false;
        for (Slab& sl : slabs_) {
            int ob, oe;
            owned_range(sl, ob, oe);
            const int b = std::max(kb, ob), e = std::min(ke, oe);
            if (b >= e) continue;
            any = true;
            copy_planes_out(sl, ensure(sl, field), sl.cs, b, e, host + (size_t)(b - kb) * S * S);
        }
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.cs));
        return any;
    }

    // 1-D banded grid of launch L for the one-vector-per-thread kernels: fills block, returns the map and block count.
    sfk::TileMap flat_map(const Launch& L, dim3& block, unsigned& nblocks) const {
        // these kernels take their i+-1 values by loads, so a row tile may have any width: one tile per row up
        // to 256 vectors (no idle lanes for N = 324, 408, ...), 64-lane tiles beyond
        const int nvec = ceil_div(N_, W);
        const int tx = nvec <= 256 ? nvec : 64;
        const int ty = std::max(1, 256 / tx);
        block = dim3(tx, ty, 1);
        sfk::TileMap m{};
        m.rows = 0;
        m.gx = ceil_div(nvec, tx);
        m.gy = ceil_div(N_, ty);
        m.nxcd = 8;
        m.band = (m.gy >= 16) ? ceil_div(m.gy, 8) : 0;
        m.ishell_mem = 1;
        m.ishell_write = 1;
        m.split = L.split;
        m.gap = L.gap;
        const long per_plane = m.band > 0 ? (long)m.nxcd * m.gx * m.band : (long)m.gx * m.gy;
        nblocks = (unsigned)(per_plane * (L.ke - L.kb));
        return m;
    }

    // Runs `launch(Launch)` over the interior planes of every slab. With P > 1 the two
    // slab-boundary planes go first, their completion is recorded, and the rest follows so that the
    // halo exchange issued by the caller overlaps the interior work.
    // Streams of a decomposed grid (P > 1). Per operator and slab:
    //   bs: boundary launch B (first / last G interior planes; needs the previous halo and everything issued so far)
    //   cs: interior launch I (needs the previous B and I, never a halo — its stencil stays inside the slab)
    //   hs: halo exchange of B's planes, concurrent with I
    // so a pair costs max(I, B + exchange) instead of B + max(I, exchange). Whole-field operators run on cs after
    // join(), which makes cs wait for the last B and the last halo.
    // ---- schedule trace (SF_TRACE_SCHEDULE=<file>) -------------------------------------------------------------
    // Every launch, exchange and stream-ordering call of the decomposed step is appended to <file> as one JSON line:
    //   {"t":"ctx", ...}                                   context geometry (first line of a context)
    //   {"t":"op","name":..,"slab":g,"stream":"cs|bs|hs","acc":[["r"|"w",buffer,lo,hi],...]}   plane ranges [lo,hi)
    //   {"t":"rec","slab":g,"stream":..,"ev":..}           hipEventRecord
    //   {"t":"wait","slab":g,"stream":..,"ev":..,"evslab":h}   hipStreamWaitEvent (on the event's latest record)
    //   {"t":"xchg","seq":n,"fields":[..],"G":G}           one halo exchange (sequence number: the same on every rank)
    // Reads carry the stencil reach of the kernel (an S-sweep launch reads x on S planes either side). tests/
    // schedule_check.py rebuilds the happens-before relation (stream order + event edges) and asserts that no two
    // accesses to overlapping planes of one buffer, one of them a write, are unordered — the write-after-read race of
    // round 2 (DESIGN §4 log) is such a pair. ",inject=trap" after the file name re-introduces that bug (growth S_j
    // instead of max(S_j, S_{j-1})) so the checker can be shown to catch it; results may then be wrong by design.
    struct Acc {
        const void* buf;
        bool write;
        int lo, hi;
    };
    void trace_open() {
        const char* t = std::getenv("SF_TRACE_SCHEDULE");
        if (!t || !*t) return;
        std::string path(t);
        const size_t c = path.find(',');
        if (c != std::string::npos) {
            inject_trap_bug_ = path.substr(c + 1) == "inject=trap";
            path.resize(c);
        }
        trace_ = std::fopen(path.c_str(), "a");
        if (!trace_) throw Failure{SF_ERR_INVALID, "SF_TRACE_SCHEDULE: cannot open " + path};
        std::fprintf(trace_, "{\"t\":\"ctx\",\"N\":%d,\"P\":%d,\"L\":%d,\"rank\":%d,\"G\":%d,\"nzl\":%d,\"np\":%d,\"trap\":%d,"
                             "\"hs_is_bs\":%d,\"inject\":%d}\n",
                     N_, P_, L_, rank_, G_, nzl_, nplanes_, trap_m_, slabs_[0].hs == slabs_[0].bs ? 1 : 0,
                     inject_trap_bug_ ? 1 : 0);
    }
    const char* sname(const Slab& sl, hipStream_t st) const { return st == sl.cs ? "cs" : (st == sl.bs ? "bs" : "hs"); }
    static const char* ename(hipEvent_t Slab::*e) {
        return e == &Slab::cs_mark ? "cs_mark" : (e == &Slab::boundary_done ? "boundary" : "halo");
    }
    int buf_id(const void* p) {
        auto it = buf_ids_.find(p);
        if (it == buf_ids_.end()) it = buf_ids_.emplace(p, (int)buf_ids_.size()).first;
        return it->second;
    }
    void ev_record(Slab& sl, hipEvent_t Slab::*e, hipStream_t st) {
        SF_HIP(hipEventRecord(sl.*e, st));
        if (trace_)
            std::fprintf(trace_, "{\"t\":\"rec\",\"slab\":%d,\"stream\":\"%s\",\"ev\":\"%s\"}\n", sl.gid, sname(sl, st), ename(e));
    }
    void st_wait(Slab& wsl, hipStream_t st, Slab& esl, hipEvent_t Slab::*e) {
        SF_HIP(hipStreamWaitEvent(st, esl.*e, 0));
        if (trace_)
            std::fprintf(trace_, "{\"t\":\"wait\",\"slab\":%d,\"stream\":\"%s\",\"ev\":\"%s\",\"evslab\":%d}\n", wsl.gid,
                         sname(wsl, st), ename(e), esl.gid);
    }
    void tr_op(const char* name, const Slab& sl, hipStream_t st, const std::vector<Acc>& acc) {
        if (!trace_) return;
        std::fprintf(trace_, "{\"t\":\"op\",\"name\":\"%s\",\"slab\":%d,\"stream\":\"%s\",\"acc\":[", name, sl.gid, sname(sl, st));
        bool first = true;
        for (const Acc& a : acc) {
            const int lo = std::max(a.lo, 0), hi = std::min(a.hi, nplanes_);
            if (lo >= hi) continue;
            std::fprintf(trace_, "%s[\"%s\",%d,%d,%d]", first ? "" : ",", a.write ? "w" : "r", buf_id(a.buf), lo, hi);
            first = false;
        }
        std::fprintf(trace_, "]}\n");
        std::fflush(trace_);
    }
    // whole-field operator on the compute stream
    void tr_whole(const char* name, const Slab& sl, std::initializer_list<const void*> reads,
                  std::initializer_list<const void*> writes) {
        if (!trace_) return;
        std::vector<Acc> acc;
        for (const void* r : reads) acc.push_back({r, false, 0, nplanes_});
        for (const void* w : writes) acc.push_back({w, true, 0, nplanes_});
        tr_op(name, sl, sl.cs, acc);
    }
    // planes [kb, ke) written by a launch, widened by the physical shell plane a wall slab's launch also writes
    void wr_range(const Slab& sl, int kb, int ke, int& lo, int& hi) const {
        lo = (sl.geom.wall_lo && kb == G_) ? kb - 1 : kb;
        hi = (sl.geom.wall_hi && ke == G_ + nzl_) ? ke + 1 : ke;
    }

    // ---- reductions (SPEC §10) ---------------------------------------------------------------------------------
    // rows of a plane padded to the next power of two: the width of the plane partial's halving fold
    int rows_pad() const {
        int n = 1;
        while (n < N_) n *= 2;
        return n;
    }
    void records_alloc() {
        SF_REQUIRE(rows_pad() <= 2048, "reductions take N <= 2048");
        const size_t nv = sfk::DIAG_NV;
        for (Slab& sl : slabs_) {
            if (!sl.red_rows) sl.red_rows = own_.dev<double>(nv * nzl_ * (size_t)rows_pad() * sizeof(double));
            if (!sl.red_planes) sl.red_planes = own_.dev<double>(nv * nzl_ * sizeof(double));
        }
        if (comm_ && !red_gather_) red_gather_ = own_.dev<double>(nv * N_ * sizeof(double));
        if (!red_host_) red_host_ = own_.pinned<double>(nv * N_ * sizeof(double));
    }
    unsigned row_blocks(const Level& h) const { return (unsigned)ceil_div((long)h.N * h.nzl, 4L); }
    // a slab's geometry on a level: its share of the level's planes, the wall flags of the slab
    sfk::Geom level_geom(const Slab& sl, const Level& h) const {
        sfk::Geom g = sl.geom;
        g.N = h.N, g.nzl = h.nzl, g.G = h.G, g.np = h.np, g.px = h.px, g.plane = h.plane;
        g.kg0 = sl.gid * h.nzl + 1 - h.G;
        return g;
    }
    // One row kernel (one wave per row, the nzl planes of a slab in one launch: SPEC §10, §11) on every slab's compute
    // stream, with its trace. args(sl): the kernel's argument after the geometry; acc(sl): its field accesses. RECORDS:
    // the kernel also takes, and writes, the slab's row records.
    // lv: the level whose rows the launch runs over (the multigrid kernels; row records only from the face codes of a
    // coarse level, which nothing reads).
    template <bool RECORDS = true, class K, class ArgsF, class AccF>
    void launch_rows(const char* name, K kernel, ArgsF args, AccF acc, const Level* lv = nullptr) {
        const Level& h = lv ? *lv : lv0_;
        for (Slab& sl : slabs_) {
            if constexpr (RECORDS)
                hipLaunchKernelGGL(kernel, dim3(row_blocks(h)), dim3(256), 0, sl.cs, lv ? level_geom(sl, h) : sl.geom, args(sl),
                                   sl.red_rows, rows_pad());
            else
                hipLaunchKernelGGL(kernel, dim3(row_blocks(h)), dim3(256), 0, sl.cs, lv ? level_geom(sl, h) : sl.geom, args(sl));
            SF_HIP(hipGetLastError());
            if (!trace_) continue;
            std::vector<Acc> a = acc(sl);
            if (RECORDS) a.push_back({sl.red_rows, true, 0, nplanes_});
            tr_op(name, sl, sl.cs, a);
        }
    }
    // Row records -> plane records -> host -> (all ranks' records) -> the fold over global k. Values below nsum are
    // sums, the next nmin minima, the rest maxima. Leaves every compute stream idle.
    void finish_records(int nv, int nsum, int nmin, double* out) {
        const int npad = rows_pad();
        const size_t per_slab = (size_t)nzl_ * nv;
        for (Slab& sl : slabs_) {
            hipLaunchKernelGGL(sfk::fold_rows_kernel, dim3(nzl_, nv), dim3(256), 0, sl.cs, sl.red_rows, sl.red_planes, N_,
                               npad, nsum, nmin);
            SF_HIP(hipGetLastError());
            tr_op("fold_rows", sl, sl.cs, {{sl.red_rows, false, 0, nplanes_}, {sl.red_planes, true, 0, nplanes_}});
            SF_HIP(hipMemcpyAsync(red_host_ + sl.gid * per_slab, sl.red_planes, per_slab * sizeof(double),
                                  hipMemcpyDeviceToHost, sl.cs));
            tr_op("records_out", sl, sl.cs, {{sl.red_planes, false, 0, nplanes_}});
        }
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.cs));
        if (comm_) {
            // the plane record is the unit that crosses ranks: every rank ends with all N of them and folds them itself
            Slab& s0 = slabs_[0];
            const size_t cnt = (size_t)L_ * per_slab, off = (size_t)rank_ * cnt;
            SF_HIP(hipMemcpyAsync(red_gather_ + off, red_host_ + off, cnt * sizeof(double), hipMemcpyHostToDevice, s0.cs));
            SF_NCCL(ncclGroupStart());
            SF_NCCL(ncclAllGather(red_gather_ + off, red_gather_, cnt, ncclDouble, comm_, s0.cs));
            SF_NCCL(ncclGroupEnd());
            ++rccl_groups_;
            tr_op("records_allgather", s0, s0.cs, {{red_gather_, false, 0, nplanes_}, {red_gather_, true, 0, nplanes_}});
            SF_HIP(hipMemcpyAsync(red_host_, red_gather_, (size_t)nranks_ * cnt * sizeof(double), hipMemcpyDeviceToHost,
                                  s0.cs));
            SF_HIP(hipStreamSynchronize(s0.cs));
        }
        // a loopback context stands for one rank of several and has nobody to gather from: its own planes only
        const bool own_only = nranks_ > 1 && !comm_;
        const int k0 = own_only ? rank_ * L_ * nzl_ : 0, k1 = own_only ? k0 + L_ * nzl_ : N_;
        for (int v = 0; v < nv; ++v) {
            const bool sum = v < nsum, mn = !sum && v < nsum + nmin;
            double t = sum ? 0.0 : (mn ? (double)INFINITY : -(double)INFINITY);
            for (int k = k0; k < k1; ++k) {
                const double x = red_host_[(size_t)k * nv + v];
                t = sum ? t + x : (mn ? (x < t ? x : t) : (x > t ? x : t));
            }
            out[v] = sum ? t : t + 0.0;  // a zero minimum / maximum is +0
        }
    }

    void join() {
        if (P_ == 1 || !pending_join_) return;
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            st_wait(sl, sl.cs, sl, &Slab::boundary_done);
            wait_neighbourhood(s, sl.cs, &Slab::halo_done);
        }
        pending_join_ = false;
    }

    // name, acc: the trace of the operator. acc(sl, a, b, lo, hi, out) appends its accesses over the planes [a, b) of
    // one launch; [lo, hi) is that range widened by the shell plane a wall slab's launch also writes (wr_range).
    // grow > 0 (lin_solve only): the boundary launch takes that many more planes per side than the last one did, so
    // this interior launch reads nothing a boundary launch wrote since the last resync and the compute stream needs no
    // cross-stream wait (see op_lin_solve).
    template <class AccF, class F>
    void for_planes(const char* name, AccF acc, F launch, int depth = 1, int grow = 0, bool interior_reads_ghosts = false) {
        // the exchange that follows ships G_ planes per side, so at least G_ planes per side must come out of
        // the boundary launch (whose completion the halo stream waits for), not out of the interior launch
        depth = std::max(depth, G_);
        const int kb = G_, ke = G_ + nzl_;
        auto emit = [&](Slab& sl, hipStream_t st, int a0, int a1, int b0 = 0, int b1 = 0) {
            if (!trace_) return;
            std::vector<Acc> out;
            int lo, hi;
            wr_range(sl, a0, a1, lo, hi);
            acc(sl, a0, a1, lo, hi, out);
            if (b1 > b0) {
                wr_range(sl, b0, b1, lo, hi);
                acc(sl, b0, b1, lo, hi, out);
            }
            tr_op(name, sl, st, out);
        };
        auto run = [&](Slab& sl, hipStream_t st, int a, int b) {
            launch(Launch{sl, st, a, b});
            emit(sl, st, a, b);
        };
        if (P_ == 1) {
            run(slabs_[0], slabs_[0].cs, kb, ke);
            SF_HIP(hipGetLastError());
            return;
        }
        const int extra = (nzl_ > 2 * (depth + grow) && sw_.split && !interior_reads_ghosts) ? grow : 0;
        const bool two_streams = nzl_ > 2 * depth && sw_.split && !interior_reads_ghosts;
        if (!two_streams) join();
        depth += extra;
        for (Slab& sl : slabs_) {
            if (!two_streams) {
                if (nzl_ <= 2 * depth) {
                    run(sl, sl.cs, kb, ke);
                    ev_record(sl, &Slab::boundary_done, sl.cs);
                } else {
                    run(sl, sl.cs, kb, kb + depth);
                    run(sl, sl.cs, ke - depth, ke);
                    ev_record(sl, &Slab::boundary_done, sl.cs);
                    run(sl, sl.cs, kb + depth, ke - depth);
                }
                continue;
            }
            // I of this operator reads what the previous B wrote (unless B has grown, see above); B reads everything
            // issued on cs so far
            if (extra == 0) st_wait(sl, sl.cs, sl, &Slab::boundary_done);
            ev_record(sl, &Slab::cs_mark, sl.cs);
            st_wait(sl, sl.bs, sl, &Slab::cs_mark);
            // ONE launch over the first and the last `depth` interior planes (split plane range)
            launch(Launch{sl, sl.bs, kb, kb + 2 * depth, depth, nzl_ - 2 * depth});
            emit(sl, sl.bs, kb, kb + depth, ke - depth, ke);
            ev_record(sl, &Slab::boundary_done, sl.bs);
            run(sl, sl.cs, kb + depth, ke - depth);
        }
        SF_HIP(hipGetLastError());
    }

    // Launch of an operator kernel kernel(geom, args, kb, ke, rest...) for L.
    template <class F, class Args, class... Rest>
    void launch_k(const Launch& L, F kernel, dim3 nblocks, dim3 block, const Args& args, Rest... rest) {
        hipLaunchKernelGGL(kernel, nblocks, block, 0, L.st, L.sl.geom, args, L.kb, L.ke, rest...);
    }

    // trace of one slab's share of a halo exchange on stream `st`: its low / high ghost planes are written from the last
    // / first interior planes of `lo` / `hi` (the neighbouring slab of this process; with a neighbour in another
    // process — or the loopback stand-in — the planes READ are this slab's own outgoing ones)
    template <int NF>
    void tr_halo(const char* name, Slab& sl, hipStream_t st, const int (&fields)[NF], Slab* lo, Slab* hi, bool lo_remote,
                 bool hi_remote, const Level& h) {
        if (!trace_) return;
        std::vector<Acc> acc;
        for (int f = 0; f < NF; ++f) {
            const T* mine = sl.field[fields[f]];
            if (lo) acc.push_back({lo->field[fields[f]], false, h.nzl, h.nzl + h.G});
            if (lo_remote) acc.push_back({mine, false, h.G, 2 * h.G});
            if (lo || lo_remote) acc.push_back({mine, true, 0, h.G});
            if (hi) acc.push_back({hi->field[fields[f]], false, h.G, 2 * h.G});
            if (hi_remote) acc.push_back({mine, false, h.nzl, h.nzl + h.G});
            if (hi || hi_remote) acc.push_back({mine, true, h.G + h.nzl, 2 * h.G + h.nzl});
        }
        tr_op(name, sl, st, acc);
    }
    template <int NF>
    void tr_xchg(const int (&fields)[NF], const Level& h) {
        if (!trace_) return;
        std::fprintf(trace_, "{\"t\":\"xchg\",\"seq\":%ld,\"G\":%d,\"fields\":[", xchg_seq_, h.G);
        for (int f = 0; f < NF; ++f) std::fprintf(trace_, "%s%d", f ? "," : "", fields[f]);
        std::fprintf(trace_, "]}\n");
    }

    // G_ planes per direction and field: the first / last G_ interior planes go to the neighbour's ghost planes.
    // Offsets in elements from the start of a field.
    struct HaloPlanes {
        size_t count, send_lo, send_hi, recv_lo, recv_hi;
    };
    HaloPlanes halo_planes(const Level& h) const {
        return {(size_t)h.G * h.plane, (size_t)h.G * h.plane, (size_t)h.nzl * h.plane, 0, (size_t)(h.G + h.nzl) * h.plane};
    }
    // stream st of local slab s waits for event e of that slab and of its neighbours in this process
    void wait_neighbourhood(int s, hipStream_t st, hipEvent_t Slab::*e) {
        Slab& sl = slabs_[s];
        st_wait(sl, st, sl, e);
        if (s > 0) st_wait(sl, st, slabs_[s - 1], e);
        if (s < L_ - 1) st_wait(sl, st, slabs_[s + 1], e);
    }
    // Consumers of an exchange: the next boundary launch reads my ghosts, and neighbours that pulled from my planes
    // must be done before I overwrite them two sweeps later. The compute stream only waits when it runs a
    // whole-field operator (join()).
    void consumers_wait_halo() {
        for (int s = 0; s < L_; ++s) wait_neighbourhood(s, slabs_[s].bs, &Slab::halo_done);
        pending_join_ = true;
    }
    // One copy kernel on sl's halo stream for all fields and both sides: sl's low ghost planes from slab `lo`, its high
    // ghost planes from slab `hi` (null: that side is not copied). A neighbour gives the planes next to sl; sl itself
    // (the loopback stand-in) the planes it would send that way.
    template <int NF>
    void halo_copy(Slab& sl, const int (&fields)[NF], const Slab* lo, const Slab* hi, const Level& lv) {
        const HaloPlanes h = halo_planes(lv);
        sfk::HaloCopyArgs H;
        H.nseg = 0;
        H.n16 = (long)(h.count * sizeof(T) / 16);
        for (int f = 0; f < NF; ++f) {
            T* mine = sl.field[fields[f]];
            if (lo) {
                H.src[H.nseg] = reinterpret_cast<const float4*>(lo->field[fields[f]] + (lo == &sl ? h.send_lo : h.send_hi));
                H.dst[H.nseg++] = reinterpret_cast<float4*>(mine + h.recv_lo);
            }
            if (hi) {
                H.src[H.nseg] = reinterpret_cast<const float4*>(hi->field[fields[f]] + (hi == &sl ? h.send_hi : h.send_lo));
                H.dst[H.nseg++] = reinterpret_cast<float4*>(mine + h.recv_hi);
            }
        }
        const unsigned gx = (unsigned)std::max(1L, std::min((H.n16 + 255) / 256, 512L));
        hipLaunchKernelGGL(sfk::halo_copy_kernel, dim3(gx, H.nseg), dim3(256), 0, sl.hs, H);
        SF_HIP(hipGetLastError());
    }

    // Halo exchange of NF fields: first / last interior plane -> neighbour's ghost plane.
    // Must follow for_planes (uses boundary_done). Compute streams wait on the result.
    // lv: the level the fields live on (a coarse level of the multigrid hierarchy ships its one ghost plane).
    template <int NF>
    void exchange(const int (&fields)[NF], const Level* lvp = nullptr) {
        if (P_ == 1) return;
        const Level& lv = lvp ? *lvp : lv0_;
        tr_xchg<NF>(fields, lv);
        ++xchg_seq_;
        if (rccl_self_) {
            exchange_rccl_self<NF>(fields, lv);
            return;
        }
        const HaloPlanes h = halo_planes(lv);
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            wait_neighbourhood(s, sl.hs, &Slab::boundary_done);
            // pull from neighbours that live in this process
            Slab* lo = s > 0 ? &slabs_[s - 1] : nullptr;
            Slab* hi = s < L_ - 1 ? &slabs_[s + 1] : nullptr;
            if (lo || hi) {
                halo_copy<NF>(sl, fields, lo, hi, lv);
                tr_halo<NF>("halo_pull", sl, sl.hs, fields, lo, hi, false, false, lv);
            }
            // neighbours in other processes: grouped send/recv over RCCL (xGMI point-to-point)
            const bool lo_remote = sl.gid > 0 && !lo, hi_remote = sl.gid < P_ - 1 && !hi;
            if ((lo_remote || hi_remote) && loopback_) {
                // SF_FLAG_LOOPBACK_HALO: same bytes, same stream, same dependencies, but from this slab's own planes
                halo_copy<NF>(sl, fields, lo_remote ? &sl : nullptr, hi_remote ? &sl : nullptr, lv);
                tr_halo<NF>("halo_loopback", sl, sl.hs, fields, nullptr, nullptr, lo_remote, hi_remote, lv);
            } else if (lo_remote || hi_remote) {
                const ncclDataType_t dt = sizeof(T) == 4 ? ncclFloat : ncclDouble;
                SF_NCCL(ncclGroupStart());
                for (int f = 0; f < NF; ++f) {
                    T* mine = sl.field[fields[f]];
                    if (lo_remote) {
                        SF_NCCL(ncclSend(mine + h.send_lo, h.count, dt, rank_ - 1, comm_, sl.hs));
                        SF_NCCL(ncclRecv(mine + h.recv_lo, h.count, dt, rank_ - 1, comm_, sl.hs));
                    }
                    if (hi_remote) {
                        SF_NCCL(ncclSend(mine + h.send_hi, h.count, dt, rank_ + 1, comm_, sl.hs));
                        SF_NCCL(ncclRecv(mine + h.recv_hi, h.count, dt, rank_ + 1, comm_, sl.hs));
                    }
                }
                SF_NCCL(ncclGroupEnd());
                ++rccl_groups_;
                tr_halo<NF>("halo_rccl", sl, sl.hs, fields, nullptr, nullptr, lo_remote, hi_remote, lv);
            }
            ev_record(sl, &Slab::halo_done, sl.hs);
        }
        consumers_wait_halo();
    }

    // SF_FLAG_RCCL_SELF: the ghost planes of the L logical slabs travel through a real RCCL communicator (one rank,
    // this GPU) as grouped ncclSend / ncclRecv to self — the calls, datatype, counts, buffer offsets, stream choice
    // (each slab's halo stream, which is its boundary stream under SF_HALO_STREAM=2 as in production) and the
    // system-scope halo_done event of the multi-process branch of exchange(). RCCL matches the sends and the receives
    // of one peer in issue order, so every transfer is issued as the pair (send from the owner's planes, receive into
    // the neighbour's ghost planes); one group spans all slabs because a send to self needs its receive in the same
    // group.
    template <int NF>
    void exchange_rccl_self(const int (&fields)[NF], const Level& lv) {
        const ncclDataType_t dt = sizeof(T) == 4 ? ncclFloat : ncclDouble;
        const HaloPlanes h = halo_planes(lv);
        for (int s = 0; s < L_; ++s) wait_neighbourhood(s, slabs_[s].hs, &Slab::boundary_done);
        SF_NCCL(ncclGroupStart());
        for (int s = 0; s + 1 < L_; ++s) {
            Slab& lo = slabs_[s];
            Slab& hi = slabs_[s + 1];
            for (int f = 0; f < NF; ++f) {
                T* a = lo.field[fields[f]];
                T* b = hi.field[fields[f]];
                // upward: last interior planes of slab s -> low ghost planes of slab s+1
                SF_NCCL(ncclSend(a + h.send_hi, h.count, dt, 0, comm_, lo.hs));
                SF_NCCL(ncclRecv(b + h.recv_lo, h.count, dt, 0, comm_, hi.hs));
                // downward: first interior planes of slab s+1 -> high ghost planes of slab s
                SF_NCCL(ncclSend(b + h.send_lo, h.count, dt, 0, comm_, hi.hs));
                SF_NCCL(ncclRecv(a + h.recv_hi, h.count, dt, 0, comm_, lo.hs));
            }
        }
        SF_NCCL(ncclGroupEnd());
        ++rccl_groups_;
        for (int s = 0; s < L_; ++s)
            tr_halo<NF>("halo_rccl_self", slabs_[s], slabs_[s].hs, fields, s > 0 ? &slabs_[s - 1] : nullptr,
                        s < L_ - 1 ? &slabs_[s + 1] : nullptr, false, false, lv);
        for (int s = 0; s < L_; ++s) ev_record(slabs_[s], &Slab::halo_done, slabs_[s].hs);
        consumers_wait_halo();
    }
    // after whole-field kernels wrote field x on every slab's compute stream: its ghost planes
    void publish_from_cs(int x, const Level* lv = nullptr) {
        if (P_ == 1) return;
        for (Slab& sl : slabs_) ev_record(sl, &Slab::boundary_done, sl.cs);
        const int fs[1] = {x};
        exchange<1>(fs, lv);
    }

    template <int NF>
    void op_add_source(const int (&x)[NF], const int (&s)[NF]) {
        join();
        const long nvec = field_elems_ / W;
        for (Slab& sl : slabs_) {
            sfk::AddSourceArgs<T, NF> A;
            for (int f = 0; f < NF; ++f) {
                A.x[f] = ensure(sl, x[f]);
                A.s[f] = ensure(sl, s[f]);
            }
            A.dt = dt_;
            A.nvec = nvec;
            hipLaunchKernelGGL((sfk::add_source_kernel<T, NF>), dim3((unsigned)ceil_div(nvec, 256L)), dim3(256), 0, sl.cs, A);
            for (int f = 0; f < NF; ++f) tr_whole("add_source", sl, {A.x[f], A.s[f]}, {A.x[f]});
        }
        SF_HIP(hipGetLastError());
        // ghosts of x and s were current, so the ghosts of the result are current: no exchange
    }

    template <int NF>
    void op_add_source_bound(const int (&x)[NF], const int (&s_copy)[NF], const int (&src)[NF]) {
        join();
        const long nvec = field_elems_ / W;
        for (Slab& sl : slabs_) {
            sfk::AddSourceBoundArgs<T, NF> A;
            for (int f = 0; f < NF; ++f) {
                A.x[f] = ensure(sl, x[f]);
                A.s_copy[f] = ensure(sl, s_copy[f]);
                A.src[f] = ensure(sl, src[f]);
            }
            A.dt = dt_;
            A.nvec = nvec;
            hipLaunchKernelGGL((sfk::add_source_bound_kernel<T, NF>), dim3((unsigned)ceil_div(nvec, 256L)), dim3(256), 0, sl.cs, A);
            for (int f = 0; f < NF; ++f) tr_whole("add_source_bound", sl, {A.x[f], A.src[f]}, {A.x[f], A.s_copy[f]});
        }
        SF_HIP(hipGetLastError());
    }

    // Single-sweep launcher (flat register-blocked kernel with XCD bands): odd last sweeps, grids the fused kernels do
    // not take. SF_NT: 0 never / 1 always / 2 auto non-temporal stores. SF_ISHELL: 0 = always read+write the i-shell,
    // 1 = recompute it in intermediate sweeps (default).
    template <int NF, bool NT, int RJ, int RK>
    void launch_rb(const Launch& L, const sfk::JacobiArgs<T, NF>& A, bool first, bool last) {
        const int nvec = ceil_div(N_, W);
        int tx = 1;
        while (tx < nvec && tx < 64) tx <<= 1;
        const int ty = 256 / tx;
        sfk::TileMap m{};
        m.gx = ceil_div(nvec, tx);
        m.gy = ceil_div(N_, ty * RJ);
        m.nxcd = 8;
        m.band = (m.gy >= 16) ? ceil_div(m.gy, 8) : 0;
        m.ishell_mem = (!ishell_skip_ || first) ? 1 : 0;
        m.ishell_write = (!ishell_skip_ || last) ? 1 : 0;
        m.split = L.split;
        m.gap = L.gap;
        const long per_plane = m.band > 0 ? (long)m.nxcd * m.gx * m.band : (long)m.gx * m.gy;
        const long nblocks = per_plane * ceil_div(L.ke - L.kb, RK) * NF;
        launch_k(L, sfk::jacobi_rb_kernel<T, NF, NT, RJ, RK>, dim3((unsigned)nblocks), dim3(tx, ty), A, m);
    }

    template <int NF, bool NT>
    void launch_rb_shape(const Launch& L, const sfk::JacobiArgs<T, NF>& A, bool first, bool last) {
        // measured (512^3 / 256^3 fp32): 2x2 blocks win once the sweep streams from HBM (286 vs 309 us),
        // 1x1 wins while x, x0, x' sit in the Infinity Cache (30.8 vs 34.0 us)
        const bool blocks = NT && !(L.is_split() && L.split % 2 != 0);  // a plane block must not straddle the split
        if (blocks)
            launch_rb<NF, NT, 2, 2>(L, A, first, last);
        else
            launch_rb<NF, NT, 1, 1>(L, A, first, last);
    }

    // SF_NT: non-temporal stores never (0), always (1), or (2) once x, x0 and x' of the nf fields of a launch no longer
    // fit the 256 MiB Infinity Cache
    bool nt_stores(int nf) const {
        return sw_.nt == 1 || (sw_.nt == 2 && (size_t)field_elems_ * sizeof(T) * 3 * nf > ((size_t)384 << 20));
    }
    // f(std::bool_constant<nt_stores(nf)>): the store form of a launch of nf fields as a compile-time constant
    template <class F>
    void with_nt(int nf, F f) const {
        if (nt_stores(nf))
            f(std::true_type{});
        else
            f(std::false_type{});
    }
    // bytes of x, x0 and x' of one field of a solve, and whether a working set fits the 256 MiB Infinity Cache
    double solve_bytes() const { return 3.0 * (double)(N_ + 2) * (N_ + 2) * nplanes_ * sizeof(T); }
    static bool fits_ic(double bytes) { return bytes <= 0.9 * 256.0 * 1048576.0; }

    // Two fused sweeps (temporal blocking). Usable when a row fits one workgroup, N is a multiple of the
    // vector width and the grid is not decomposed (a second ghost plane would be needed).
    // (measured against single sweeps: +20 % at 512^3, +35 % at 256^3, +11 % at 1024^3 fp32, +15 % at 512^3 fp64)
    bool can_fuse2() const {
        return sw_.fuse2 && (P_ == 1 || G_ >= 2) && N_ % W == 0 && N_ / W <= fuse_maxvec_;
    }

    // field f of A as the arguments of a one-field launch
    template <int NF>
    static sfk::JacobiArgs<T, 1> field_args(const sfk::JacobiArgs<T, NF>& A, int f) {
        sfk::JacobiArgs<T, 1> B;
        B.x[0] = A.x[f];
        B.x0[0] = A.x0[f];
        B.xn[0] = A.xn[f];
        B.x0out[0] = A.x0out[f];
        B.b[0] = A.b[f];
        B.a = A.a;
        B.inv = A.inv;
        B.dt = A.dt;
        return B;
    }

    // x_zero: the iterate is zero (implicit-zero first pair of project's lin_solve)
    template <int NF, bool NT, int RJ, int RK, bool SRC = false>
    void launch_fused2(const Launch& L, const sfk::JacobiArgs<T, NF>& A, bool first, bool last, bool x_zero) {
        const int nvec = N_ / W;
        sfk::TileMap m{};
        // row strips per 256-thread workgroup: packed densely (strip = nvec lanes; rows then start anywhere inside a
        // wave and both ends of most waves are seams -> LDS hand-over of x) or aligned to wave boundaries (strip
        // = multiple of 64; idle lanes, but one seam per wave at most). Aligned wins unless it idles >10 % more lanes.
        const int aligned = ceil_div(nvec, 64) * 64;
        const double eff_dense = (double)((256 / nvec) * nvec), eff_aligned = (double)((256 / aligned) * nvec);
        m.strip = (nvec % 64 == 0 || 64 % nvec == 0 || eff_aligned >= 0.9 * eff_dense) ? std::max(aligned, nvec) : nvec;
        if (64 % nvec == 0) m.strip = nvec;  // narrow rows: several whole rows per wave, never a seam
        m.rows = std::max(1, 256 / m.strip);
        m.gx = 1;
        m.gy = ceil_div(N_, m.rows * RJ);
        m.nxcd = 8;
        m.band = (m.gy >= 16) ? ceil_div(m.gy, 8) : 0;
        m.ishell_mem = (!ishell_skip_ || first) ? 1 : 0;
        m.ishell_write = (!ishell_skip_ || last) ? 1 : 0;
        m.split = L.split;
        m.gap = L.gap;
        // rows that neither fill whole waves nor divide one: the seam-free overlapped mapping (SF_OVL: 0 never,
        // 1 for such rows (default), 2 for every width)
        // ... and rows wider than two waves, where it also beats one row strip per workgroup (1024^3 fp32: 2026 vs
        // 1986 us/sweep; the single-sweep kernel: 2207)
        // (a row strip must fit the 256 threads of a workgroup: beyond that only the overlapped mapping exists)
        const bool ovl = sw_.ovl == 2 || (sw_.ovl == 1 && ((nvec % 64 != 0 && 64 % nvec != 0) || nvec > 128)) ||
                         nvec > 256;
        if (ovl) {
            const int items = ceil_div(N_, RJ) * nvec;
            m.gy = ceil_div(ceil_div(items, sfk::SF_OVL_OUT), 4);
            m.band = (m.gy >= 16) ? ceil_div(m.gy, 8) : 0;
        }
        // warm-up loads (see TileMap::pf_dz): about 32 workgroups ahead on the same XCD (measured best at 256^3 and
        // 512^3), expressed in plane blocks at the same j position
        // Automatic mode: only where the data comes from HBM (x, x0, x' of the launch's fields exceed the Infinity
        // Cache: a resident working set gains nothing, 256^3) and only where a plane block is a fine enough unit of
        // distance (<= 48 workgroups per XCD and plane block) and rows are at most 128 vectors wide: with rows of 256
        // vectors the early lines evict the j / k reuse from the 4 MB L2 (1024^3 fp32 ran 8 % slower, 512^3 fp64 5-15 %).
        {
            const int per_xcd_round = m.band > 0 ? m.band : m.gy;
            if (per_xcd_round <= 48 && nvec <= 128 && !fits_ic(NF * solve_bytes()))
                m.pf_dz = std::max(1, (32 + per_xcd_round / 2) / std::max(1, per_xcd_round));
            else
                m.pf_dz = 0;
        }
        m.strip_shift = (m.strip & (m.strip - 1)) == 0 ? __builtin_ctz((unsigned)m.strip) : -1;
        m.nvec_magic = nvec > 1 ? 0xFFFFFFFFu / (unsigned)nvec + 1u : 0u;
        const dim3 nb(m.band > 0 ? (unsigned)m.nxcd : (unsigned)m.gy, m.band > 0 ? (unsigned)m.band : 1u,
                      (unsigned)(ceil_div(L.ke - L.kb, RK) * NF));
        const bool xlds = m.strip % 64 != 0 && 64 % m.strip != 0;
        if constexpr (!SRC) {
            if (NF == 1 && x_zero) {
                if (ovl)
                    launch_k(L, sfk::jacobi2_kernel<T, 1, NT, RJ, RK, false, true, true>, nb, 256u, field_args(A, 0), m);
                else if (xlds)
                    launch_k(L, sfk::jacobi2_kernel<T, 1, NT, RJ, RK, true, true>, nb, 256u, field_args(A, 0), m);
                else
                    launch_k(L, sfk::jacobi2_kernel<T, 1, NT, RJ, RK, false, true>, nb, 256u, field_args(A, 0), m);
                return;
            }
        }
        if (ovl)
            launch_k(L, sfk::jacobi2_kernel<T, NF, NT, RJ, RK, false, false, true, SRC>, nb, 256u, A, m);
        else if (xlds)
            launch_k(L, sfk::jacobi2_kernel<T, NF, NT, RJ, RK, true, false, false, SRC>, nb, 256u, A, m);
        else
            launch_k(L, sfk::jacobi2_kernel<T, NF, NT, RJ, RK, false, false, false, SRC>, nb, 256u, A, m);
    }

    // Does the marching kernel (sfk::jacobi_sk_kernel; SF_MARCH=0 switches it off) fit a launch of `planes` planes of
    // this grid? The one place the size thresholds are compared. Small grids do not fill the chip with workgroups of
    // 32-48 rows (128^3: 9.0 vs 4.3 us/sweep; the crossover: Switches::march_min_cells).
    bool march_fits(int planes) const {
        return sw_.march != 0 && planes >= sw_.march_minp && (long)N_ * N_ * planes >= sw_.march_min_cells;
    }
    // ... and may it run there? It leaves the i-shell implicit between passes: with SF_ISHELL=0 — every pass reads it
    // from memory — it must not run at all, on one slab or many. (Round 2 checked that for P_ == 1 only, and a
    // decomposed solve mixed marching passes with pair passes that read a stale i-shell.)
    bool march_takes(int planes) const { return ishell_skip_ && march_fits(planes); }
    // S sweeps per pass on a decomposed grid need S ghost planes, the two-stream schedule, and an interior launch
    // [max(S, G) + extra, ...) (for_planes; extra: the growth of the boundary launch) the marching kernel takes (the
    // boundary launch always goes through it: there is no other kernel of that depth)
    bool march_takes_slab(int S, int extra) const {
        return G_ >= S && sw_.split && march_takes(nzl_ - 2 * (std::max(S, G_) + extra));
    }
    // an S-sweep marching pass of a solve on this context
    bool march_pass(int S, int extra = 0) const { return P_ == 1 ? march_takes(nzl_) : march_takes_slab(S, extra); }

    int sk_chunks(int ncb, int np, int S) const {
        const int max_chunks = std::max(1, np / 8);
        double best = -1;
        int nchunk = 1;
        for (int c = 1; c <= max_chunks; ++c) {
            const int kc = ceil_div(np, c);
            const long total = (long)ncb * ceil_div(np, kc);
            // (workgroups are dealt to the eight XCDs in turn; an XCD runs one per CU at a time)
            const double tm = (double)ceil_div(ceil_div(total, 8L), (long)std::max(1, num_cu_ / 8)) * (kc + 2 * S - 2 + 2);
            if (best < 0 || tm < best * 0.999) {
                best = tm;
                nchunk = c;
            }
        }
        return nchunk;
    }
    // Tile of the four-sweep launches (rows per wave x waves stacked in j; the lane vector is 8 bytes in both types).
    // fp32: 2 x 16 — four waves per SIMD at <= 128 registers: a march step is bound by each wave's serial instruction
    // stream (tools/sk_probe.hip -DSF_SK_DIAG=4: 88 % of its time with every load and store removed), so 16 thin waves
    // beat 8 waves of four rows (256^3: 62 -> 59 us per pass, 512^3: 441 -> 392, same 32-row tile and bytes).
    // fp64: 5 x 8 — half the cells per lane, twice the bytes per cell: there the 40-row tile (32 rows stored instead
    // of 24 of 32) is worth more than the waves (512^3 K = 40 step: 50.5 against 56.4 ms).
    // First passes over caller data (FIRST = 1, 2) hold a ring of shell cells and the right-hand side on top and
    // spill at 128 registers: 4 x 8 in both types.
    static constexpr int SK4_TJ = sizeof(T) == 4 ? 2 : 5, SK4_NW = sizeof(T) == 4 ? 16 : 8;
    static constexpr int SK4F_TJ = 4, SK4F_NW = 8;
    template <bool NT, int S, int TJ, int NW, int FIRST = 0, int NF = 1>
    void launch_sk_cfg(const Launch& L, const sfk::JacobiArgs<T, NF>& A, bool last) {
        constexpr int WL = W / 2;  // 8 bytes per lane
        constexpr int V = NW * TJ - 2 * S, P = 64 - 2 * ((S + WL - 1) / WL);
        const int nvec = N_ / WL;
        sfk::SkMap m{};
        m.njb = ceil_div(N_, V);
        const long items = (long)m.njb * nvec;
        m.ncb = (int)ceil_div(items, (long)P);
        m.band = ceil_div(m.ncb, 8);
        m.nvec_magic = nvec > 1 ? 0xFFFFFFFFu / (unsigned)nvec + 1u : 0u;
        const int np = L.ke - L.kb;
        int nchunk;
        if (L.is_split()) {
            // boundary launch of a decomposed grid: the first and the last `split` interior planes as two chunks
            nchunk = 2;
            m.gap = L.gap;
        } else {
            // One workgroup per CU at a time (LDS, registers): time ~ (workgroups per CU, rounded up) x (steps per
            // chunk: kc + 2S-2, plus start-up).
            nchunk = sk_chunks(m.ncb * NF, np, S);  // (NF fields in one grid: NF times the column blocks)
        }
        m.kc = L.is_split() ? L.split : ceil_div(np, nchunk);
        nchunk = ceil_div(np, m.kc);
        dim3 nb(8u, (unsigned)m.band, (unsigned)(nchunk * NF));
        if constexpr (FIRST != 0) {  // a first pass is never the last one (sk_first_ok)
            launch_k(L, sfk::jacobi_sk_kernel<T, NF, WL, NT, S, TJ, NW, false, FIRST>, nb, 64u * NW, A, m);
        } else if constexpr (NF > 1) {  // (fields in one grid: plain passes only, launch_sk)
            launch_k(L, sfk::jacobi_sk_kernel<T, NF, WL, NT, S, TJ, NW, false>, nb, 64u * NW, A, m);
        } else {
            if (last)
                launch_k(L, sfk::jacobi_sk_kernel<T, 1, WL, NT, S, TJ, NW, true>, nb, 64u * NW, A, m);
            else
                launch_k(L, sfk::jacobi_sk_kernel<T, 1, WL, NT, S, TJ, NW, false>, nb, 64u * NW, A, m);
        }
    }

    // What the first pass of a solve takes as its iterate; the values are the FIRST argument of sfk::jacobi_sk_kernel
    // (sfk::SkFirst). NONE: not a first pass — the iterate has been swept before and its i-shell is implicit.
    enum class First : int { NONE = 0, CALLER = 1, SOURCE = 2, ZERO = 3 };  // caller data / folded add_source / zero

    // One pass of a solve as plan_solve lays it out: `sweeps` fused sweeps per launch, then one exchange.
    struct Pass {
        int sweeps;        // 1 .. 4
        int depth, extra;  // for_planes: planes per side of the boundary launch (before max(.., G)), trapezoid growth
        First first;
        bool last;         // the pass that writes the i-shell
        bool batch;        // its marching launches take all fields of the solve as one grid (batch_march)
        const char* name;  // trace op
    };

    // First pass of a solve through the marching kernel (four sweeps). One launch per field, or one for all NF of a
    // folded-source pass in a batched solve (batch).
    template <int NF>
    void launch_sk_first(const Launch& L, const sfk::JacobiArgs<T, NF>& A, First first, bool batch) {
        // (tiles: SK4F_* for the passes that read the caller's i-shell, SK4_* for the zero-iterate pass, see above)
        with_nt(NF, [&](auto nt) {
            constexpr bool NT = decltype(nt)::value;
            if constexpr (NF > 1) {
                if (first == First::SOURCE && batch) {
                    launch_sk_cfg<NT, 4, SK4F_TJ, SK4F_NW, int(First::SOURCE), NF>(L, A, false);
                    return;
                }
            }
            for (int f = 0; f < NF; ++f) {
                const sfk::JacobiArgs<T, 1> B = field_args(A, f);
                if (first == First::CALLER)
                    launch_sk_cfg<NT, 4, SK4F_TJ, SK4F_NW, int(First::CALLER)>(L, B, false);
                else if (first == First::SOURCE)
                    launch_sk_cfg<NT, 4, SK4F_TJ, SK4F_NW, int(First::SOURCE)>(L, B, false);
                else
                    launch_sk_cfg<NT, 4, SK4_TJ, SK4_NW, int(First::ZERO)>(L, B, false);
            }
        });
    }
    // May the FIRST pass of a K-sweep solve go through the marching kernel? Four-sweep launches enabled, a grid the
    // kernel takes (slabs: four ghost planes and an interior launch it takes), and sweeps left over afterwards (no
    // i-shell-writing variant of a first pass).
    bool sk_first_ok(int K) const { return sw_.sk_first && sw_.sk_s >= 4 && can_fuse2() && K >= 7 && march_pass(4); }

    // The NF fields of a batched solve (u, v, w of a diffusion) as ONE marching grid on an undecomposed slab: NF times
    // the column blocks let the launch fill the chip with NF times fewer, longer chunks — a chunk pays 2(S-1) warm-up
    // planes whatever its length (256^3: 3 chunks of 86 planes instead of 10 of 26 per field: 92 instead of 96 steps per
    // workgroup; plain pass 51.3 against 53.3 us per field, folded-source first pass 74 against 86). Only on one
    // undecomposed slab (P_ == 1), so never in a split boundary launch.
    // ... which the solve only asks for when every pass is a four-sweep marching launch (K a multiple of four on a
    // grid the kernel takes): a pair-kernel pass over three fields at once would leave the Infinity Cache. And only
    // where it was measured to pay (same-box A/B of the full fp32 K = 20 step, ms, fields apart / in one grid; `one` =
    // x + x0 + x' of one field): 160^3 (52 MB) 0.846 / 0.881; 192^3 (89 MB) 1.666 / 1.506; 208^3 (113 MB) 1.399 / 1.281;
    // 224^3 (141 MB) 1.960 / 2.069 — one field still fits the 256 MiB Infinity Cache there, three do not —; 256^3 (201 MB)
    // 2.17 / 2.09; 320^3 3.95 / 3.92; 384^3 6.59 / 6.54; 512^3 K = 40 25.64 / 25.35; 1024^3 121.8 / 123.5 and 512^3 fp64
    // 49.6 / 49.8 (chunks are long anyway); fp64: 144^3 (76 MB) 1.579 / 1.409; 176^3 (137 MB) 2.048 / 2.162; 192^3
    // (178 MB) 2.662 / 2.646; 256^3 (403 MB) 4.60 / 4.32; 320^3 7.89 / 7.75. Hence two windows in bytes, whatever the
    // precision: 75..125 MB and 170 MB..2 GB.
    // K: the sweeps still to run; continued: a first pass (folded source) has run already.
    bool batch_march(int K, bool continued) const {
        if (!(P_ == 1 && split_fields_ != 2 && K % 4 == 0 && K >= 4 && sw_.sk_first && sw_.sk_s >= 4 && can_fuse2() &&
              march_takes(nzl_)))
            return false;
        const double mb = solve_bytes() / 1048576.0;
        if (split_fields_ == 1 && !((mb >= 75.0 && mb <= 125.0) || (mb >= 170.0 && mb <= 2048.0))) return false;
        return continued || K >= 8;
    }
    // Solve the NF fields of a solve one after the other? x, x0 and x' of ONE field fit the 256 MiB Infinity Cache where
    // those of NF fields together do not: every pair after the first then stays out of HBM (256^3 fp32: 3 x 50.8 us
    // against 175.9 us per pair of three fields). Independent fields: same results.
    bool solve_apart(int K) const {
        return split_fields_ == 2 || (split_fields_ == 1 && fits_ic(solve_bytes()) && !batch_march(K, false));
    }

    // S sweeps of the marching kernel on an iterate swept before. batch: as in Pass.
    template <int NF, int S>
    void launch_sk(const Launch& L, const sfk::JacobiArgs<T, NF>& A, bool last, bool batch) {
        SF_REQUIRE(ishell_skip_ && sw_.march != 0, "internal: marching launch while SF_ISHELL=0 / SF_MARCH=0");
        // Tile: SK4_* at S = 4 (above); six rows x eight waves at S <= 3. Four levels hold 17 planes of rows per
        // lane (x 3, x0 5, three intermediate levels x 3). (A spill in the wall workgroups alone doubles a launch
        // at 256^3, where every workgroup runs at once and the slowest one is the launch.)
        constexpr int TJ0 = S == 4 ? SK4_TJ : 6, NW0 = S == 4 ? SK4_NW : 8;
        with_nt(NF, [&](auto nt) {
            constexpr bool NT = decltype(nt)::value;
            if constexpr (NF > 1 && S == 4) {
                if (!last && batch) {
                    launch_sk_cfg<NT, S, TJ0, NW0, 0, NF>(L, A, false);
                    return;
                }
            }
            for (int f = 0; f < NF; ++f)  // one launch per field (fields are independent)
                launch_sk_cfg<NT, S, TJ0, NW0>(L, field_args(A, f), last);
        });
    }

    // The launch of pass p of a solve on the plane range L: the whole choice of kernel form.
    template <int NF>
    void launch_pass(const Launch& L, const sfk::JacobiArgs<T, NF>& A, const Pass& p) {
        const bool first = p.first != First::NONE;
        const int np = L.ke - L.kb;
        if (p.sweeps >= 3) {  // the marching kernel (pass_sweeps has asked march_pass)
            if (first)
                launch_sk_first<NF>(L, A, p.first, p.batch);
            else if (p.sweeps == 4)
                launch_sk<NF, 4>(L, A, p.last, p.batch);
            else
                launch_sk<NF, 3>(L, A, p.last, p.batch);
        } else if (p.sweeps == 2 && !first && !L.is_split() && march_takes(np) && (long)N_ * N_ * np >= sk2_min_cells_) {
            // two-sweep launches — slab interiors with two ghost planes, remainders — go through the marching kernel
            // on large grids only: at 256^3 the register-blocked pair kernel takes 49 us, the marching kernel 67; at
            // 512^3 437 against 365. Never a first pass (iterate in memory, zero or a source) or a split boundary launch.
            launch_sk<NF, 2>(L, A, p.last, false);
        } else if (p.sweeps == 2) {
            // 2x2 output vectors per thread: measured best of 1x1, 2x1, 1x2, 2x2, 4x2 (4x2 spills)
            with_nt(NF, [&](auto nt) {
                if (p.first == First::SOURCE)
                    launch_fused2<NF, decltype(nt)::value, 2, 2, true>(L, A, true, p.last, false);
                else
                    launch_fused2<NF, decltype(nt)::value, 2, 2>(L, A, first, p.last, p.first == First::ZERO);
            });
        } else {
            with_nt(NF, [&](auto nt) { launch_rb_shape<NF, decltype(nt)::value>(L, A, first, p.last); });
        }
    }

    // Sweeps fused into the pass that starts at iteration `it` of a K-sweep solve: 4 or 3 where the marching kernel
    // takes it — a first pass (iterate = caller data, zero or a source) only as four sweeps under sk_first_ok; remainders
    // of 5 and 6 go as 3 + 2 and 3 + 3; a remainder of 4 without four-sweep launches as 2 + 2 — else 2 where pairs
    // can be fused, else 1. extra: the growth of its boundary launch (for_planes).
    int pass_sweeps(int it, int K, bool first, int extra) const {
        const bool pair = can_fuse2() && it + 2 <= K;
        const int left = K - it;
        if (first) return sk_first_ok(K) ? 4 : (pair ? 2 : 1);
        const bool march = pair && sw_.sk_s >= 3 && left >= 3;
        if (march && sw_.sk_s >= 4 && left >= 4 && left != 5 && left != 6 && march_pass(4, extra)) return 4;
        if (march && left != 4 && march_pass(3, extra)) return 3;
        return pair ? 2 : 1;
    }
    // boundary depth of a two-sweep launch: the register-blocked pair kernel works on plane pairs, and a plane block
    // must not straddle the split of a boundary launch, so with three ghost planes it takes four planes per side
    int pair_depth() const { return G_ >= 3 ? 4 : 2; }

    // The passes of a K-sweep solve. source: the first pass folds add_source in (op_diffuse_src); x_zero: the iterate
    // is zero (project's pressure); dead_ishell: nothing reads the result's i-shell, so no pass writes it. Reads what
    // the constructor (and tune_schedule) set, launches nothing.
    //
    // Trapezoid blocks. Decomposed grid, fused pairs: a cross-stream wait in front of every interior launch costs
    // ~10 us of idle GPU per pair (measured: tools/evgap.hip, profiles of tools/rank_share.py). So the boundary launch
    // grows by two planes per side and pair ("trapezoid") for trap_m_ pairs: interior launch j then covers planes
    // [G+2+2j, ...) and reads only what interior launch j-1 wrote (planes [G+2j, ...)), back to back on the compute
    // stream, while boundary launch j (planes [G, G+2+2j), on its own stream, after interior j-1 and halo j-1) feeds
    // the halo exchange. Every trap_m_ pairs the interior snaps back and waits for the boundary once. Same arithmetic
    // on every plane whichever launch computes it: results do not change.
    // With S sweeps per launch the growth is S planes per side: if interior launch j-1 started D planes into the slab,
    // launch j starts D + max(S_j, S_{j-1}) planes in (S_j = its sweeps). S_j: it reads only what interior launch j-1
    // wrote. S_{j-1}: it WRITES the buffer that was the input of launch j-1, which boundary launch j-1 (another
    // stream, possibly still running) reads up to D + S_{j-1} planes in — a four-sweep launch followed by a
    // three-sweep one raced there until this was the maximum. Its boundary launch takes those planes.
    std::vector<Pass> plan_solve(int K, bool source, bool x_zero, bool dead_ishell) const {
        std::vector<Pass> plan;
        bool batch = batch_march(K, false);
        int tj = 0, dprev = 0, sprev = 0;  // passes in the trapezoid block so far; depth and sweeps of the pass before
        for (int it = 0; it < K;) {
            const bool pair = can_fuse2() && it + 2 <= K;
            Pass p{};
            // (a zero iterate is implicit in a fused pair or a marching pass only: the first pair then loads no x at all)
            p.first = it > 0 ? First::NONE : (source ? First::SOURCE : (x_zero && pair ? First::ZERO : First::CALLER));
            p.sweeps = pass_sweeps(it, K, it == 0, 0);
            p.depth = p.sweeps == 2 ? pair_depth() : p.sweeps;
            const int depth0 = std::max(p.depth, G_);  // boundary depth without growth
            // where its interior launch would start if it continued the trapezoid block
            // (inject_trap_bug_: SF_TRACE_SCHEDULE's ",inject=trap" — the round-2 race, for the checker's own test)
            const int d = dprev + (inject_trap_bug_ ? p.sweeps : std::max(p.sweeps, sprev));
            bool cont = pair && P_ > 1 && G_ >= 2 && trap_m_ > 1 && tj > 0 && tj < trap_m_ && d >= depth0 && nzl_ > 2 * d + 2;
            if (cont && p.sweeps >= 3 && pass_sweeps(it, K, it == 0, d - depth0) != p.sweeps) cont = false;  // interior too short
            if (cont && p.sweeps == 2 && (d & 1)) cont = false;  // plane pairs: even boundary depth
            p.extra = cont ? d - depth0 : 0;
            dprev = depth0 + p.extra;
            sprev = p.sweeps;
            tj = cont ? tj + 1 : 1;
            p.last = it + p.sweeps == K && !dead_ishell;
            p.batch = batch;
            p.name = source && it == 0 ? "jacobi_src"
                                       : (p.sweeps == 4 ? "jacobi4" : (p.sweeps == 3 ? "jacobi3" : (p.sweeps == 2 ? "jacobi2" : "jacobi1")));
            plan.push_back(p);
            it += p.sweeps;
            if (p.first == First::SOURCE) {
                // the passes after a folded source form a solve of their own: a new trapezoid block, batched by their
                // own count (K = 6: a pair, then one batched four-sweep pass)
                tj = 0;
                batch = batch_march(K - it, true);
            }
        }
        return plan;
    }

    // K Jacobi sweeps on NF fields at once; scratch buffers are swapped into the slots — or, with `partner`, the buffers
    // of those slots (the preconditioner of SPEC §11.2, whose caller holds the scratch buffers). dead_ishell, x_zero: see
    // plan_solve. src: diffuse with add_source folded in (op_diffuse_src) — the first pass reads the source as its
    // iterate and the field x before add_source, forms x + dt*src in registers and stores it to the x0 slot's buffer
    // (whose old content is dead) for the later passes.
    template <int NF>
    void op_lin_solve(const int (&x)[NF], const int (&x0)[NF], const int (&b)[NF], T a, T c, int K, bool dead_ishell,
                      bool x_zero = false, const int (*src)[NF] = nullptr, const int (*partner)[NF] = nullptr) {
        static_assert(NF <= NSCRATCH, "not enough scratch buffers");
        // the buffer a pass of field f writes: the ping-pong partner of x[f]
        auto xn = [&](Slab& sl, int f) -> T*& { return partner ? sl.field[(*partner)[f]] : sl.scratch[f]; };
        if constexpr (NF > 1) {
            if (solve_apart(K)) {
                for (int f = 0; f < NF; ++f) {
                    const int xf[1] = {x[f]}, x0f[1] = {x0[f]}, bf[1] = {b[f]}, sf[1] = {src ? (*src)[f] : 0};
                    const int pf[1] = {partner ? (*partner)[f] : 0};
                    op_lin_solve<1>(xf, x0f, bf, a, c, K, dead_ishell, x_zero, src ? &sf : nullptr, partner ? &pf : nullptr);
                }
                return;
            }
        }
        const T inv = T(1) / c;
        for (Slab& sl : slabs_)
            for (int f = 0; f < NF; ++f) {
                ensure(sl, x[f]);
                ensure(sl, x0[f]);
                if (src) ensure(sl, (*src)[f]);
            }
        for (const Pass& p : plan_solve(K, src != nullptr, x_zero, dead_ishell)) {
            const bool from_src = p.first == First::SOURCE;
            const int s = p.sweeps;  // = the reach of the pass in planes
            auto accesses = [&](Slab& sl, int a, int b, int lo, int hi, std::vector<Acc>& acc) {
                for (int f = 0; f < NF; ++f) {
                    if (p.first != First::ZERO) acc.push_back({sl.field[from_src ? (*src)[f] : x[f]], false, a - s, b + s});
                    acc.push_back({sl.field[from_src ? x[f] : x0[f]], false, a - (s - 1), b + (s - 1)});
                    acc.push_back({xn(sl, f), true, lo, hi});
                    if (from_src) acc.push_back({sl.field[x0[f]], true, a, b});
                }
            };
            for_planes(p.name, accesses, [&](const Launch& L) {
                sfk::JacobiArgs<T, NF> A{};
                for (int f = 0; f < NF; ++f) {
                    A.x[f] = L.sl.field[from_src ? (*src)[f] : x[f]];  // iterate (the source: Stam's initial guess)
                    A.x0[f] = L.sl.field[from_src ? x[f] : x0[f]];     // right-hand side (the field before add_source)
                    A.xn[f] = xn(L.sl, f);
                    if (from_src) A.x0out[f] = L.sl.field[x0[f]];  // right-hand side x + dt*src for the later passes
                    A.b[f] = b[f];
                }
                A.a = a;
                A.inv = inv;
                if (from_src) A.dt = dt_;
                launch_pass<NF>(L, A, p);
            }, p.depth, p.extra);
            // The pass stores the folded right-hand side on the planes it computes; on a decomposed grid the later
            // passes also read it on the ghost planes next to the slab, which a small launch fills from the (current)
            // ghost planes of x and src.
            if (from_src) rhs_on_ghost_planes<NF>(x, x0, *src, p.depth);
            // the new iterate becomes the field; the old buffer becomes scratch
            for (Slab& sl : slabs_)
                for (int f = 0; f < NF; ++f) std::swap(sl.field[x[f]], xn(sl, f));
            exchange<NF>(x);
        }
    }

    // Right-hand side x + dt*src of a folded add_source on the G-1 ghost planes next to the slab on either side (an
    // S-sweep launch evaluates its first S-1 levels there and needs x0 for them; the source pass itself stores it on the
    // planes it computes). It reads ghost planes of x, so it must follow the last halo: on the boundary stream when
    // for_planes ran its two-stream schedule with that boundary depth (bs waits for every halo and the next boundary
    // launch follows in stream order), on the compute stream otherwise (for_planes has just joined it).
    template <int NF>
    void rhs_on_ghost_planes(const int (&x)[NF], const int (&x0)[NF], const int (&src)[NF], int depth) {
        if (P_ == 1) return;
        const bool two = sw_.split && nzl_ > 2 * std::max(depth, G_);
        for (Slab& sl : slabs_) {
            sfk::RhsPlanesArgs<T, NF> R;
            for (int f = 0; f < NF; ++f) {
                R.out[f] = sl.field[x0[f]];
                R.a[f] = sl.field[x[f]];
                R.s[f] = sl.field[src[f]];
            }
            R.dt = dt_;
            R.off[0] = (long)1 * plane_;            // planes 1 .. G-1
            R.off[1] = (long)(G_ + nzl_) * plane_;  // planes G+nzl .. G+nzl+G-2
            R.nvec = (long)(G_ - 1) * plane_ / W;
            hipLaunchKernelGGL((sfk::rhs_planes_kernel<T, NF>), dim3((unsigned)ceil_div(R.nvec, 256L), 2), dim3(256), 0,
                               two ? sl.bs : sl.cs, R);
            if (trace_) {
                std::vector<Acc> acc;
                for (int f = 0; f < NF; ++f)
                    for (int side = 0; side < 2; ++side) {
                        const int lo = side ? G_ + nzl_ : 1, hi = lo + G_ - 1;
                        acc.push_back({sl.field[x[f]], false, lo, hi});
                        acc.push_back({sl.field[src[f]], false, lo, hi});
                        acc.push_back({sl.field[x0[f]], true, lo, hi});
                    }
                tr_op("rhs_ghost", sl, two ? sl.bs : sl.cs, acc);
            }
        }
        SF_HIP(hipGetLastError());
    }

    // diffuse with add_source folded in (sources bound to resident slots): replaces
    //     add_source_bound(x, x0 <- src); swap(x0, x); lin_solve(x, x0)
    // by a solve whose first pass reads the source (op_lin_solve). One pass over the arrays less per field.
    template <int NF>
    void op_diffuse_src(const int (&x)[NF], const int (&x0)[NF], const int (&b)[NF], const int (&src)[NF], T a, T c,
                        int K, bool dead_ishell) {
        if (sw_.fuse_src && can_fuse2() && K >= 2) {
            op_lin_solve<NF>(x, x0, b, a, c, K, dead_ishell, false, &src);
            return;
        }
        op_add_source_bound<NF>(x, x0, src);
        for (int f = 0; f < NF; ++f) swap_slots(x0[f], x[f]);
        op_lin_solve<NF>(x, x0, b, a, c, K, dead_ishell);
    }

    // The cell-to-lane mapping of the advect kernels (SF_ADVECT_ROW = 0 the gather form always, 2 / 3 always the
    // sharing / the pair form). Default: one cell per lane for the three velocity components. fp32: the i0+1 samples
    // from the neighbour lane (256^3 245 -> 171 us, 512^3 1628 -> 1217; with own (i0, i0+1) pair loads 215 / 1537).
    // fp64: own pair loads (256^3 376 -> 307 us; with neighbour-lane sharing 415). One field: the gather form stays
    // (fp32 79 vs 88 / 113, fp64 130 vs 150 / 129).
    enum class AdvectForm { GATHER, ROW, ROW_PAIRS };
    AdvectForm advect_form(int nf) const {
        if (!(sw_.advect_row >= 2 || (sw_.advect_row == 1 && nf >= 2))) return AdvectForm::GATHER;
        return (sw_.advect_row == 3 || (sw_.advect_row == 1 && sizeof(T) == 8)) ? AdvectForm::ROW_PAIRS : AdvectForm::ROW;
    }
    // the members AdvectArgs and AdvectMcArgs have in common
    template <class Args, int NF>
    void fill_advect_args(Args& A, const Slab& sl, const int (&d)[NF], const int (&d0)[NF], const int (&b)[NF], int u,
                          int v, int w, bool dead_ishell) const {
        for (int f = 0; f < NF; ++f) {
            A.d[f] = sl.field[d[f]];
            A.d0[f] = sl.field[d0[f]];
            A.b[f] = b[f];
        }
        A.u = sl.field[u];
        A.v = sl.field[v];
        A.w = sl.field[w];
        A.dt0 = dt_ * (T)N_;
        A.flag = sl.d_flag;
        A.skip_ishell = dead_ishell ? 1 : 0;
    }
    // launch of the kernel of advect_form(nf) among the three given
    template <class Args, class KG, class KR, class KP>
    void launch_advect(const Launch& L, int nf, const Args& A, KG gather, KR row, KP row_pairs) {
        const AdvectForm form = advect_form(nf);
        if (form == AdvectForm::GATHER) {
            dim3 block;
            unsigned nblocks;
            const sfk::TileMap m = flat_map(L, block, nblocks);
            launch_k(L, gather, dim3(nblocks), block, A, m);
            return;
        }
        const int wpr = ceil_div(N_, 64);
        const dim3 nblocks((unsigned)ceil_div((long)wpr * N_ * (L.ke - L.kb), 4L));
        if (form == AdvectForm::ROW_PAIRS)
            launch_k(L, row_pairs, nblocks, 256u, A, wpr);
        else
            launch_k(L, row, nblocks, 256u, A, wpr);
    }

    // dead_ishell: nothing reads the i-shell of the result, which is left unwritten
    template <int NF>
    void op_advect(const int (&d)[NF], const int (&d0)[NF], const int (&b)[NF], int u, int v, int w, bool dead_ishell) {
        for (Slab& sl : slabs_) {
            for (int f = 0; f < NF; ++f) {
                ensure(sl, d[f]);
                ensure(sl, d0[f]);
            }
            for (int f : {u, v, w}) ensure(sl, f);
        }
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            for (int f = 0; f < NF; ++f) {
                acc.push_back({sl.field[d0[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[d[f]], true, lo, hi});
            }
            acc.push_back({sl.field[u], false, a, b_});
            acc.push_back({sl.field[v], false, a, b_});
            acc.push_back({sl.field[w], false, a, b_});
        };
        for_planes("advect", accesses, [&](const Launch& L) {
            sfk::AdvectArgs<T, NF> A;
            fill_advect_args(A, L.sl, d, d0, b, u, v, w, dead_ishell);
            launch_advect(L, NF, A, sfk::advect_kernel<T, NF>, sfk::advect_row_kernel<T, NF>,
                          sfk::advect_row_kernel<T, NF, true>);
        }, 1, 0, /*interior_reads_ghosts=*/true);  // a long back-trace may reach a ghost plane from any plane
        exchange<NF>(d);
    }

    // SPEC §9 advect_mc: pass 1 is op_advect into `hat` (every shell written, ghost planes exchanged: pass 2 reads hat
    // wherever advect reads d0), pass 2 the limited correction into d. dead_ishell applies to d only.
    template <int NF>
    void op_advect_mc(const int (&d)[NF], const int (&d0)[NF], const int (&b)[NF], int u, int v, int w, bool dead_ishell) {
        static_assert(NF <= NSCRATCH, "not enough scratch buffers");
        for (Slab& sl : slabs_) {
            for (int f = 0; f < NF; ++f) {
                ensure(sl, d[f]);
                ensure(sl, d0[f]);
            }
            for (int f : {u, v, w}) ensure(sl, f);
        }
        // hat lives in the scratch buffers, addressed through the HAT slots while this operator is issued
        ScratchAlias hat_slots(slabs_, NF);
        int hat[NF];
        for (int f = 0; f < NF; ++f) hat[f] = HAT_SLOT + f;
        op_advect<NF>(hat, d0, b, u, v, w, false);
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            for (int f = 0; f < NF; ++f) {
                acc.push_back({sl.field[d0[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[hat[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[d[f]], true, lo, hi});
            }
            for (int q : {u, v, w}) acc.push_back({sl.field[q], false, a, b_});
        };
        for_planes("advect_mc", accesses, [&](const Launch& L) {
            sfk::AdvectMcArgs<T, NF> A;
            fill_advect_args(A, L.sl, d, d0, b, u, v, w, dead_ishell);
            for (int f = 0; f < NF; ++f) A.hat[f] = L.sl.field[hat[f]];
            launch_advect(L, NF, A, sfk::advect_mc_kernel<T, NF>, sfk::advect_mc_row_kernel<T, NF>,
                          sfk::advect_mc_row_kernel<T, NF, true>);
        }, 1, 0, /*interior_reads_ghosts=*/true);  // either trace may reach a ghost plane from any plane
        exchange<NF>(d);
    }

    sfk::ProjectArgs<T> project_args(Slab& sl, int u, int v, int w, int p, int div, bool mirror_u, bool mirror_p,
                                     bool skip_div_ishell) {
        const T Nf = (T)N_;
        const T h = T(1) / Nf;
        sfk::ProjectArgs<T> A;
        A.u = ensure(sl, u);
        A.v = ensure(sl, v);
        A.w = ensure(sl, w);
        A.p = ensure(sl, p);
        A.div = ensure(sl, div);
        A.c_div = T(-0.5) * h;
        A.c_grad = T(0.5) * Nf;
        A.mirror_u = mirror_u ? 1 : 0;
        A.mirror_p = mirror_p ? 1 : 0;
        A.skip_div_ishell = skip_div_ishell ? 1 : 0;
        return A;
    }

    // First half of SPEC §3 project: p = 0 (zero_p: the whole field, ghosts and shells included; else the solve that
    // follows treats p as literal zeros), div with set_bnd(0, div), div's ghost planes.
    void project_first_half(int u, int v, int w, int p, int div, bool mirror_u, bool dead_div, bool zero_p) {
        if (zero_p) join();
        for (Slab& sl : slabs_) {
            ensure(sl, p);
            if (zero_p) {
                SF_HIP(hipMemsetAsync(sl.field[p], 0, (size_t)field_elems_ * sizeof(T), sl.cs));
                tr_whole("zero_p", sl, {}, {sl.field[p]});
            }
        }
        auto div_acc = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            acc.push_back({sl.field[u], false, a, b_});
            acc.push_back({sl.field[v], false, a, b_});
            acc.push_back({sl.field[w], false, a - 1, b_ + 1});
            acc.push_back({sl.field[div], true, lo, hi});
        };
        for_planes("project_div", div_acc, [&](const Launch& L) {
            dim3 block;
            unsigned nblocks;
            const sfk::TileMap m = flat_map(L, block, nblocks);
            launch_k(L, sfk::project_div_kernel<T>, dim3(nblocks), block,
                     project_args(L.sl, u, v, w, p, div, mirror_u, false, dead_div), m);
        });
        // div's ghost planes are exchanged although a single sweep reads div at cell centres only: the fused
        // sweep pair evaluates its first sweep on the first ghost plane and needs x0 = div there, and div is left
        // in the v0 slot, where the caller may use it as the next step's source / initial guess (all G planes).
        // p is zero, ghosts included.
        const int dv[1] = {div};
        exchange<1>(dv);
    }

    // Second half of SPEC §3 project: the gradient subtracted, set_bnd(1, u), (2, v), (3, w), their ghost planes.
    void project_second_half(int u, int v, int w, int p, int div, bool mirror_p) {
        auto sub_acc = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            acc.push_back({sl.field[p], false, a - 1, b_ + 1});
            for (int q : {u, v, w}) {
                acc.push_back({sl.field[q], false, a, b_});
                acc.push_back({sl.field[q], true, lo, hi});
            }
        };
        for_planes("project_sub", sub_acc, [&](const Launch& L) {
            dim3 block;
            unsigned nblocks;
            const sfk::TileMap m = flat_map(L, block, nblocks);
            launch_k(L, sfk::project_sub_kernel<T>, dim3(nblocks), block,
                     project_args(L.sl, u, v, w, p, div, false, mirror_p, false), m);
        });
        const int uvw[3] = {u, v, w};
        exchange<3>(uvw);
    }

    // ---- the two halves under obstacles (SPEC §15): one row launch per slab on its compute stream ----
    sfk::ProjectMaskArgs<T> project_mask_args(Slab& sl, int u, int v, int w, int p, int div) {
        const T Nf = (T)N_;
        sfk::ProjectMaskArgs<T> A{};
        A.u = u >= 0 ? ensure(sl, u) : nullptr;
        A.v = v >= 0 ? ensure(sl, v) : nullptr;
        A.w = w >= 0 ? ensure(sl, w) : nullptr;
        A.p = ensure(sl, p);
        A.div = div >= 0 ? ensure(sl, div) : nullptr;
        A.code = sl.field[OBST_SLOT];
        A.c_div = T(-0.5) * (T(1) / Nf);
        A.c_grad = T(0.5) * Nf;
        return A;
    }
    // a field as a row launch over the slab's own planes writes it: the shell plane of a wall slab included
    Acc rows_written(const Slab& sl, const T* buf) const {
        int lo, hi;
        wr_range(sl, G_, G_ + nzl_, lo, hi);
        return Acc{buf, true, lo, hi};
    }
    // SPEC §19: the argument of the moving siblings, and the solid velocity as the two halves read it
    sfk::ProjectMovingArgs<T> project_moving_args(Slab& sl, int u, int v, int w, int p, int div) {
        return sfk::ProjectMovingArgs<T>{project_mask_args(sl, u, v, w, p, div), sl.field[OBSTV_SLOT], sl.field[OBSTV_SLOT + 1],
                                         sl.field[OBSTV_SLOT + 2]};
    }
    void project_first_half_masked(int u, int v, int w, int p, int div) {
        join();
        for (Slab& sl : slabs_) {
            for (int f : {u, v, w, p, div}) ensure(sl, f);
            SF_HIP(hipMemsetAsync(sl.field[p], 0, (size_t)field_elems_ * sizeof(T), sl.cs));
            tr_whole("zero_p", sl, {}, {sl.field[p]});
        }
        if (obstv_on_) {
            launch_rows<false>("project_div_moving", sfk::project_div_moving_kernel<T>,
                               [&](Slab& sl) { return project_moving_args(sl, u, v, w, p, div); },
                               [&](Slab& sl) {
                                   return std::vector<Acc>{{sl.field[u], false, G_, G_ + nzl_},
                                                           {sl.field[v], false, G_, G_ + nzl_},
                                                           {sl.field[w], false, G_ - 1, G_ + nzl_ + 1},
                                                           {sl.field[OBST_SLOT], false, G_, G_ + nzl_},
                                                           {sl.field[OBSTV_SLOT], false, G_, G_ + nzl_},
                                                           {sl.field[OBSTV_SLOT + 1], false, G_, G_ + nzl_},
                                                           {sl.field[OBSTV_SLOT + 2], false, G_ - 1, G_ + nzl_ + 1},
                                                           rows_written(sl, sl.field[div])};
                               });
            publish_from_cs(div);
            return;
        }
        launch_rows<false>("project_div_masked", sfk::project_div_masked_kernel<T>,
                           [&](Slab& sl) { return project_mask_args(sl, u, v, w, p, div); },
                           [&](Slab& sl) {
                               return std::vector<Acc>{{sl.field[u], false, G_, G_ + nzl_},
                                                       {sl.field[v], false, G_, G_ + nzl_},
                                                       {sl.field[w], false, G_ - 1, G_ + nzl_ + 1},
                                                       {sl.field[OBST_SLOT], false, G_, G_ + nzl_},
                                                       rows_written(sl, sl.field[div])};
                           });
        publish_from_cs(div);
    }
    void project_second_half_masked(int u, int v, int w, int p, int div) {
        join();  // p's ghost planes
        auto acc = [&](Slab& sl) {
            std::vector<Acc> a{{sl.field[p], false, G_ - 1, G_ + nzl_ + 1}, {sl.field[OBST_SLOT], false, G_, G_ + nzl_}};
            for (int q : {u, v, w}) {
                a.push_back({sl.field[q], false, G_, G_ + nzl_});
                a.push_back(rows_written(sl, sl.field[q]));
            }
            if (obstv_on_)
                for (int q = 0; q < 3; ++q) a.push_back({sl.field[OBSTV_SLOT + q], false, G_, G_ + nzl_});
            return a;
        };
        if (obstv_on_)  // SPEC §19
            launch_rows<false>("project_sub_moving", sfk::project_sub_moving_kernel<T>,
                               [&](Slab& sl) { return project_moving_args(sl, u, v, w, p, div); }, acc);
        else
            launch_rows<false>("project_sub_masked", sfk::project_sub_masked_kernel<T>,
                               [&](Slab& sl) { return project_mask_args(sl, u, v, w, p, div); }, acc);
        if (P_ == 1) return;
        for (Slab& sl : slabs_) ev_record(sl, &Slab::boundary_done, sl.cs);
        const int uvw[3] = {u, v, w};
        exchange<3>(uvw);
    }
    // the end of dens_step under obstacles: x = +0 on solid cells, set_bnd(0, x), its ghost planes
    void op_zero_solid(int x) {
        join();
        launch_rows<false>("zero_solid", sfk::zero_solid_kernel<T>,
                           [&](Slab& sl) { return project_mask_args(sl, -1, -1, -1, x, -1); },
                           [&](Slab& sl) {
                               return std::vector<Acc>{{sl.field[x], false, G_, G_ + nzl_},
                                                       {sl.field[OBST_SLOT], false, G_, G_ + nzl_},
                                                       rows_written(sl, sl.field[x])};
                           });
        publish_from_cs(x);
    }

    // ---- mask-aware transport (SPEC §17) ----
    // advect_masked reads the face codes at its sample cells: +0 into the shell entries of OBST_SLOT on the planes each
    // slab is the owner of (face_code_kernel writes interior cells only), then its ghost planes.
    void code_shells_publish() {
        join();
        for (Slab& sl : slabs_) {
            const int kb = G_ - (sl.geom.wall_lo ? 1 : 0), ke = G_ + nzl_ + (sl.geom.wall_hi ? 1 : 0);
            const long rows = (long)(N_ + 2) * (ke - kb);
            hipLaunchKernelGGL(sfk::code_shell_kernel<T>, dim3((unsigned)ceil_div(rows, 256L)), dim3(256), 0, sl.cs, sl.geom,
                               sl.field[OBST_SLOT], kb, ke);
            SF_HIP(hipGetLastError());
            tr_op("code_shells", sl, sl.cs, {{sl.field[OBST_SLOT], true, kb, ke}});
        }
        publish_from_cs(OBST_SLOT);
    }
    // K masked Jacobi sweeps on NF fields at once (§17 lin_solve_masked): one row launch per sweep and slab on the
    // compute stream, the ghost planes of the new iterate after each; ping-pong with scratch[f] as op_lin_solve.
    template <int NF>
    void op_lin_solve_masked(const int (&x)[NF], const int (&x0)[NF], const int (&b)[NF], T a, T c, int K) {
        static_assert(NF <= NSCRATCH, "not enough scratch buffers");
        const T inv = T(1) / c;
        for (Slab& sl : slabs_)
            for (int f = 0; f < NF; ++f) {
                ensure(sl, x[f]);
                ensure(sl, x0[f]);
            }
        // SPEC §19: the moving sibling when a solid velocity is set and some field is a velocity component (a b = 0
        // field in such a launch reads us and uses nothing of it)
        bool moving = false;
        for (int f = 0; f < NF; ++f) moving = moving || (obstv_on_ && b[f] != 0);
        auto xs_slot = [&](int f) { return OBSTV_SLOT + (b[f] > 0 ? b[f] - 1 : 0); };
        auto margs = [&](Slab& sl) {
            sfk::LinSolveMaskArgs<T, NF> A{};
            for (int f = 0; f < NF; ++f) {
                A.x[f] = sl.field[x[f]];
                A.x0[f] = sl.field[x0[f]];
                A.xn[f] = sl.scratch[f];
                A.b[f] = b[f];
            }
            A.code = sl.field[OBST_SLOT];
            A.a = a;
            A.inv = inv;
            return A;
        };
        auto macc = [&](Slab& sl) {
            std::vector<Acc> acc{{sl.field[OBST_SLOT], false, G_, G_ + nzl_}};
            for (int f = 0; f < NF; ++f) {
                acc.push_back({sl.field[x[f]], false, G_ - 1, G_ + nzl_ + 1});
                acc.push_back({sl.field[x0[f]], false, G_, G_ + nzl_});
                acc.push_back(rows_written(sl, sl.scratch[f]));
                if (moving) {  // the k-neighbour rows of ws for b = 3, the slab's own planes otherwise
                    const int g = b[f] == 3 ? 1 : 0;
                    acc.push_back({sl.field[xs_slot(f)], false, G_ - g, G_ + nzl_ + g});
                }
            }
            return acc;
        };
        for (int it = 0; it < K; ++it) {
            join();  // the ghost planes of the iterate
            if (moving)
                launch_rows<false>("lin_solve_moving", sfk::lin_solve_moving_kernel<T, NF>,
                                   [&](Slab& sl) {
                                       sfk::LinSolveMovingArgs<T, NF> A{};
                                       A.a = margs(sl);
                                       for (int f = 0; f < NF; ++f) A.xs[f] = sl.field[xs_slot(f)];
                                       return A;
                                   },
                                   macc);
            else
                launch_rows<false>("lin_solve_masked", sfk::lin_solve_masked_kernel<T, NF>, margs, macc);
            // the new iterate becomes the field; the old buffer becomes scratch
            for (Slab& sl : slabs_)
                for (int f = 0; f < NF; ++f) std::swap(sl.field[x[f]], sl.scratch[f]);
            if (P_ == 1) continue;
            for (Slab& sl : slabs_) ev_record(sl, &Slab::boundary_done, sl.cs);
            exchange<NF>(x);
        }
    }
    // §17 advect_masked: op_advect with the masked sibling of the gather form (the one form there is), which also
    // reads the face codes wherever it reads d0.
    template <int NF>
    void op_advect_masked(const int (&d)[NF], const int (&d0)[NF], const int (&b)[NF], int u, int v, int w) {
        for (Slab& sl : slabs_) {
            for (int f = 0; f < NF; ++f) {
                ensure(sl, d[f]);
                ensure(sl, d0[f]);
            }
            for (int f : {u, v, w}) ensure(sl, f);
        }
        // SPEC §19: the moving sibling when a solid velocity is set and some field is a velocity component
        bool moving = false;
        for (int f = 0; f < NF; ++f) moving = moving || (obstv_on_ && b[f] != 0);
        auto xs_slot = [&](int f) { return OBSTV_SLOT + (b[f] > 0 ? b[f] - 1 : 0); };
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            for (int f = 0; f < NF; ++f) {
                acc.push_back({sl.field[d0[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[d[f]], true, lo, hi});
            }
            acc.push_back({sl.field[OBST_SLOT], false, a - 1, b_ + 1});
            for (int q : {u, v, w}) acc.push_back({sl.field[q], false, a, b_});
            if (moving)
                for (int f = 0; f < NF; ++f) acc.push_back({sl.field[xs_slot(f)], false, a - 1, b_ + 1});
        };
        for_planes(moving ? "advect_moving" : "advect_masked", accesses, [&](const Launch& L) {
            sfk::AdvectMaskArgs<T, NF> A;
            fill_advect_args(A.a, L.sl, d, d0, b, u, v, w, false);
            A.code = L.sl.field[OBST_SLOT];
            dim3 block;
            unsigned nblocks;
            const sfk::TileMap m = flat_map(L, block, nblocks);
            if (moving) {
                sfk::AdvectMovingArgs<T, NF> MV;
                MV.m = A;
                for (int f = 0; f < NF; ++f) MV.xs[f] = L.sl.field[xs_slot(f)];
                launch_k(L, sfk::advect_moving_kernel<T, NF>, dim3(nblocks), block, MV, m);
            } else {
                launch_k(L, sfk::advect_masked_kernel<T, NF>, dim3(nblocks), block, A, m);
            }
        }, 1, 0, /*interior_reads_ghosts=*/true);  // a long back-trace may reach a ghost plane from any plane
        exchange<NF>(d);
    }
    // §18 advect_mc_masked: pass 1 is op_advect_masked into `hat` (every shell written, ghost planes exchanged), pass 2
    // the masked sibling of advect_mc's gather form, which reads the face codes wherever either trace samples.
    template <int NF>
    void op_advect_mc_masked(const int (&d)[NF], const int (&d0)[NF], const int (&b)[NF], int u, int v, int w) {
        static_assert(NF <= NSCRATCH, "not enough scratch buffers");
        for (Slab& sl : slabs_) {
            for (int f = 0; f < NF; ++f) {
                ensure(sl, d[f]);
                ensure(sl, d0[f]);
            }
            for (int f : {u, v, w}) ensure(sl, f);
        }
        // hat lives in the scratch buffers, addressed through the HAT slots while this operator is issued
        ScratchAlias hat_slots(slabs_, NF);
        int hat[NF];
        for (int f = 0; f < NF; ++f) hat[f] = HAT_SLOT + f;
        op_advect_masked<NF>(hat, d0, b, u, v, w);
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            for (int f = 0; f < NF; ++f) {
                acc.push_back({sl.field[d0[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[hat[f]], false, a - 1, b_ + 1});
                acc.push_back({sl.field[d[f]], true, lo, hi});
            }
            acc.push_back({sl.field[OBST_SLOT], false, a - 1, b_ + 1});
            for (int q : {u, v, w}) acc.push_back({sl.field[q], false, a, b_});
        };
        for_planes("advect_mc_masked", accesses, [&](const Launch& L) {
            sfk::AdvectMcMaskArgs<T, NF> A;
            fill_advect_args(A.a, L.sl, d, d0, b, u, v, w, false);
            for (int f = 0; f < NF; ++f) A.a.hat[f] = L.sl.field[hat[f]];
            A.code = L.sl.field[OBST_SLOT];
            dim3 block;
            unsigned nblocks;
            const sfk::TileMap m = flat_map(L, block, nblocks);
            launch_k(L, sfk::advect_mc_masked_kernel<T, NF>, dim3(nblocks), block, A, m);
        }, 1, 0, /*interior_reads_ghosts=*/true);  // either trace may reach a ghost plane from any plane
        exchange<NF>(d);
    }

    void note_solve(int solver, int status, int iterations, double rel) {
        info_.solver = solver;
        info_.status = status;
        info_.iterations = iterations;
        info_.rel_residual = rel;
        info_.solves_total += 1;
        info_.iterations_total += iterations;
    }

    // mirror_u: u's i-shell was left unwritten by the solve before (b = 1: mirrored in project_div); dead_p: nothing reads
    // p after this projection (its slot is overwritten before anyone looks), so the solve leaves p's i-shell unwritten
    // and project_sub mirrors it. Both false for the public sf_project().
    void op_project(int u, int v, int w, int p, int div, bool mirror_u = false, bool dead_p = false) {
        mirror_u = mirror_u && ishell_skip_;
        dead_p = dead_p && ishell_skip_ && K_ >= 1;
        // (a projection whose pressure is dead is the first one of vel_step: its div slot is overwritten as well)
        const bool dead_div = dead_p;
        // p = 0: when the first two sweeps are fused the kernel treats x as literal zeros and p is never read,
        // so the fill (one word per cell) is skipped; otherwise zero the whole field (ghosts and shells included)
        const bool implicit_zero = can_fuse2() && K_ >= 2 && sw_.zero_skip;
        project_first_half(u, v, w, p, div, mirror_u, dead_div, !implicit_zero);
        const int ps[1] = {p}, dv[1] = {div}, b0[1] = {0};
        op_lin_solve<1>(ps, dv, b0, T(1), T(6), K_, dead_p, implicit_zero);
        project_second_half(u, v, w, p, div, dead_p);
        note_solve(SF_PRESSURE_JACOBI, SF_CG_MAX_ITERS, K_, -1.0);
    }

    // ---- conjugate-gradient projection (SPEC §11) ---------------------------------------------------------------
    // The work fields r, d, q are the three scratch buffers, addressed through internal slots while the operator is
    // issued (exchange() takes slots), as `hat` is in op_advect_mc. Every row kernel runs a slab's nzl planes in one
    // launch on its compute stream; d's ghost planes travel on the halo stream after every update of d.
    // One skeleton, cg_iterate<DEV>, issues the solve: plain (§11) or with z = M(r) and a third sum, r.z, in every
    // iteration (§11.2, op_precondition: the Jacobi sweeps, or the V-cycle of §11.3); with the scalars on the host (check_every_ = 0) or on the device (m >= 1).
    // The two forms differ in what a sum's stage is (cg_sum), in the kernels' DEV parameter and argument (cg_args) and
    // in the state that the DEV forms add to a kernel's trace; what a stage does with its sum (the stop tests, their
    // status, alpha and beta as T) is sfk::cg_stage on both. Host waits: one per sum by value (2 + 2 per iteration,
    // three per iteration preconditioned), one per m iterations with DEV (cg_state_read).
    double one_sum() {
        double r[1];
        finish_records(1, 1, 0, r);
        ++host_waits_;
        return r[0];
    }
    void cg_state_alloc() {
        // the plane records of all N planes in one buffer (the all-gather's, where there is a communicator)
        if (!red_gather_) red_gather_ = own_.dev<double>((size_t)sfk::DIAG_NV * N_ * sizeof(double));
        if (!cg_state_) {
            cg_state_ = own_.dev<sfk::CgState<T>>(sizeof(sfk::CgState<T>));
            SF_HIP(hipMemset(cg_state_, 0, sizeof(sfk::CgState<T>)));
        }
        if (!cg_state_host_) cg_state_host_ = own_.pinned<sfk::CgState<T>>(sizeof(sfk::CgState<T>));
    }
    // a slab's plane records inside red_gather_ (one value per plane)
    double* cg_records(const Slab& sl) const { return red_gather_ + (size_t)sl.gid * nzl_; }
    // What one_sum() does, without the host: row records -> every slab's plane records, next to each other in
    // red_gather_ -> (all ranks' records, gathered in place) -> cg_scalars_kernel on slab 0's compute stream, which the
    // other slabs' compute streams wait for. c: the stage's constant (N^3, tol * tol).
    template <int STAGE>
    void cg_scalars(double c) {
        Slab& s0 = slabs_[0];
        for (Slab& sl : slabs_) {
            hipLaunchKernelGGL(sfk::fold_rows_kernel, dim3(nzl_, 1), dim3(256), 0, sl.cs, sl.red_rows, cg_records(sl), N_,
                               rows_pad(), 1, 0);
            SF_HIP(hipGetLastError());
            tr_op("fold_rows", sl, sl.cs, {{sl.red_rows, false, 0, nplanes_}, {cg_records(sl), true, 0, nplanes_}});
        }
        for (int s = 1; s < L_; ++s) {
            ev_record(slabs_[s], &Slab::cs_mark, slabs_[s].cs);
            st_wait(s0, s0.cs, slabs_[s], &Slab::cs_mark);
        }
        std::vector<Acc> acc;
        for (Slab& sl : slabs_) acc.push_back({cg_records(sl), false, 0, nplanes_});
        if (comm_) {
            const size_t cnt = (size_t)L_ * nzl_;
            SF_NCCL(ncclGroupStart());
            SF_NCCL(ncclAllGather(red_gather_ + (size_t)rank_ * cnt, red_gather_, cnt, ncclDouble, comm_, s0.cs));
            SF_NCCL(ncclGroupEnd());
            ++rccl_groups_;
            acc.push_back({red_gather_, true, 0, nplanes_});  // (the other ranks' records)
            tr_op("records_allgather", s0, s0.cs, acc);
            acc.back().write = false;
        }
        // a loopback context stands for one rank of several and has nobody to gather from: its own planes only
        const bool own_only = nranks_ > 1 && !comm_;
        const int k0 = own_only ? rank_ * L_ * nzl_ : 0, k1 = own_only ? k0 + L_ * nzl_ : N_;
        hipLaunchKernelGGL((sfk::cg_scalars_kernel<T, STAGE>), dim3(1), dim3(256), 0, s0.cs, (const double*)red_gather_, k0, k1,
                           c, cg_state_);
        SF_HIP(hipGetLastError());
        acc.push_back({cg_state_, false, 0, nplanes_});
        acc.push_back({cg_state_, true, 0, nplanes_});
        tr_op("cg_scalars", s0, s0.cs, acc);
        if (L_ > 1) ev_record(s0, &Slab::cs_mark, s0.cs);
        for (int s = 1; s < L_; ++s) st_wait(slabs_[s], slabs_[s].cs, s0, &Slab::cs_mark);
    }
    // the one host wait of a batch: the state, as the last enqueued cg_scalars left it
    const sfk::CgState<T>& cg_state_read() {
        Slab& s0 = slabs_[0];
        SF_HIP(hipMemcpyAsync(cg_state_host_, cg_state_, sizeof(sfk::CgState<T>), hipMemcpyDeviceToHost, s0.cs));
        tr_op("cg_state_out", s0, s0.cs, {{cg_state_, false, 0, nplanes_}});
        SF_HIP(hipStreamSynchronize(s0.cs));
        ++host_waits_;
        return *cg_state_host_;
    }
    // One sum of a solve and what its stage does with it (sfk::cg_stage). By value: the host waits for the sum and
    // applies the stage to st; false once the solve has stopped. DEV: cg_scalars() enqueues both, and issuing goes on.
    template <bool DEV, int STAGE>
    bool cg_sum(sfk::CgState<T>& st, double c) {
        if constexpr (DEV) {
            cg_scalars<STAGE>(c);
            return true;
        } else {
            sfk::cg_stage<T, STAGE>(&st, one_sum(), c);
            return st.active != 0;
        }
    }
    // The argument of a CG row kernel. rhs: the field at div's place (z, for the kernels that read z: SPEC §11.2). The
    // scalar goes by value, or (DEV) the state goes where the by-value forms have it.
    template <bool DEV>
    sfk::CgArgs<T> cg_args(Slab& sl, int p, int rhs, T s) const {
        sfk::CgArgs<T> A;
        A.div = sl.field[rhs];
        A.p = sl.field[p];
        A.r = sl.field[CG_R];
        A.d = sl.field[CG_D];
        A.q = sl.field[CG_Q];
        if constexpr (DEV)
            A.st = cg_state_;
        else
            A.s = s;
        return A;
    }
    // ---- its Jacobi-sweep preconditioner (SPEC §11.2) ----
    void pcg_alloc() {
        for (Slab& sl : slabs_)
            for (int f : {CG_Z, CG_ZP})
                if (!sl.field[f]) sl.field[f] = alloc_field();
    }
    // z = M(r): z = +0, then lin_solve(0, z, r, 1, 6, sweeps) as the pass planner lays any solve out, ping-pong between
    // the two owning slots. A pass of s fused sweeps reads its right-hand side s - 1 planes beyond its own, so r's ghost
    // planes go first; it runs whether or not the solve is still active (the Jacobi kernels know no state) and leaves the
    // compute streams joined for the row kernel that follows.
    // The one place that chooses M: the V-cycle of §11.3 while sf_set_pressure_multigrid has it in force, else the sweeps.
    // z, r: the slots of the solve, or the two fields of sf_precondition.
    // masked: the V-cycle of §16 (the Jacobi sweeps never know the mask: SPEC §15).
    void op_precondition(int sweeps, int z = CG_Z, int r = CG_R, bool masked = false) {
        if (mg_nu_ > 0) {
            op_vcycle(z, r, masked);
            return;
        }
        publish_from_cs(r);
        // as in op_project: a fused first pass takes the zero iterate as literal zeros, any other reads it
        const bool implicit_zero = can_fuse2() && sweeps >= 2 && sw_.zero_skip;
        if (!implicit_zero) {
            join();
            for (Slab& sl : slabs_) {
                SF_HIP(hipMemsetAsync(sl.field[z], 0, (size_t)field_elems_ * sizeof(T), sl.cs));
                tr_whole("zero_z", sl, {}, {sl.field[z]});
            }
        }
        const int zs[1] = {z}, rs[1] = {r}, b0[1] = {0}, zp[1] = {CG_ZP};
        op_lin_solve<1>(zs, rs, b0, T(1), T(6), sweeps, false, implicit_zero, nullptr, &zp);
        join();
    }
    // sweeps of the z = M(r) in force: nu of the V-cycle, m of the Jacobi kind, 0 without a preconditioner
    int precond_sweeps_in_force() const {
        return mg_nu_ > 0 ? mg_nu_ : (precond_ == SF_PRECOND_JACOBI ? precond_sweeps_ : 0);
    }

    // ---- its multigrid preconditioner (SPEC §11.3) ----
    // n_0 = N and n_{l+1} = n_l / 2 while n_l is even, n_l / 2 >= 4 and the depth allows: N and max_levels decide alone
    std::vector<int> mg_sizes(int max_levels) const {
        std::vector<int> n{N_};
        while (n.back() % 2 == 0 && n.back() / 2 >= 4 && (max_levels == 0 || (int)n.size() < max_levels) &&
               (int)n.size() < MG_MAXL)
            n.push_back(n.back() / 2);
        return n;
    }
    // Level 0 is the solver's own geometry; a coarse level has the row layout of §4 for its n, one ghost plane per
    // side and no padding (the marching kernel never runs there).
    std::vector<Level> mg_levels() const {
        std::vector<Level> lv{lv0_};
        const std::vector<int> n = mg_sizes(mg_maxl_);
        const int line = 128 / (int)sizeof(T);
        for (size_t l = 1; l < n.size(); ++l) {
            Level h;
            h.N = n[l];
            h.nzl = n[l] / P_;
            h.G = 1;
            h.np = h.nzl + 2;
            h.px = ceil_div(lead_ + n[l] + 1 + W, line) * line;
            h.plane = (long)h.px * (n[l] + 2);
            h.elems = (h.plane * h.np + 256 + W - 1) / W * W;
            lv.push_back(h);
        }
        return lv;
    }
    // The face codes of the coarse levels (SPEC §16): level l + 1 is solid where all eight children are solid on level
    // l. The coarse mask is built in the level's right-hand side (free between cycles), its one ghost plane travels,
    // and face_code_kernel turns it into the level's codes exactly as sf_set_obstacles does on level 0 (the row records
    // it writes are not used). Same codes for every decomposition.
    void mg_codes_build(const std::vector<Level>& lv) {
        const int nl = (int)lv.size();
        for (Slab& sl : slabs_)
            for (int l = 1; l < nl; ++l)
                if (!sl.field[mg_code(l)]) sl.field[mg_code(l)] = alloc_field(&lv[l]);
        for (int l = 0; l + 1 < nl; ++l) {
            const Level &hf = lv[l], &hc = lv[l + 1];
            join();
            launch_rows<false>("mg_coarsen_mask", sfk::mg_coarsen_mask_kernel<T>,
                               [&](Slab& sl) {
                                   return sfk::MgMaskArgs<T>{{nullptr, nullptr, sl.field[mg_r(l + 1)], l == 0 ? sl.geom : level_geom(sl, hf)},
                                                             sl.field[mg_code(l)]};
                               },
                               [&](Slab& sl) {
                                   return std::vector<Acc>{{sl.field[mg_code(l)], false, hf.G, hf.G + hf.nzl},
                                                           {sl.field[mg_r(l + 1)], true, hc.G, hc.G + hc.nzl}};
                               }, &hc);
            publish_from_cs(mg_r(l + 1), &hc);
            join();
            launch_rows("mg_face_code", sfk::face_code_kernel<T>,
                        [&](Slab& sl) { return sfk::FaceCodeArgs<T>{sl.field[mg_r(l + 1)], sl.field[mg_code(l + 1)]}; },
                        [&](Slab& sl) {
                            return std::vector<Acc>{{sl.field[mg_r(l + 1)], false, hc.G - 1, hc.G + hc.nzl + 1},
                                                    {sl.field[mg_code(l + 1)], true, hc.G, hc.G + hc.nzl}};
                        }, &hc);
        }
        mg_codes_ok_ = true;
    }
    // One symmetric V-cycle z = V(0, r) (SPEC §11.3): down with nu sweeps from zero and the restricted residual per
    // level, nu_c sweeps on the coarsest, up with the correction and nu sweeps. Every kernel runs on the compute stream
    // of its slab; the ghost planes of z on a level travel after every sweep and after the correction (so they are
    // current before each sweep and before the residual), those of the coarse right-hand sides never (read on own planes
    // only). Leaves the compute streams joined.
    // masked (SPEC §16): the same cycle with the masked sibling of every kernel, which reads the face codes of its level
    // (restrict and prolong: of the fine level) besides.
    void op_vcycle(int z, int r, bool masked = false) {
        const std::vector<Level> lv = mg_levels();
        const int nl = (int)lv.size();
        for (Slab& sl : slabs_)
            for (int l = 1; l < nl; ++l)
                for (int f : {mg_z(l), mg_zp(l), mg_r(l)})
                    if (!sl.field[f]) sl.field[f] = alloc_field(&lv[l]);
        if (masked && !mg_codes_ok_) mg_codes_build(lv);
        auto zs = [&](int l) { return l == 0 ? z : mg_z(l); };
        auto ps = [&](int l) { return l == 0 ? CG_ZP : mg_zp(l); };
        auto rs = [&](int l) { return l == 0 ? r : mg_r(l); };
        auto lp = [&](int l) { return l == 0 ? (const Level*)nullptr : &lv[l]; };
        auto geom = [&](Slab& sl, int l) { return l == 0 ? sl.geom : level_geom(sl, lv[l]); };
        // planes a launch over the level's own planes writes: the shell plane of a wall slab included
        auto written = [&](Slab& sl, int l, const T* buf) {
            const Level& h = lv[l];
            return Acc{buf, true, sl.geom.wall_lo ? h.G - 1 : h.G, h.G + h.nzl + (sl.geom.wall_hi ? 1 : 0)};
        };
        // the masked forms: the sibling's argument and accesses, and the codes of level l on its own planes
        auto margs = [&](auto args, int l) {
            return [args, l](Slab& sl) { return sfk::MgMaskArgs<T>{args(sl), sl.field[mg_code(l)]}; };
        };
        auto macc = [&](auto acc, int l) {
            return [acc, l, &lv](Slab& sl) {
                std::vector<Acc> a = acc(sl);
                a.push_back({sl.field[mg_code(l)], false, lv[l].G, lv[l].G + lv[l].nzl});
                return a;
            };
        };
        auto sweeps = [&](int l, int count, bool from_zero) {
            const Level& h = lv[l];
            for (int t = 0; t < count; ++t) {
                join();  // z's ghost planes
                const bool first = from_zero && t == 0;
                auto args = [&](Slab& sl) { return sfk::MgArgs<T>{sl.field[zs(l)], sl.field[rs(l)], sl.field[ps(l)], sfk::Geom{}}; };
                auto acc = [&](Slab& sl) {
                    std::vector<Acc> a{{sl.field[rs(l)], false, h.G, h.G + h.nzl}, written(sl, l, sl.field[ps(l)])};
                    if (!first) a.push_back({sl.field[zs(l)], false, h.G - 1, h.G + h.nzl + 1});
                    return a;
                };
                if (masked && first)
                    launch_rows<false>("mg_smooth0_masked", sfk::mg_smooth_masked_kernel<T, true>, margs(args, l), macc(acc, l), lp(l));
                else if (masked)
                    launch_rows<false>("mg_smooth_masked", sfk::mg_smooth_masked_kernel<T, false>, margs(args, l), macc(acc, l), lp(l));
                else if (first)
                    launch_rows<false>("mg_smooth0", sfk::mg_smooth_kernel<T, true>, args, acc, lp(l));
                else
                    launch_rows<false>("mg_smooth", sfk::mg_smooth_kernel<T, false>, args, acc, lp(l));
                swap_slots(zs(l), ps(l));
                publish_from_cs(zs(l), lp(l));
            }
        };
        for (int l = 0;; ++l) {
            sweeps(l, l < nl - 1 ? mg_nu_ : mg_nuc_, true);
            if (l == nl - 1) break;
            const Level &hf = lv[l], &hc = lv[l + 1];
            join();  // the residual reads z's ghost planes
            auto args = [&](Slab& sl) { return sfk::MgArgs<T>{sl.field[zs(l)], sl.field[rs(l)], sl.field[rs(l + 1)], geom(sl, l)}; };
            auto acc = [&](Slab& sl) {
                return std::vector<Acc>{{sl.field[zs(l)], false, hf.G - 1, hf.G + hf.nzl + 1},
                                        {sl.field[rs(l)], false, hf.G, hf.G + hf.nzl},
                                        {sl.field[rs(l + 1)], true, hc.G, hc.G + hc.nzl}};
            };
            if (masked)
                launch_rows<false>("mg_restrict_masked", sfk::mg_restrict_masked_kernel<T>, margs(args, l), macc(acc, l), &hc);
            else
                launch_rows<false>("mg_restrict", sfk::mg_restrict_kernel<T>, args, acc, &hc);
        }
        for (int l = nl - 2; l >= 0; --l) {
            const Level &hf = lv[l], &hc = lv[l + 1];
            join();
            auto args = [&](Slab& sl) { return sfk::MgArgs<T>{sl.field[zs(l + 1)], nullptr, sl.field[zs(l)], geom(sl, l + 1)}; };
            auto acc = [&](Slab& sl) {
                return std::vector<Acc>{{sl.field[zs(l + 1)], false, hc.G, hc.G + hc.nzl},
                                        {sl.field[zs(l)], false, hf.G, hf.G + hf.nzl},
                                        written(sl, l, sl.field[zs(l)])};
            };
            if (masked)
                launch_rows<false>("mg_prolong_masked", sfk::mg_prolong_masked_kernel<T>, margs(args, l), macc(acc, l), lp(l));
            else
                launch_rows<false>("mg_prolong", sfk::mg_prolong_kernel<T>, args, acc, lp(l));
            publish_from_cs(zs(l), lp(l));
            sweeps(l, mg_nu_, false);
        }
        join();
    }

    void op_set_bnd(int b, int x, const char* trace_name) {
        join();
        for (Slab& sl : slabs_) {
            T* dev = ensure(sl, x);
            const long n0 = std::max((long)N_ * nzl_, (long)N_ * N_);
            const long n1 = std::max(N_, nzl_);
            hipLaunchKernelGGL((sfk::set_bnd_kernel<T>), dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0,
                               sl.cs, sl.geom, dev, b, 0);
            hipLaunchKernelGGL((sfk::set_bnd_kernel<T>), dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0,
                               sl.cs, sl.geom, dev, b, 1);
            hipLaunchKernelGGL((sfk::set_bnd_kernel<T>), dim3(1), dim3(64), 0, sl.cs, sl.geom, dev, b, 2);
            if (trace_name) tr_whole(trace_name, sl, {dev}, {dev});
        }
        SF_HIP(hipGetLastError());
        publish_from_cs(x);
    }

    // The iteration of SPEC §11 (pm = 0) or §11.2 (pm sweeps of z = M(r)), written once. DEV false: every stage is a
    // host wait, and nothing more is issued once a stage has stopped the solve. DEV: the stages are enqueued with the
    // kernels, which are no-ops past the iteration that stops the solve (cg_live) while the sweeps of M(r) and the
    // exchange of d go on as they were, so what is left does not depend on m; the state is read every m iterations.
    // Returns the state the solve ended in.
    template <bool DEV>
    sfk::CgState<T> cg_iterate(int p, int div, double tol, int max_iters, int pm) {
        const int kb = G_, ke = G_ + nzl_;
        const bool pc = pm > 0;
        const bool masked = obst_on_;  // SPEC §15: the masked siblings of init and apply, n_fluid as mu's divisor
        // d as a kernel writes it: the shell plane of a wall slab included
        auto d_written = [&](Slab& sl) {
            int lo, hi;
            wr_range(sl, kb, ke, lo, hi);
            return Acc{sl.field[CG_D], true, lo, hi};
        };
        // the fields each row kernel touches (z is whichever buffer the last pass of M(r) left in its slot)
        auto init_acc = [&](Slab& sl) {
            std::vector<Acc> a{{sl.field[div], false, kb, ke}, {sl.field[CG_R], true, kb, ke}, d_written(sl)};
            if (masked) a.push_back({sl.field[OBST_SLOT], false, kb, ke});
            return a;
        };
        auto apply_acc = [&](Slab& sl) {
            std::vector<Acc> a{{sl.field[CG_D], false, kb - 1, ke + 1}, {sl.field[CG_Q], true, kb, ke}};
            if (masked) a.push_back({sl.field[OBST_SLOT], false, kb, ke});
            return a;
        };
        auto update_acc = [&](Slab& sl) {
            return std::vector<Acc>{{sl.field[CG_D], false, kb, ke}, {sl.field[CG_Q], false, kb, ke},
                                    {sl.field[p], false, kb, ke},    {sl.field[p], true, kb, ke},
                                    {sl.field[CG_R], false, kb, ke}, {sl.field[CG_R], true, kb, ke}};
        };
        auto direction_acc = [&](Slab& sl) {
            return std::vector<Acc>{{sl.field[CG_R], false, kb, ke}, {sl.field[CG_D], false, kb, ke}, d_written(sl)};
        };
        auto dot_acc = [&](Slab& sl) {
            return std::vector<Acc>{{sl.field[CG_R], false, kb, ke}, {sl.field[CG_Z], false, kb, ke}};
        };
        auto direction_z_acc = [&](Slab& sl) {
            return std::vector<Acc>{{sl.field[CG_Z], false, kb, ke}, {sl.field[CG_D], false, kb, ke}, d_written(sl)};
        };
        // ... to which the device-scalar forms add the state they read
        auto acc = [&](auto fields) {
            return [this, fields](Slab& sl) {
                std::vector<Acc> a = fields(sl);
                if (DEV) a.push_back({cg_state_, false, 0, nplanes_});
                return a;
            };
        };
        // rhs: the field at div's place; s: the scalar of the by-value forms
        auto args = [&](int rhs, T s) { return [this, p, rhs, s](Slab& sl) { return cg_args<DEV>(sl, p, rhs, s); }; };
        auto margs = [&](int rhs, T s) {
            return [this, p, rhs, s](Slab& sl) {
                return sfk::CgMaskArgs<T>{cg_args<DEV>(sl, p, rhs, s), sl.field[OBST_SLOT]};
            };
        };

        sfk::CgState<T> st{};
        // z = M(r), gamma = r.z, then the direction from z: d = z (the first one) or z + beta * d
        auto direction_pc = [&](auto first) {
            constexpr bool INIT = decltype(first)::value;
            op_precondition(pm, CG_Z, CG_R, masked);
            launch_rows("cg_dot", sfk::cg_dot_kernel<T, DEV>, args(CG_Z, T(0)), acc(dot_acc));
            if (!cg_sum<DEV, INIT ? sfk::STAGE_GAMMA0 : sfk::STAGE_GAMMA>(st, 0.0)) return false;
            launch_rows<false>("cg_direction_z", sfk::cg_direction_z_kernel<T, DEV, INIT>, args(CG_Z, st.bT),
                               acc(direction_z_acc));
            publish_from_cs(CG_D);
            return true;
        };
        auto iteration = [&] {
            join();  // d's ghost planes
            if (masked)
                launch_rows("cg_apply_dot_masked", sfk::cg_apply_dot_masked_kernel<T, false, DEV>, margs(div, T(0)),
                            acc(apply_acc));
            else
                launch_rows("cg_apply_dot", sfk::cg_apply_dot_kernel<T, false, DEV>, args(div, T(0)), acc(apply_acc));
            if (!(pc ? cg_sum<DEV, sfk::STAGE_DELTA_PC>(st, 0.0) : cg_sum<DEV, sfk::STAGE_DELTA>(st, 0.0))) return false;
            launch_rows("cg_update", sfk::cg_update_kernel<T, DEV>, args(div, st.aT), acc(update_acc));
            if (!(pc ? cg_sum<DEV, sfk::STAGE_RHO_PC>(st, tol * tol) : cg_sum<DEV, sfk::STAGE_RHO>(st, tol * tol)))
                return false;
            if (pc) return direction_pc(std::false_type{});
            // the one row kernel of a plain solve that writes no row records
            launch_rows<false>("cg_direction", sfk::cg_direction_kernel<T, DEV>, args(div, st.bT), acc(direction_acc));
            publish_from_cs(CG_D);
            return true;
        };

        launch_rows("cg_sum_div", sfk::reduce_rows_kernel<T, sfk::RED_SUM>,
                    [&](Slab& sl) { return (const T*)sl.field[div]; },
                    [&](Slab& sl) { return std::vector<Acc>{{sl.field[div], false, kb, ke}}; });
        // (with no fluid cell the sum is +0 and there is nothing to divide: mu = 0)
        const double cells = masked ? (n_fluid_ > 0 ? (double)n_fluid_ : 1.0) : (double)N_ * (double)N_ * (double)N_;
        cg_sum<DEV, sfk::STAGE_MU>(st, cells);
        if (masked)
            launch_rows("cg_init_masked", sfk::cg_init_masked_kernel<T, DEV>, margs(div, st.mu), acc(init_acc));
        else
            launch_rows("cg_init", sfk::cg_init_kernel<T, DEV>, args(div, st.mu), acc(init_acc));
        if (!pc) publish_from_cs(CG_D);  // (a preconditioned solve replaces d before anything reads its ghost planes)
        bool go = cg_sum<DEV, sfk::STAGE_RHO0>(st, 0.0);
        if (go && pc) go = direction_pc(std::true_type{});
        if constexpr (DEV) {
            int n = 0;
            do {
                for (const int end = n + std::min(check_every_, max_iters - n); n < end; ++n) iteration();
                st = cg_state_read();
            } while (st.active && n < max_iters);
        } else {
            for (int n = 0; go && n < max_iters; ++n) go = iteration();
        }
        return st;
    }

    void op_project_cg(int u, int v, int w, int p, int div, double tol, int max_iters, bool mirror_u = false) {
        mirror_u = mirror_u && ishell_skip_;
        SF_REQUIRE(!(obst_on_ && mg_nu_ > 0) || obst_mg_,
                   "project_cg: obstacles with the multigrid preconditioner in force are not supported (its coarse "
                   "operators do not know the mask); switch one of them off");
        records_alloc();
        static_assert(sfk::CG_ST_CONVERGED == SF_CG_CONVERGED && sfk::CG_ST_MAX_ITERS == SF_CG_MAX_ITERS &&
                          sfk::CG_ST_BREAKDOWN == SF_CG_BREAKDOWN, "CgState::status holds sf_cg_status values");
        const bool dev = check_every_ > 0;  // the scalars on the device, read back every check_every_ iterations
        if (dev) cg_state_alloc();
        const int pm = precond_sweeps_in_force();  // sweeps of z = M(r); 0: §11 as it stands
        if (pm > 0) pcg_alloc();
        host_waits_ = 0;
        ScratchAlias work_slots(slabs_, 3);
        if (obst_on_)
            project_first_half_masked(u, v, w, p, div);
        else
            project_first_half(u, v, w, p, div, mirror_u, false, true);
        join();
        // (a solve that max_iters ends is still active, with the status its rho0 stage left: SF_CG_MAX_ITERS)
        const sfk::CgState<T> st =
            dev ? cg_iterate<true>(p, div, tol, max_iters, pm) : cg_iterate<false>(p, div, tol, max_iters, pm);
        host_waits_total_ += host_waits_;
        op_set_bnd(0, p, "cg_set_bnd_p");
        if (obst_on_)
            project_second_half_masked(u, v, w, p, div);
        else
            project_second_half(u, v, w, p, div, false);
        note_solve(SF_PRESSURE_CG, st.status, st.iterations, st.rho0 == 0.0 ? 0.0 : std::sqrt(st.last / st.rho0));
    }

    // ---- external forces (SPEC §8) ------------------------------------------------------------------------------
    sfk::ForceArgs<T> force_args(const Launch& L) const {
        const T Nf = (T)N_;
        const T h = T(1) / Nf;
        sfk::ForceArgs<T> A{};
        A.c_grad = T(0.5) * Nf;
        A.eps_h = eps_ * h;
        A.beta = beta_;
        A.amb = amb_;
        A.tiny = (T)1e-20;
        A.axis = axis_;
        A.split = L.split;
        A.gap = L.gap;
        A.wpr = ceil_div(N_, 64);
        return A;
    }
    unsigned force_blocks(int nplanes) const { return (unsigned)ceil_div((long)ceil_div(N_, 64) * N_ * nplanes, 4L); }

    // pass A: mag = |curl(u, v, w)| on the owned planes with its shells, then its ghost planes
    void op_vorticity(int u, int v, int w, int mag) {
        for (Slab& sl : slabs_)
            for (int f : {u, v, w, mag}) ensure(sl, f);
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            acc.push_back({sl.field[u], false, a - 1, b_ + 1});
            acc.push_back({sl.field[v], false, a - 1, b_ + 1});
            acc.push_back({sl.field[w], false, a, b_});
            acc.push_back({sl.field[mag], true, lo, hi});
        };
        for_planes("vorticity", accesses, [&](const Launch& L) {
            sfk::ForceArgs<T> A = force_args(L);
            A.u = L.sl.field[u];
            A.v = L.sl.field[v];
            A.w = L.sl.field[w];
            A.mag = L.sl.field[mag];
            launch_k(L, sfk::vorticity_mag_kernel<T>, dim3(force_blocks(L.ke - L.kb)), 256u, A);
        });
        const int m[1] = {mag};
        exchange<1>(m);
    }

    template <bool VORT, bool BUOY, bool BOUND>
    void launch_forces(const Launch& L, const sfk::ForceArgs<T>& A) {
        launch_k(L, sfk::add_forces_kernel<T, VORT, BUOY, BOUND>, dim3(force_blocks(L.ke - L.kb)), 256u, A);
    }

    // add_forces(u, v, w, dens, src -> dst): dst_a = src_a + f_a on interior cells, src's shells copied where dst is
    // another slot (bound sources), then the ghost planes of dst. |curl u| lives in scratch[0] meanwhile (MAG_SLOT).
    void op_add_forces(int u, int v, int w, int dens, const int (&src)[3], const int (&dst)[3]) {
        const bool vort = eps_ != T(0), buoy = beta_ != T(0);
        if (!vort && !buoy) return;
        const bool bound = src[0] != dst[0] || src[1] != dst[1] || src[2] != dst[2];
        for (Slab& sl : slabs_) {
            for (int f : {u, v, w, dens}) ensure(sl, f);
            for (int a = 0; a < 3; ++a) {
                ensure(sl, src[a]);
                ensure(sl, dst[a]);
            }
        }
        ScratchAlias mag_slot(slabs_, vort ? 1 : 0);
        if (vort) op_vorticity(u, v, w, MAG_SLOT);
        auto accesses = [&](Slab& sl, int a, int b_, int lo, int hi, std::vector<Acc>& acc) {
            if (vort) {
                acc.push_back({sl.field[u], false, a - 1, b_ + 1});
                acc.push_back({sl.field[v], false, a - 1, b_ + 1});
                acc.push_back({sl.field[w], false, a, b_});
                acc.push_back({sl.field[MAG_SLOT], false, a - 1, b_ + 1});
            }
            if (buoy) acc.push_back({sl.field[dens], false, a, b_});
            for (int c = 0; c < 3; ++c) {
                const bool copy = src[c] != dst[c];  // shells copied too (wall planes on the end slabs)
                if (!(vort || copy || c == axis_)) continue;
                acc.push_back({sl.field[src[c]], false, copy ? lo : a, copy ? hi : b_});
                acc.push_back({sl.field[dst[c]], true, copy ? lo : a, copy ? hi : b_});
            }
        };
        for_planes("add_forces", accesses, [&](const Launch& L) {
            Slab& sl = L.sl;
            sfk::ForceArgs<T> A = force_args(L);
            A.u = sl.field[u];
            A.v = sl.field[v];
            A.w = sl.field[w];
            A.mag = vort ? sl.field[MAG_SLOT] : nullptr;
            A.dens = sl.field[dens];
            for (int a = 0; a < 3; ++a) {
                A.src[a] = sl.field[src[a]];
                A.dst[a] = sl.field[dst[a]];
            }
            if (vort && buoy)
                bound ? launch_forces<true, true, true>(L, A) : launch_forces<true, true, false>(L, A);
            else if (vort)
                bound ? launch_forces<true, false, true>(L, A) : launch_forces<true, false, false>(L, A);
            else
                bound ? launch_forces<false, true, true>(L, A) : launch_forces<false, true, false>(L, A);
        });
        // the sources' ghost planes: the fused first sweep of diffuse evaluates on the first ghost plane and reads x0
        // and the initial iterate there (see op_project)
        exchange<3>(dst);
    }

    // ---- volume rendering and light marching (SPEC §12) ----------------------------------------------------------
    // How the image pair of the slab below (d = 0) / above (d = 1) of local slab s reaches it when a k-ray crosses that
    // boundary: the routes of the tracer records (tr_side), except that a loopback context has nobody to receive from
    // and starts its rays afresh.
    int ray_side(int s, int d) const {
        const int side = tr_side(s, d);
        return (side == TR_MSG && loopback_) ? (int)TR_NONE : side;
    }
    // the k-rays of direction `high` end in local slab s (the last slab of the grid, or of a loopback context)
    bool ray_leaves_here(int s, int high) const { return ray_side(s, high ? 0 : 1) == TR_NONE; }

    template <int MODE>
    void launch_rays(Slab& sl, int axis, int high, const sfk::RayArgs<T>& A) {
        const unsigned wpr = (unsigned)ceil_div(N_, 64);
        if (axis == 2)
            hipLaunchKernelGGL((sfk::ray_march_kernel<T, 2, MODE>), dim3(wpr * N_), dim3(64), 0, sl.cs, sl.geom, A);
        else if (axis == 1)
            hipLaunchKernelGGL((sfk::ray_march_kernel<T, 1, MODE>), dim3(wpr * nzl_), dim3(64), 0, sl.cs, sl.geom, A);
        else if (high)
            hipLaunchKernelGGL((sfk::ray_row_kernel<T, MODE, true>), dim3(wpr * nzl_), dim3(64), 0, sl.cs, sl.geom, A);
        else
            hipLaunchKernelGGL((sfk::ray_row_kernel<T, MODE, false>), dim3(wpr * nzl_), dim3(64), 0, sl.cs, sl.geom, A);
        SF_HIP(hipGetLastError());
    }

    // The image pair [w] of every slab (cnt values) and, where the pair of the slab before it arrives as a message, the
    // buffer it arrives in: allocated on first use, as zeros.
    void ray_buffers(int w, size_t cnt, bool chain, int high) {
        for (int s = 0; s < L_; ++s) {
            Slab& sl = slabs_[s];
            for (T** buf : {&sl.ray_img[w], (chain && ray_side(s, high ? 1 : 0) == TR_MSG) ? &sl.ray_in[w] : nullptr}) {
                if (!buf || *buf) continue;
                *buf = own_.dev<T>(cnt * sizeof(T));
                SF_HIP(hipMemset(*buf, 0, cnt * sizeof(T)));
                SF_HIP(hipDeviceSynchronize());  // (as alloc_field: the streams do not order against the null stream)
            }
        }
    }

    // One march over every slab, on its compute stream: march(sl, in) launches it and traces it; `in` is the image pair
    // the march starts from (null: the rays start here). Without a chain the slabs run side by side. With one the rays
    // cross the slabs in visit order (downwards when `high`): a slab starts from the pair [w] (cnt values) the one before
    // it left — read in place when that slab is in this process, a message otherwise (to self through the communicator
    // with SF_FLAG_RCCL_SELF) — so the chain has P stages. At the end every compute stream has waited for the last
    // stage: the next march may overwrite any pair. With `resume` a slab that has nobody to receive from starts from
    // the pair [w] it holds itself (the second pass of §14, after a chain the other way ended there) and march() reads
    // and writes that one buffer.
    template <class MarchF>
    void ray_chain(int w, size_t cnt, bool chain, int high, MarchF march, bool resume = false) {
        const ncclDataType_t dt = sizeof(T) == 4 ? ncclFloat : ncclDouble;
        for (int n = 0; n < L_; ++n) {
            const int s = (chain && high) ? L_ - 1 - n : n;  // rays from the high side visit the slabs downwards
            Slab& sl = slabs_[s];
            const T* in = nullptr;
            if (chain) {
                const int from = high ? 1 : 0, side = ray_side(s, from);
                Slab* prev = (high ? s < L_ - 1 : s > 0) ? &slabs_[s + (high ? 1 : -1)] : nullptr;
                if (side != TR_NONE && prev) st_wait(sl, sl.cs, *prev, &Slab::cs_mark);
                if (side == TR_LOCAL) {
                    in = prev->ray_img[w];
                } else if (side == TR_MSG) {
                    SF_NCCL(ncclGroupStart());
                    if (prev) {  // SF_FLAG_RCCL_SELF: the pair (send from the slab the rays left, receive here)
                        SF_NCCL(ncclSend(prev->ray_img[w], cnt, dt, 0, comm_, prev->cs));
                        SF_NCCL(ncclRecv(sl.ray_in[w], cnt, dt, 0, comm_, sl.cs));
                    } else {
                        SF_NCCL(ncclRecv(sl.ray_in[w], cnt, dt, rank_ + (high ? 1 : -1), comm_, sl.cs));
                    }
                    SF_NCCL(ncclGroupEnd());
                    ++rccl_groups_;
                    if (trace_) {
                        std::vector<Acc> acc{{sl.ray_in[w], true, 0, nplanes_}};
                        if (prev) acc.push_back({prev->ray_img[w], false, 0, nplanes_});
                        tr_op(prev ? "rays_carry_rccl_self" : "rays_carry_recv", sl, sl.cs, acc);
                    }
                    in = sl.ray_in[w];
                } else if (resume) {
                    in = sl.ray_img[w];
                }
            }
            march(sl, in);
            if (!chain) continue;
            if (L_ > 1) ev_record(sl, &Slab::cs_mark, sl.cs);
            if (nranks_ > 1 && !loopback_ && !ray_leaves_here(s, high) && tr_side(s, high ? 0 : 1) == TR_MSG) {
                SF_NCCL(ncclGroupStart());
                SF_NCCL(ncclSend(sl.ray_img[w], cnt, dt, rank_ + (high ? -1 : 1), comm_, sl.cs));
                SF_NCCL(ncclGroupEnd());
                ++rccl_groups_;
                tr_op("rays_carry_send", sl, sl.cs, {{sl.ray_img[w], false, 0, nplanes_}});
            }
        }
        if (chain && L_ > 1) {
            Slab& last = slabs_[high ? 0 : L_ - 1];
            for (Slab& sl : slabs_)
                if (&sl != &last) st_wait(sl, sl.cs, last, &Slab::cs_mark);
        }
    }

    // The marches of §12. Rays along i and j stay inside a plane: the slabs run side by side and each writes the pixel
    // rows of its planes. Rays along k go through the chain.
    void op_rays(int mode, int axis, int high, double sigma, int dens, int emit, int dst) {
        const int w = mode == sfk::RAY_FIELD ? 1 : 0;
        const size_t cnt = 2 * (size_t)N_ * N_;
        const bool chain = axis == 2 && P_ > 1;
        for (Slab& sl : slabs_)
            for (int f : {dens, emit, dst})
                if (f >= 0) ensure(sl, f);
        ray_buffers(w, cnt, chain, high);
        join();
        const T h = T(1) / (T)N_;
        const int kb = G_, ke = G_ + nzl_;
        const char* names[3][3] = {{"render_i", "render_j", "render_k"},
                                   {"render_emit_i", "render_emit_j", "render_emit_k"},
                                   {"light_i", "light_j", "light_k"}};
        ray_chain(w, cnt, chain, high, [&](Slab& sl, const T* in) {
            sfk::RayArgs<T> A{};
            A.dens = sl.field[dens];
            A.emit = emit >= 0 ? sl.field[emit] : nullptr;
            A.dst = dst >= 0 ? sl.field[dst] : nullptr;
            A.img = sl.ray_img[w];
            A.s = (T)sigma * h;
            A.from_high = high;
            A.in = in;
            switch (mode) {
                case sfk::RAY_IMAGE: launch_rays<sfk::RAY_IMAGE>(sl, axis, high, A); break;
                case sfk::RAY_IMAGE_EMIT: launch_rays<sfk::RAY_IMAGE_EMIT>(sl, axis, high, A); break;
                default: launch_rays<sfk::RAY_FIELD>(sl, axis, high, A); break;
            }
            if (trace_) {
                std::vector<Acc> acc{{A.dens, false, kb, ke}, {A.img, true, 0, nplanes_}};
                if (A.emit) acc.push_back({A.emit, false, kb, ke});
                if (A.dst) acc.push_back({A.dst, true, kb, ke});
                if (A.in) acc.push_back({A.in, false, 0, nplanes_});
                tr_op(names[mode][axis], sl, sl.cs, acc);
            }
        });
    }

    // The image pair [2] holds cnt values from here on: a pair of another size goes, once the device is done with it.
    void view_resize(size_t cnt) {
        if (cnt == view_cnt_) return;
        for (Slab& sl : slabs_) SF_HIP(hipStreamSynchronize(sl.cs));
        for (Slab& sl : slabs_) {
            own_.release(sl.ray_img[2]);
            own_.release(sl.ray_in[2]);
        }
        view_cnt_ = cnt;
        view_w_ = view_h_ = 0;  // no image to read until this render has been issued
    }

    // The march of §13: every slab applies the samples it owns of every ray, in the chain's order — upwards when
    // T(step_z) >= 0, downwards otherwise. A sample reads the planes k0 and k0 + 1: the slab's interior planes, the
    // ghost plane above them and, on slab 0, the shell plane below (all current after every operator, §10).
    void op_view(const sf_view_params& p) {
        const int mode = p.emit >= 0 ? sfk::RAY_IMAGE_EMIT : sfk::RAY_IMAGE;
        const size_t cnt = 2 * (size_t)p.width * p.height;
        const bool chain = P_ > 1;
        const int high = (T)p.step[2] < T(0) ? 1 : 0;
        for (Slab& sl : slabs_)
            for (int f : {p.dens, p.emit})
                if (f >= 0) ensure(sl, f);
        view_resize(cnt);
        ray_buffers(2, cnt, chain, high);
        join();
        const int kb = G_, ke = G_ + nzl_;
        const unsigned tiles = (unsigned)(ceil_div(p.width, 8) * ceil_div(p.height, 8));
        ray_chain(2, cnt, chain, high, [&](Slab& sl, const T* in) {
            sfk::ViewArgs<T> A{};
            A.dens = sl.field[p.dens];
            A.emit = p.emit >= 0 ? sl.field[p.emit] : nullptr;
            A.in = in;
            A.img = sl.ray_img[2];
            for (int c = 0; c < 3; ++c) A.o[c] = (T)p.origin[c], A.du[c] = (T)p.du[c], A.dv[c] = (T)p.dv[c], A.ds[c] = (T)p.step[c];
            A.s = (T)p.sigma * (T(1) / (T)N_);
            A.width = p.width, A.height = p.height, A.samples = p.samples;
            if (mode == sfk::RAY_IMAGE_EMIT)
                hipLaunchKernelGGL((sfk::view_march_kernel<T, sfk::RAY_IMAGE_EMIT>), dim3(tiles), dim3(64), 0, sl.cs, sl.geom, A);
            else
                hipLaunchKernelGGL((sfk::view_march_kernel<T, sfk::RAY_IMAGE>), dim3(tiles), dim3(64), 0, sl.cs, sl.geom, A);
            SF_HIP(hipGetLastError());
            if (trace_) {
                const int lo = sl.geom.wall_lo ? kb - 1 : kb;
                std::vector<Acc> acc{{A.dens, false, lo, ke + 1}, {A.img, true, 0, nplanes_}};
                if (A.emit) acc.push_back({A.emit, false, lo, ke + 1});
                if (A.in) acc.push_back({A.in, false, 0, nplanes_});
                tr_op(A.emit ? "render_view_emit" : "render_view", sl, sl.cs, acc);
            }
        });
        view_w_ = p.width, view_h_ = p.height, view_high_ = high;
    }

    // The march of §14 into the pair of §13. The corner rule names the chains: one, as §13's, when every pixel's rays
    // climb or every pixel's descend; else an upward chain that applies the up pixels and a downward one, resumed from
    // the pair the upward chain left on the last slab, that applies the down pixels. Either hands the whole pair on.
    // Without a chain (one slab) a single launch applies every pixel.
    void op_camera(const sf_camera_params& c, int passes) {
        const sf_view_params& p = c.view;
        const int mode = p.emit >= 0 ? sfk::RAY_IMAGE_EMIT : sfk::RAY_IMAGE;
        const size_t cnt = 2 * (size_t)p.width * p.height;
        const bool chain = P_ > 1;
        for (Slab& sl : slabs_)
            for (int f : {p.dens, p.emit})
                if (f >= 0) ensure(sl, f);
        view_resize(cnt);
        for (int high = 0; high < 2; ++high)
            if (passes == SF_CAMERA_BOTH || passes == high) ray_buffers(2, cnt, chain, high);
        join();
        const int kb = G_, ke = G_ + nzl_;
        const unsigned tiles = (unsigned)(ceil_div(p.width, 8) * ceil_div(p.height, 8));
        static const char* names[2][3] = {{"render_camera_up", "render_camera_down", "render_camera_both"},
                                          {"render_camera_emit_up", "render_camera_emit_down", "render_camera_emit_both"}};
        for (int high = 0; high < 2; ++high) {
            if (passes != SF_CAMERA_BOTH && passes != high) continue;
            const int pass = !chain ? (int)sfk::CAMERA_BOTH : passes == SF_CAMERA_BOTH ? high : (int)sfk::CAMERA_BOTH;
            ray_chain(2, cnt, chain, high, [&](Slab& sl, const T* in) {
                sfk::CameraArgs<T> A{};
                A.dens = sl.field[p.dens];
                A.emit = p.emit >= 0 ? sl.field[p.emit] : nullptr;
                A.in = in;
                A.img = sl.ray_img[2];
                for (int x = 0; x < 3; ++x) {
                    A.o[x] = (T)p.origin[x], A.du[x] = (T)p.du[x], A.dv[x] = (T)p.dv[x], A.ds[x] = (T)p.step[x];
                    A.dsu[x] = (T)c.step_du[x], A.dsv[x] = (T)c.step_dv[x];
                }
                A.sh = (T)p.sigma * (T(1) / (T)N_);
                A.width = p.width, A.height = p.height, A.samples = p.samples, A.pass = pass;
                if (mode == sfk::RAY_IMAGE_EMIT)
                    hipLaunchKernelGGL((sfk::camera_march_kernel<T, sfk::RAY_IMAGE_EMIT>), dim3(tiles), dim3(64), 0, sl.cs, sl.geom, A);
                else
                    hipLaunchKernelGGL((sfk::camera_march_kernel<T, sfk::RAY_IMAGE>), dim3(tiles), dim3(64), 0, sl.cs, sl.geom, A);
                SF_HIP(hipGetLastError());
                if (trace_) {
                    const int lo = sl.geom.wall_lo ? kb - 1 : kb;
                    std::vector<Acc> acc{{A.dens, false, lo, ke + 1}, {A.img, true, 0, nplanes_}};
                    if (A.emit) acc.push_back({A.emit, false, lo, ke + 1});
                    if (A.in) acc.push_back({A.in, false, 0, nplanes_});  // (the resumed stage: the buffer just named)
                    tr_op(names[A.emit ? 1 : 0][pass], sl, sl.cs, acc);
                }
            }, chain && passes == SF_CAMERA_BOTH && high == 1);
            if (!chain) break;  // one slab: the single launch has applied every pixel
        }
        view_w_ = p.width, view_h_ = p.height, view_high_ = passes == SF_CAMERA_UP ? 0 : 1;
    }

    // Communicator guard: destroyed before own_ (declared after it), so before the streams its calls were issued on.
    struct Comm {
        ncclComm_t h = nullptr;
        Comm() = default;
        Comm(const Comm&) = delete;
        Comm& operator=(const Comm&) = delete;
        ~Comm() {
            if (h) ncclCommDestroy(h);
        }
        operator ncclComm_t() const { return h; }
    };

    int N_, K_, device_;
    Owned own_;  // every device and pinned block, stream and event of this context; before all that refer to them
    Comm comm_;
    int L_ = 1, nranks_ = 1, rank_ = 0, P_ = 1, G_ = 1;
    const Switches sw_{};
    int fuse_maxvec_ = 512;  // widest row (vectors) the fused kernels take
    int trap_m_ = 4, split_fields_ = 1, tuned_trap_ = -1, tuned_split_ = -1;
    int bound_[4] = {-1, -1, -1, -1};  // resident source slots (sf_bind_sources)
    bool pending_join_ = false, graphs_ = false;
    std::vector<GraphEntry> graph_cache_;
    T dt_{}, diff_{}, visc_{};
    T eps_{}, beta_{}, amb_{};  // forces of SPEC §8 (0: off)
    int axis_ = 1;
    int mc_vel_ = SF_ADVECT_SEMI_LAGRANGIAN, mc_dens_ = SF_ADVECT_SEMI_LAGRANGIAN;  // advection schemes (SPEC §9)
    int pressure_ = SF_PRESSURE_JACOBI, cg_max_iters_ = 100;  // what vel_step's projections run (SPEC §11)
    double cg_tol_ = 1e-3;
    int check_every_ = 0, host_waits_ = 0;  // sf_set_pressure_sync; host waits of the last CG projection
    int precond_ = SF_PRECOND_NONE, precond_sweeps_ = 0;  // sf_set_pressure_preconditioner (SPEC §11.2)
    int mg_nu_ = 0, mg_maxl_ = 0, mg_nuc_ = 8;            // sf_set_pressure_multigrid (SPEC §11.3); nu = 0: off
    bool obst_tr_ = false;      // sf_set_obstacle_transport (SPEC §17): with obstacles on, diffuse and advect are masked
    bool obst_mc_ = false;      // sf_set_obstacle_maccormack (SPEC §18): MacCormack under masked transport runs, masked
    bool obst_mg_ = false;      // sf_set_obstacle_multigrid (SPEC §16): a masked solve under the V-cycle runs, masked
    bool mg_codes_ok_ = false;  // the face codes of the coarse levels match the mask and the levels in force
    bool obstv_on_ = false;   // sf_set_obstacle_velocity (SPEC §19): the solid velocity of the OBSTV slots is in force
    bool obst_on_ = false;    // sf_set_obstacles (SPEC §15): the face codes of OBST_SLOT are in force
    long long n_fluid_ = 0;   // fluid interior cells under them
    long long host_waits_total_ = 0;
    sf_pressure_info info_{SF_PRESSURE_JACOBI, SF_CG_MAX_ITERS, 0, -1.0, 0, 0};  // the last projection
    int num_cu_ = 256;
    int nzl_ = 0, lead_ = 0, px_ = 0, nplanes_ = 0;
    bool dead_ishell_opt_ = true;   // SF_ISHELL=2 switches the dead-shell elision off (1: on, 0: every sweep writes it)
    bool ishell_skip_ = true;
    long sk2_min_cells_ = 60000000;  // smallest launch a TWO-sweep marching pass takes (launch_pass)
    long plane_ = 0, field_elems_ = 0, pad_front_ = 0, pad_back_ = 0;
    Level lv0_;  // the solver-wide geometry above as a Level: the default of every function that takes one
    std::vector<Slab> slabs_;
    FILE* trace_ = nullptr;  // SF_TRACE_SCHEDULE
    bool inject_trap_bug_ = false;
    std::map<const void*, int> buf_ids_;
    long xchg_seq_ = 0;
    bool loopback_ = false, rccl_self_ = false;
    long rccl_groups_ = 0;  // RCCL send/recv groups issued so far (sf_schedule_info: proof the transport ran)
    hipEvent_t t0_ = nullptr, t1_ = nullptr;
    T* tr_pos_ = nullptr;
    T* tr_dens_ = nullptr;
    T* tr_speed_ = nullptr;
    int tr_n_ = 0, snap_count_ = 0;
    // decomposed tracers: dense id-indexed output / owned-order id output, the list of the ping-pong pair in use, the
    // send capacity in force and the one asked for (sf_tracers_set_capacity; <= 0: the tracer count)
    int* tr_ids_ = nullptr;
    int tr_cur_ = 0, tr_cap_ = 0, tr_cap_req_ = 0;
    void* copy_src_ = nullptr;
    void* copy_dst_ = nullptr;
    size_t copy_bytes_ = 0;
    double* red_host_ = nullptr;    // pinned: the plane records of all N planes ([global k - 1][value])
    double* red_gather_ = nullptr;  // device: the same, the all-gather's buffer (contexts with a communicator) and what
                                    // cg_scalars_kernel folds (any context with check_every_ >= 1)
    T* ray_stage_ = nullptr;         // pinned: the image pair on its way to the caller (sf_render_read)
    int ray_axis_ = -1, ray_high_ = 0;  // view of the last sf_render (-1: none yet)
    size_t view_cnt_ = 0;                     // values of the image pair of sf_render_view now allocated
    int view_w_ = 0, view_h_ = 0, view_high_ = 0;  // frame of the last sf_render_view (width 0: none yet)
    sfk::CgState<T>* cg_state_ = nullptr;       // device: the scalars of a CG solve (check_every_ >= 1)
    sfk::CgState<T>* cg_state_host_ = nullptr;  // pinned: its mirror, filled by cg_state_read()
};

}  // namespace sfi
