// C ABI of libschpf_hip.so (include/schpf_hip.h): context management and the ordering of kernel launches that makes one
// CAVI iteration (scHPF_.py:657-714).  The matrix an engine holds and the uploads that build it: engine.h, upload.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

#include "engine.h"
#include "kernels.h"

using namespace schpf;

thread_local std::string schpf::g_err;

namespace {

// The model state the engine holds once per matrix axis, allocated at schpf_create and never again (captured graphs bake
// the DevBuf::p pointers in).  Engine::side[0] is the cell axis (major = cell: xi, theta), side[1] the gene axis (eta,
// beta) -- the numbering of Matrix::axis, run_sweep, loss_side, order_of and the policy.
struct Side {
    int n = 0;                         // rows of this axis: N / G
    DevBuf cap_shape, cap_rate;        // xi / eta                            [n]
    DevBuf shape, rate;                // theta / beta (C-contiguous)         [n, K]
    DevBuf tab_exp, tab_e, tab_log;    // tables, padding columns zero        [n, KP]
    DevBuf colpart;                    // the update kernel's column partials double[UPD_BLOCKS * K]
    bool dirty = true;                 // the tables and column sums are older than the parameters
};

struct ScopedTimer {
    Profiler &p; hipStream_t st; int kind; hipEvent_t a{}, b{};
    ScopedTimer(Profiler &p_, hipStream_t st_, int kind_) : p(p_), st(st_), kind(kind_)
    {
        if (p.on) { a = p.get(); b = p.get(); HIPCHK(hipEventRecord(a, st)); }
    }
    void stop()
    {
        if (p.on) { HIPCHK(hipEventRecord(b, st)); p.recs.push_back({kind, a, b}); }
    }
};

template <typename T> struct Engine final : Uploader {
    Side side[2];                                   // 0: cells, 1: genes.  Below: what exists once, or for one axis only
    DevBuf exchange_buf;                            // gene side: [G*K + K] of T, the sums a sharded fit all-reduces + K sums of E[theta]
    DevBuf dense_cell;                              // cell side: [N*K] of T (t = 0 only; the genes' twin is the exchange buffer)
    DevBuf s_theta, s_beta, s_beta_next;            // double[K] column sums of E[theta], E[beta]; beta's double-buffered (beta_parity)
    DevBuf scalars;                                 // scalars[0]=llh sum
    // the loss pass's two results land in pinned host memory that the device writes directly: the reduction kernels
    // store there, the host reads after the stream has drained -- no copy of 24 bytes out of pageable memory per check
    double *loss_host = nullptr;
    DevBuf dual_queue;                              // persistent dual launch: {next slot, workgroups done}, self-zeroing
    DevBuf clock_probe;                             // 5 x u64: shader cycles, constant-rate ticks, 2 start stamps, launches (sweep_impl.h)
    DevBuf elbo_part, elbo_sums;                    // ELBO: Gamma-term block partials, their sums (elbo_terms)
    DevBuf ppc_e[2], ppc_out;                       // predictive_rows: E of each side as doubles; [zeros | rate | rate2] of an axis
    int beta_parity = 0;               // swaps of the sum-of-beta buffers mod 2: which cached graph fits (schpf_ctx::graphs)
    // small problems: the update kernels sum the other side's per-block column sums themselves and the
    // two reduce launches of an iteration are skipped; s_theta / s_beta are then brought up to date
    // only when a path that reads them comes along (sums_stale)
    bool sums_stale = false;
    static constexpr int UPD_BLOCKS = 2048;
    static constexpr size_t TABLE_PAD = 256 * 1024;

    Engine(int device_, void *stream_, int dtype_, int N_, int G_, int K_) : Uploader(sizeof(T))
    {
        device = device_; dtype = dtype_; N = N_; G = G_; K = K_;
        HIPCHK(hipSetDevice(device));
        // NULL: a stream of our own; SCHPF_STREAM_DEFAULT: the device's null stream (what
        // torch.cuda.current_stream() is unless the caller switched streams); else the given handle
        if (stream_ == SCHPF_STREAM_DEFAULT) stream = nullptr;
        else if (stream_) stream = (hipStream_t)stream_;
        else { HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
        {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
                cu_count = prop.multiProcessorCount;
        }
        const schpf::Config cfg = schpf::choose_config(K, (int)sizeof(T), tuning);
        want_tile = cfg.tile; LPC = cfg.LPC; NV = cfg.NV; KL = cfg.KL; KP = cfg.KP;
        const size_t s = sizeof(T);
        dual_queue.alloc(2 * sizeof(int), true, stream);
        clock_probe.alloc(8 * sizeof(unsigned long long), true, stream);
        side[0].n = N; side[1].n = G;
        for (Side &sd : side) {
            const size_t n = (size_t)sd.n;
            sd.cap_shape.alloc(n * s); sd.cap_rate.alloc(n * s);
            sd.shape.alloc(n * K * s); sd.rate.alloc(n * K * s);
            // + TABLE_PAD zero bytes: slack behind the last row for whole-piece copies
            for (DevBuf *b : {&sd.tab_exp, &sd.tab_e, &sd.tab_log}) b->alloc(n * KP * s + TABLE_PAD, true, stream);
            sd.colpart.alloc((size_t)UPD_BLOCKS * K * sizeof(double));
        }
        exchange_buf.alloc(((size_t)G * K + K) * s, true, stream);
        for (DevBuf *b : {&s_theta, &s_beta, &s_beta_next}) b->alloc((size_t)K * sizeof(double), true, stream);
        scalars.alloc(8 * sizeof(double), true, stream);
        if (hipHostMalloc((void **)&loss_host, 8 * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            loss_host = nullptr;            // falls back to the copy out of `scalars`
        } else std::memset(loss_host, 0, 8 * sizeof(double));
    }
    // the hyper-parameters stay where the C ABI sets them (schpf_ctx)
    double prior_shape(int s) const { return s == 0 ? a : c; }
    double cap_prior_rate(int s) const { return s == 0 ? bp : dp; }   // of the side's capacities (xi / eta)
    // an iteration would do nothing that must happen only once: a stretch of them may be captured as a graph
    bool steady() const
    {
        return !prof.on && stream != nullptr && pending_init == 0 && eager_since_upload && !side[0].dirty && !side[1].dirty;
    }
    // the graph of `count` (even) iterations issued by `body` for the current parity: cached or captured now
    template <typename F> hipGraphExec_t graph_for(unsigned key_flags, int count, F &&body)
    {
        CachedGraph &g = graphs[beta_parity & 1];
        if (g.exec && g.flags == key_flags && g.n == count) return g.exec;
        if (g.exec) { (void)hipStreamSynchronize(stream); (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; g.n = 0; }
        hipGraph_t graph = nullptr;
        HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        try {
            body(count);   // runs the host side of `count` iterations (an even number of swaps) without executing them
        } catch (...) {
            (void)hipStreamEndCapture(stream, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        HIPCHK(hipStreamEndCapture(stream, &graph));
        const hipError_t e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HIPCHK(e);
        g.flags = key_flags;
        g.n = count;
        return g.exec;
    }

    // One stretch of n iterations issued by body(count).  A graphable stretch replays its even part as the graph cached
    // under `key` for the current parity (captured on first use); what is left runs eagerly
    template <typename F> void stretch(unsigned key, int n, bool graphable, F &&body)
    {
        int done = 0;
        if (graphable && n >= 2) {
            done = n & ~1;
            HIPCHK(hipGraphLaunch(graph_for(key, done, body), stream));
        }
        body(n - done);
        if (n > 0) eager_since_upload = true;
    }

    // n iterations of schpf_step.  From the second call on with the same (flags, n) they are one
    // graph launch: launch overhead is what bounds small matrices (BASELINE C2: five launches of
    // 5-25 us each per iteration).  The sum-of-beta buffers swap roles every iteration, so a graph
    // always holds an even number of iterations; an odd one runs eagerly.
    void steps(unsigned flags_, int n) override
    {
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        stretch(flags_, n, tuning.graph && steady() && !(flags_ & SCHPF_SHARDED), [&](int count) {
            for (int i = 0; i < count; ++i) { step_local(flags_); step_finish(flags_); }
        });
    }

    // n iterations with the cells sharded over the ranks of `comm` (sharded.py protocol, driven from
    // here): gene-side sweep + packing on the context's stream; ONE all-reduce of [G*K sums | K sums
    // of E[theta]] on the communicator's stream, ordered after the packing by an event; the
    // cell-side sweep meanwhile; the update kernels after an event on the all-reduce.  No host
    // round trip and no Python between the launches of an iteration.
    void steps_sharded(unsigned flags_, int n) override
    {
        if (!comm) throw std::logic_error("no communicator (schpf_comm_init)");
        const unsigned base = (flags_ | SCHPF_SHARDED) & ~(unsigned)(SCHPF_LOCAL_GENE | SCHPF_LOCAL_CELL);
        const bool freeze = flags_ & SCHPF_FREEZE_GENES;
        const int dt = sizeof(T) == 4 ? 7 : 8;   // ncclFloat32 / ncclFloat64
        auto iterate = [&](int count) {
        for (int i = 0; i < count; ++i) {
            if (freeze) { step_local(base); step_finish(base); continue; }   // nothing to exchange
            step_local(base | SCHPF_LOCAL_GENE);
            HIPCHK(hipEventRecord(ev_packed, stream));
            HIPCHK(hipStreamWaitEvent(comm_stream, ev_packed, 0));
            RCCLCHK(rccl().AllReduce(exchange_buf.p, exchange_buf.p, (size_t)G * K + K, dt, 0, comm, comm_stream));
            HIPCHK(hipEventRecord(ev_reduced, comm_stream));
            step_local(base | SCHPF_LOCAL_CELL);
            HIPCHK(hipStreamWaitEvent(stream, ev_reduced, 0));
            step_finish(base);
        }
        };
        // The stretch as one hipGraph -- both streams, the events between them and the RCCL all-reduce captured (RCCL
        // supports stream capture): 0.183 -> 0.168 ms per iteration of a 1/8 shard of C3.  The default for a one-rank
        // communicator, which is all this build could ever run it with; with more ranks every rank must replay the same
        // graph, so there it stays opt-in (SCHPF_GRAPH_SHARDED=1) until tests/test_multigpu.py has seen two GPUs.
        stretch(base | 0x80000000u, n, tuning.graph_sharded.value_or(comm_world == 1) && steady() && !freeze, iterate);
    }

    // loss terms summed over the ranks (three doubles through the same communicator)
    void loss_terms_all(double *llh, double *gl, int64_t *nnz_out) override
    {
        if (!comm) throw std::logic_error("no communicator (schpf_comm_init)");
        double h[3];
        int64_t local_nnz = 0;
        loss_terms(&h[0], &h[1], &local_nnz);
        h[2] = (double)local_nnz;
        double *d = scalars.as<double>() + 4;
        HIPCHK(hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, stream));
        RCCLCHK(rccl().AllReduce(d, d, 3, 8, 0, comm, stream));
        HIPCHK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        *llh = h[0]; *gl = h[1]; *nnz_out = (int64_t)(h[2] + 0.5);
    }

    ~Engine() override
    {
        drop_graphs();
        (void)hipStreamSynchronize(stream);
        if (loss_host) (void)hipHostFree(loss_host);
        if (own_stream) (void)hipStreamDestroy(stream);
    }

    // Row and column sums of the matrix the engine holds: the ELBO's count sums (loss_constants), N + G doubles
    void marginals(double *row_sums, double *col_sums) override
    {
        need_coo();
        need_loss_constants();
        double *const out[2] = {row_sums, col_sums};
        for (int s = 0; s < 2; ++s)
            if (out[s]) HIPCHK(hipMemcpyAsync(out[s], mx.axis[s].count.p, (size_t)side[s].n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    // SCHPF_XI / THETA / ETA / BETA -> the side's capacity (xi, eta) or loading (theta, beta) buffer
    static int axis_of(int which) { return which == SCHPF_ETA || which == SCHPF_BETA; }
    static bool is_loading(int which) { return which == SCHPF_THETA || which == SCHPF_BETA; }
    DevBuf &state_buf(int which, bool rate)
    {
        if (which < SCHPF_XI || which > SCHPF_BETA) throw std::invalid_argument("which must be SCHPF_XI/THETA/ETA/BETA");
        Side &sd = side[axis_of(which)];
        if (is_loading(which)) return rate ? sd.rate : sd.shape;
        return rate ? sd.cap_rate : sd.cap_shape;
    }
    size_t state_bytes(int which) const
    {
        return (size_t)side[axis_of(which)].n * (is_loading(which) ? (size_t)K : 1) * sizeof(T);
    }
    void set_state(int which, const void *shape, const void *rate, bool dev) override
    {
        const size_t b = state_bytes(which);
        const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (shape) HIPCHK(hipMemcpyAsync(state_buf(which, false).p, shape, b, kind, stream));
        if (rate) HIPCHK(hipMemcpyAsync(state_buf(which, true).p, rate, b, kind, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (is_loading(which)) side[axis_of(which)].dirty = true;
        // the graph reads the parameters through fixed pointers: still valid; only xi/eta shapes are constants
    }
    void get_state(int which, void *shape, void *rate, bool dev) override
    {
        const size_t b = state_bytes(which);
        const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (shape) HIPCHK(hipMemcpyAsync(shape, state_buf(which, false).p, b, kind, stream));
        if (rate) HIPCHK(hipMemcpyAsync(rate, state_buf(which, true).p, b, kind, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    int rows_per_block() const { return schpf::update_rows_per_block(K); }
    int upd_blocks(int n) const
    {
        const int groups = (n + rows_per_block() - 1) / rows_per_block();
        return std::max(1, std::min(groups, (int)UPD_BLOCKS));
    }

    // what every launch of the update kernel on a side is given: its parameters, tables and column partials
    schpf::UpdateArgs<T> update_args(int s)
    {
        Side &sd = side[s];
        schpf::UpdateArgs<T> u{};
        u.n = sd.n; u.K = K; u.KP = KP; u.rows_per_block = rows_per_block();
        u.shape = sd.shape.as<T>(); u.rate = sd.rate.as<T>();
        u.tab_e = sd.tab_e.as<T>(); u.tab_log = sd.tab_log.as<T>(); u.tab_exp = sd.tab_exp.as<T>();
        u.colsum_part = sd.colpart.as<double>();
        return u;
    }
    // `out` := a side's column sums, from the block partials its update kernel left.  Not symmetric: only theta's are
    // mirrored, in the model dtype (the f32 flag), into the exchange buffer's tail, which a sharded fit all-reduces
    void reduce_colsums(int s, DevBuf &out)
    {
        void *mirror = s == 0 ? exchange_buf.as<T>() + (size_t)G * K : nullptr;
        HIPCHK(schpf::launch_colsum_reduce(side[s].colpart.as<double>(), upd_blocks(side[s].n), K, out.as<double>(), mirror,
                                           s == 0 && sizeof(T) == 4, stream));
    }

    // (re)build E, E[log], exp-shifted tables and column sums from the stored parameters: theta, then beta
    void refresh_tables()
    {
        for (int s = 0; s < 2; ++s) {
            if (!side[s].dirty) continue;
            HIPCHK(schpf::launch_gamma_update(update_args(s), schpf::SRC_NONE, upd_blocks(side[s].n), stream));
            reduce_colsums(s, s == 0 ? s_theta : s_beta);   // s_beta: the current one of the double buffer
            side[s].dirty = false;
        }
    }

    // The tables a sweep of side s reads: major = the side's own, minor = the other side's.  MODE_LLH and MODE_LLH_ROWS read the E
    // tables, every other mode the exp-shifted ones; the log tables are the same for all
    template <typename A> void table_args(A &a, int s, int mode)
    {
        const Side &mj = side[s], &mn = side[1 - s];
        const bool llh = mode == schpf::MODE_LLH || mode == schpf::MODE_LLH_ROWS;
        a.tab_major = (llh ? mj.tab_e : mj.tab_exp).template as<T>();
        a.tab_minor = (llh ? mn.tab_e : mn.tab_exp).template as<T>();
        a.log_major = mj.tab_log.template as<T>();
        a.log_minor = mn.tab_log.template as<T>();
    }

    schpf::SweepArgs<T> sweep_args(int s, int mode)
    {
        PlanDev &pd = mx.axis[s].plan;
        schpf::SweepArgs<T> a{};
        a.entries = pd.entries.as<uint4>();
        a.slice_off = pd.slice_off.as<int64_t>();
        a.slice_steps = pd.slice_steps.as<int>();
        a.chunk_major = pd.chunk_major.as<int>();
        a.chunk_natid = pd.chunk_natid.as<int>();
        a.wave_slice = pd.wave_slice.as<int>();
        table_args(a, s, mode);
        a.partials = pd.part.rows.as<T>();
        a.wave_out = mx.wave_out.as<double>();
        a.K = K;
        return a;
    }

    // tl: the side's task list the launch walks (TileDev::tasks, or llh for a cut loss pass)
    schpf::TileArgs<T> tile_args(int s, int mode, const TaskList &tl)
    {
        TileDev &td = mx.axis[s].tile;
        schpf::TileArgs<T> a{};
        a.entries = td.entries.p;
        a.steps = td.steps.as<uint16_t>();
        a.block_rows = td.block_rows.as<int>();
        a.task_block = tl.block.as<int>();
        a.task_w0 = tl.w0.as<int>();
        a.task_w1 = tl.w1.as<int>();
        a.task_stage_end = tl.stage_end.as<int>();   // nullptr for the iteration's tasks
        a.task_wave_off = tl.wave_off.as<int64_t>();
        a.task_order = nullptr;   // natural order (plan.cpp)
        table_args(a, s, mode);
        a.partials = td.part.rows.as<T>();
        a.wave_out = mx.wave_out.as<double>();
        a.K = K; a.n_minor = td.n_virtual ? td.n_virtual : side[1 - s].n; a.n_windows = td.host.n_windows; a.win_rows = td.host.win_rows;
        a.minor_of = td.n_virtual ? td.minor_of.as<int>() : nullptr;
        a.n_virtual = td.n_virtual;
        a.wpb = td.host.wpb;
        a.ring = td.host.ring; a.slot_bytes = td.host.slot16 * 16; a.sync_stage = td.host.sync_stage;
        a.single = td.host.single ? 1 : 0;
        a.clock_probe = clock_probe.as<unsigned long long>();
        a.major_is_cell = s == 0 ? 1 : 0;
        return a;
    }

    // one sweep of either plan kind.  side 0: major = cell, side 1: major = gene.
    void run_sweep(int s, int mode, uint64_t seed = 0)
    {
        if (mx.use_tile) {
            TileDev &td = mx.axis[s].tile;
            // the per-row pass keeps the iteration's own tasks: its records are addressed as their partial rows are
            const bool rows = mode == schpf::MODE_LLH_ROWS;
            const bool logs = mode == schpf::MODE_LLH || mode == schpf::MODE_ELBO || rows;   // the ELBO pass is cut as the loss pass
            const bool cut = logs && !rows && td.llh.n > 0;   // the loss pass's finer tasks (loss_tasks)
            const TaskList &tl = cut ? td.llh : td.tasks;
            auto a = tile_args(s, mode, tl);
            a.seed = seed;
            const bool persistent = mode != schpf::MODE_RANDOM && tuning.persistent;   // see step_local
            if (persistent) {
                a.queue = dual_queue.as<int>();
                a.resident = cu_count * schpf::per_cu(td.lds_bytes);
            }
            if (persistent || cut) a.task_order = tl.order.as<int>();
            // the loss pass keeps a 1 KiB logarithm table behind the window (sweep_impl.h LlhAccumulator)
            a.llh_tab_off = (int)((td.lds_bytes + 15) & ~(size_t)15);
            const size_t lds = logs ? (size_t)a.llh_tab_off + 1024 : td.lds_bytes;
            if (mode == schpf::MODE_ELBO || rows) a.clock_probe = nullptr;   // schpf_profile_clock: the sweeps and the loss pass
            if (rows) a.wave_out = mx.rows_rec.as<double>();
            HIPCHK(schpf::launch_tile_sweep<T>(a, NV, LPC, mode, td.packed ? 1 : 0, tl.n, td.threads, lds, stream));
        } else {
            PlanDev &pd = mx.axis[s].plan;
            auto a = sweep_args(s, mode);
            if (mode == schpf::MODE_LLH_ROWS) a.wave_out = mx.rows_rec.as<double>();
            if (mode == schpf::MODE_RANDOM)
                HIPCHK(schpf::launch_random_phi<T>(a, NV, LPC, seed, s == 0 ? 1 : 0, pd.launch, stream));
            else
                HIPCHK(schpf::launch_sweep<T>(a, NV, LPC, mode, pd.launch, stream));
        }
    }

    // where the update kernel finds a side's accumulated partial rows (SRC_STRIDED)
    void partial_source(int s, schpf::UpdateArgs<T> &u)
    {
        const PartialRows &pr = mx.facts(s).part;
        u.partials = pr.rows.as<T>(); u.pfirst = pr.first.as<int>(); u.pcount = pr.count.as<int>(); u.pstride = pr.stride;
    }

    void need_coo() const
    {
        if (!mx.have_coo) throw std::logic_error("no count matrix uploaded (schpf_upload_coo)");
    }
    void need_loss_constants() const
    {
        if (!mx.have_loss_constants)
            throw std::logic_error("this engine holds gathered batch rows (schpf_upload_rows): evaluate the loss on the source");
    }
    // doubles a loss / ELBO pass over side s (= loss_side()) leaves in wave_out
    int64_t n_wave_out(int s) const { return mx.facts(s).n_wave_out; }

    void init_phi_host(const double *xphi) override
    {
        need_coo();
        DevBuf dx, ord, mp;
        dx.alloc((size_t)mx.nnz * K * sizeof(double));
        HIPCHK(hipMemcpyAsync(dx.p, xphi, (size_t)mx.nnz * K * sizeof(double), hipMemcpyHostToDevice, stream));
        dense_cell.alloc((size_t)N * K * sizeof(T));
        for (int s = 0; s < 2; ++s) {
            const int *o = order_of(s, ord);
            upload(mp, major_ptr(s), stream);
            // Not symmetric: the cells' dense sums get a buffer of their own for this one iteration, the genes' go where
            // a sharded fit's do, the exchange buffer (step_finish reads both as SRC_DENSE while pending_init == 1)
            T *out = s == 0 ? dense_cell.as<T>() : exchange_buf.as<T>();
            HIPCHK(schpf::launch_segment_sum<T>(dx.as<double>(), o, mp.as<int64_t>(), side[s].n, K, out, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        pending_init = 1;
    }

    void init_phi_device(uint64_t seed) override
    {
        need_coo();
        // a rank of a communicator numbers its cells from 0 like every other rank: without this, local cell i of
        // every shard would draw the same responsibilities for a gene
        if (comm && comm_world > 1) seed += 0x9E3779B97F4A7C15ull * (uint64_t)(comm_rank + 1);
        run_sweep(0, schpf::MODE_RANDOM, seed);
        run_sweep(1, schpf::MODE_RANDOM, seed);
        pending_init = 2;
    }

    void step_local(unsigned flags_) override
    {
        need_coo();
        refresh_tables();
        const bool freeze = flags_ & SCHPF_FREEZE_GENES;
        const bool sharded = flags_ & SCHPF_SHARDED;
        const bool only_gene = flags_ & SCHPF_LOCAL_GENE, only_cell = flags_ & SCHPF_LOCAL_CELL;
        const bool do_cell = !only_gene || only_cell, do_gene = !only_cell || only_gene;
        if (sharded && sums_stale) {
            // after a fused iteration the exchange buffer's tail still mirrors an older sum of E[theta], and step_finish
            // would bring it up to date behind the all-reduce, with this rank's sum alone: do it before the packing
            reduce_colsums(0, s_theta);
            reduce_colsums(1, s_beta);
            sums_stale = false;
        }
        if (pending_init == 0 && mx.dual_slots > 0 && do_gene && do_cell && !freeze) {   // dual_slots: tile plans only
            // both sweeps read the same old tables: one launch (timed as kind 0, see schpf_profile_read)
            ScopedTimer tm(prof, stream, 0);
            // Not symmetric: the kernel takes (cell args, gene args) in that order; dual_order names gene tasks as ~task
            const TileDev &tc = mx.axis[0].tile, &tg = mx.axis[1].tile;
            auto ac = tile_args(0, schpf::MODE_PHI, tc.tasks), ag = tile_args(1, schpf::MODE_PHI, tg.tasks);
            // persistent workgroups (SCHPF_PERSISTENT=0: one workgroup per slot): as many as the device holds at
            // once draw the slots of the longest-first list from a counter -- no workgroup teardown / launch
            // between the ~6 tasks of a compute unit and whoever is free takes the next task: C3 sweep
            // -2 % f64, -5 % f32, nothing at C2 / the C5 share (profiles/r02/explore_persistent.log)
            const size_t lds = std::max(tc.lds_bytes, tg.lds_bytes);
            int *queue = nullptr;
            int resident = 0;
            if (tuning.persistent) {
                queue = dual_queue.as<int>();
                resident = cu_count * schpf::per_cu(lds);
            }
            HIPCHK(schpf::launch_tile_sweep_dual<T>(ac, ag, mx.dual_order.as<int>(), NV, LPC, tc.packed ? 1 : 0,
                                                    mx.dual_slots, tc.threads, lds, queue, resident, stream));
            tm.stop();
        } else if (pending_init == 0) {
            if (do_gene && !freeze) {
                ScopedTimer tm(prof, stream, 1);
                run_sweep(1, schpf::MODE_PHI);
                tm.stop();
            }
            if (do_cell) {
                ScopedTimer tm(prof, stream, 0);
                run_sweep(0, schpf::MODE_PHI);
                tm.stop();
            }
        }
        if (sharded && !freeze && pending_init != 1 && do_gene) {
            // fixed-order reduction of this rank's gene-side partials into the exchange buffer (the cells stay on their rank)
            const PartialRows &pr = mx.facts(1).part;
            HIPCHK(schpf::launch_combine_strided<T>(pr.rows.as<T>(), pr.first.as<int>(), pr.count.as<int>(), pr.stride, G, K,
                                                    KP, exchange_buf.as<T>(), stream));
        }
    }

    void exchange(void **p, int64_t *count) override
    {
        *p = exchange_buf.p;
        *count = (int64_t)G * K + K;
    }

    void step_finish(unsigned flags_) override
    {
        need_coo();
        const bool freeze = flags_ & SCHPF_FREEZE_GENES;
        const bool simultaneous = flags_ & SCHPF_SIMULTANEOUS;
        const bool sharded = flags_ & SCHPF_SHARDED;
        ScopedTimer tm(prof, stream, 3);
        const bool cells_first = flags_ & SCHPF_CELLS_FIRST;
        // default ordering on a small problem: no reduce launches (BASELINE C2: 2 of its 5 launches)
        const bool fuse = !sharded && !freeze && !simultaneous && !cells_first && tuning.fuse_sums &&
                          (int64_t)upd_blocks(N) * K <= 16384 && (int64_t)upd_blocks(G) * K <= 16384;
        if (!fuse && sums_stale) {   // s_theta / s_beta from the partials the last fused iteration left
            reduce_colsums(0, s_theta);
            reduce_colsums(1, s_beta);
            sums_stale = false;
        }
        // One block of the iteration: the cell block is scHPF_.py:706-714 (or :675-680), the gene block :697-704 (or
        // :668-673 + :682-685).  Where the two differ, `gene` says so.
        auto update = [&](int s) {
            const bool gene = s == 1;
            if (gene && freeze) return;   // SCHPF_FREEZE_GENES: eta / beta stay as they are
            Side &sd = side[s], &other = side[1 - s];
            schpf::UpdateArgs<T> u = update_args(s);
            int src = schpf::SRC_STRIDED;
            // dense sums instead of plan partials: right after init_phi_host (the cells' in dense_cell, the genes' in the
            // exchange buffer) and, gene side only, in every sharded iteration (the all-reduced exchange buffer)
            if (pending_init == 1 || (gene && sharded)) {
                src = schpf::SRC_DENSE;
                u.dense = gene ? exchange_buf.as<T>() : dense_cell.as<T>();
            } else partial_source(s, u);
            u.prior_shape = prior_shape(s);
            u.cap_shape = sd.cap_shape.as<T>(); u.cap_rate = sd.cap_rate.as<T>();
            if (gene) {
                u.s_other = s_theta.as<double>();
                // sharded: the all-reduced sum_i E[theta_ik] (old theta) is the tail of the exchange buffer; the
                // gene update reads it from there (s_other_t)
                if (sharded) u.s_other_t = exchange_buf.as<T>() + (size_t)G * K;
            } else {
                // theta.rate uses the beta just updated (scHPF_.py:711-713) unless the updates are
                // simultaneous (:677-679) or the genes are frozen
                u.s_other = (freeze || simultaneous || cells_first) ? s_beta.as<double>() : s_beta_next.as<double>();
            }
            if (fuse) { u.s_other_part = other.colpart.as<double>(); u.s_other_nb = upd_blocks(other.n); }
            u.cap_prior_rate = cap_prior_rate(s);
            u.cap_rate_out = sd.cap_rate.as<T>();
            HIPCHK(schpf::launch_gamma_update(u, src, upd_blocks(sd.n), stream));
            // the new beta's sums go to the other half of the double buffer: the cell update may still need the old ones
            if (!fuse) reduce_colsums(s, gene ? s_beta_next : s_theta);
        };
        if (cells_first) { update(0); update(1); }   // minibatch order: theta first, beta from the NEW theta
        else { update(1); update(0); }
        if (!freeze) { std::swap(s_beta.p, s_beta_next.p); beta_parity ^= 1; }
        if (fuse) sums_stale = true;
        if (pending_init == 1) dense_cell.release();
        pending_init = 0;
        tm.stop();
    }

    void loss_terms(double *llh, double *gl, int64_t *nnz_out) override
    {
        need_coo();
        need_loss_constants();
        refresh_tables();
        ScopedTimer tm(prof, stream, 2);
        const int ls = loss_side();
        run_sweep(ls, schpf::MODE_LLH);
        double *res = loss_host ? loss_host : scalars.as<double>();   // pinned host memory is device-addressable as it is
        HIPCHK(schpf::launch_sum_doubles(mx.wave_out.as<double>(), n_wave_out(ls), res, stream));
        // explicitly stored zeros look like padding to the sweeps (weight 0, which is what they
        // contribute to the shape updates, hpf_numba.py:97-112), but the reference's loss counts
        // them: x log r - r - lgamma(x+1) = -r (hpf_numba.py:43-50)
        if (mx.n_zero > 0)
            HIPCHK(schpf::launch_zero_rate_sum<T>(mx.zero_row.as<int>(), mx.zero_col.as<int>(), mx.n_zero, side[0].tab_e.as<T>(),
                                                  side[1].tab_e.as<T>(), K, KP, res + 2, stream));
        tm.stop();
        double h[3] = {0.0, 0.0, 0.0};
        if (!loss_host) HIPCHK(hipMemcpyAsync(h, scalars.p, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (loss_host) { h[0] = loss_host[0]; h[2] = loss_host[2]; }
        *llh = mx.n_zero > 0 ? h[0] - h[2] : h[0];
        *gl = mx.gammaln_sum;
        *nnz_out = mx.nnz;
    }

    // The evidence lower bound of the current state, terms {data, logfac, rate, cell, gene}:
    //   data  = sum x log sum_k exp(Elt + Elb) = [MODE_ELBO sweep: sum x log s] + sum_i m_i r_i + sum_g m_g c_g
    //   logfac = the loss's gammaln_sum;  rate = sum_k (sum_i E theta_ik)(sum_g E beta_gk)
    //   cell / gene = the prior and entropy terms of (xi, theta) / (eta, beta)  (elbo_gamma_kernel)
    // Reads the state only: its own scratch (the update kernels' column partials may be live, sums_stale), nothing cached.
    void elbo_terms(double ap, double cp, double terms[5]) override
    {
        need_coo();
        need_loss_constants();
        if (!(ap > 0 && cp > 0)) throw std::invalid_argument("ap and cp must be positive");
        refresh_tables();
        const int ls = loss_side();
        run_sweep(ls, schpf::MODE_ELBO);
        const int nb[2] = {upd_blocks(N), upd_blocks(G)}, W = K + 2;
        if (elbo_part.bytes < (size_t)std::max(nb[0], nb[1]) * W * sizeof(double))
            elbo_part.alloc((size_t)std::max(nb[0], nb[1]) * W * sizeof(double));
        if (!elbo_sums.p) elbo_sums.alloc((size_t)(2 * W + 1) * sizeof(double));
        double *sums = elbo_sums.as<double>();   // [W of the cell side | W of the gene side | sweep sum]
        HIPCHK(schpf::launch_sum_doubles(mx.wave_out.as<double>(), n_wave_out(ls), sums + 2 * W, stream));
        const double cap_prior_shape[2] = {ap, cp};
        for (int s = 0; s < 2; ++s) {   // cells, then genes: both through the one elbo_part scratch
            const Side &sd = side[s];
            HIPCHK(schpf::launch_elbo_gamma<T>(sd.shape.as<T>(), sd.rate.as<T>(), sd.cap_shape.as<T>(), sd.cap_rate.as<T>(),
                                               sd.tab_log.as<T>(), mx.axis[s].count.template as<double>(), sd.n, K, KP, prior_shape(s),
                                               cap_prior_shape[s], cap_prior_rate(s), elbo_part.as<double>(), nb[s], stream));
            HIPCHK(schpf::launch_colsum_reduce(elbo_part.as<double>(), nb[s], W, sums + s * W, nullptr, 0, stream));
        }
        std::vector<double> h((size_t)(2 * W + 1));
        HIPCHK(hipMemcpyAsync(h.data(), sums, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        double rate = 0.0;
        for (int k = 0; k < K; ++k) rate += h[(size_t)k] * h[(size_t)(W + k)];
        terms[0] = h[(size_t)(2 * W)] + h[(size_t)(K + 1)] + h[(size_t)(W + K + 1)];
        terms[1] = mx.gammaln_sum;
        terms[2] = rate;
        terms[3] = h[(size_t)K];
        terms[4] = h[(size_t)(W + K)];
    }

    // The stored zeros grouped by the rows of axis s, once per upload: sorted by row, upload order kept within a row, so
    // that one thread per row adds them in the same order on every call
    void build_zero_rows(int s)
    {
        Matrix::ZeroRows &z = mx.zero_rows[s];
        if (z.built) return;
        std::vector<int32_t> idx[2] = {std::vector<int32_t>((size_t)mx.n_zero), std::vector<int32_t>((size_t)mx.n_zero)};
        d2h(idx[0].data(), mx.zero_row, (size_t)mx.n_zero * 4, stream);
        d2h(idx[1].data(), mx.zero_col, (size_t)mx.n_zero * 4, stream);
        const std::vector<int32_t> &major = idx[s], &minor = idx[1 - s];
        std::vector<int64_t> perm((size_t)mx.n_zero);
        for (int64_t i = 0; i < mx.n_zero; ++i) perm[(size_t)i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return major[(size_t)x] < major[(size_t)y]; });
        std::vector<int32_t> seg_major, seg_ptr, mn((size_t)mx.n_zero);
        for (int64_t j = 0; j < mx.n_zero; ++j) {
            const int32_t m = major[(size_t)perm[(size_t)j]];
            if (seg_major.empty() || seg_major.back() != m) { seg_major.push_back(m); seg_ptr.push_back((int32_t)j); }
            mn[(size_t)j] = minor[(size_t)perm[(size_t)j]];
        }
        seg_ptr.push_back((int32_t)mx.n_zero);
        z.n_seg = (int)seg_major.size();
        upload(z.seg_major, seg_major, stream); upload(z.seg_ptr, seg_ptr, stream); upload(z.minor, mn, stream);
        HIPCHK(hipStreamSynchronize(stream));   // the host vectors die with this scope
        z.built = true;
    }

    // Per major row of axis `by` (0: cells, 1: genes), over the stored entries: sum x log r - r, sum lgamma(x + 1) and the
    // number of entries.  A MODE_LLH_ROWS sweep of THAT axis' plan over the iteration's own tasks (their
    // partial-row addressing says where a row's records lie), a fixed-order sum per row, then the stored zeros.  Reads the
    // state only, as elbo_terms does: scratch of its own, nothing cached but the sorted zero list.
    void loss_rows(int by, double *llh, double *gl, int64_t *count) override
    {
        if (by != SCHPF_BY_CELL && by != SCHPF_BY_GENE) throw std::invalid_argument("by must be SCHPF_BY_CELL or SCHPF_BY_GENE");
        need_coo();
        need_loss_constants();
        const int s = by;
        const Side &sd = side[s];
        const size_t n = (size_t)sd.n, n_max = (size_t)std::max(N, G);
        const int64_t n_rec = std::max(mx.facts(0).part.n, mx.facts(1).part.n);   // one scratch for either axis
        const size_t rec_bytes = (size_t)std::max<int64_t>(n_rec, 1) * schpf::ROW_REC * sizeof(double);
        if (mx.rows_rec.bytes < rec_bytes) mx.rows_rec.alloc(rec_bytes);
        if (mx.rows_out.bytes < n_max * 24) mx.rows_out.alloc(n_max * 24);
        if (mx.n_zero > 0) build_zero_rows(s);
        refresh_tables();
        double *d_llh = mx.rows_out.as<double>(), *d_gl = d_llh + n;
        int64_t *d_cnt = reinterpret_cast<int64_t *>(d_gl + n);
        ScopedTimer tm(prof, stream, 2);
        run_sweep(s, schpf::MODE_LLH_ROWS);
        const PartialRows &pr = mx.facts(s).part;
        HIPCHK(schpf::launch_row_records_reduce(mx.rows_rec.as<double>(), pr.first.as<int>(), pr.count.as<int>(),
                                                pr.stride, sd.n, d_llh, d_gl, d_cnt, stream));
        if (mx.n_zero > 0) {
            const Matrix::ZeroRows &z = mx.zero_rows[s];
            HIPCHK(schpf::launch_zero_rate_rows<T>(z.seg_major.template as<int>(), z.seg_ptr.template as<int>(), z.n_seg,
                                                   z.minor.template as<int>(),
                                                   sd.tab_e.as<T>(), side[1 - s].tab_e.as<T>(), K, KP, d_llh, d_cnt, stream));
        }
        tm.stop();
        HIPCHK(hipMemcpyAsync(llh, d_llh, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(gl, d_gl, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(count, d_cnt, n * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    // Per major row of axis `by`, over ALL rows of the other axis: sum exp(-lambda), sum lambda, sum lambda^2 with lambda =
    // E theta . E beta.  From the stored shape / rate, not the tables (which may be older, sums_stale /
    // dirty, and stay so); needs no matrix; writes its own scratch only.  No clock probe, never captured, as elbo_terms.
    void predictive_rows(int by, double *zeros, double *rate, double *rate2) override
    {
        if (by != SCHPF_BY_CELL && by != SCHPF_BY_GENE) throw std::invalid_argument("by is neither SCHPF_BY_CELL nor SCHPF_BY_GENE");
        if (!zeros && !rate && !rate2) throw std::invalid_argument("zeros, rate and rate2 are all NULL: nothing to return");
        const size_t n = (size_t)side[by].n;
        for (int s = 0; s < 2; ++s) {
            const size_t bytes = (size_t)schpf::predictive_pad(side[s].n) * K * sizeof(double);
            if (ppc_e[s].bytes < bytes) ppc_e[s].alloc(bytes);
            HIPCHK(schpf::launch_predictive_e<T>(side[s].shape.as<T>(), side[s].rate.as<T>(), side[s].n, K, ppc_e[s].as<double>(), stream));
        }
        if (ppc_out.bytes < 3 * n * sizeof(double)) ppc_out.alloc(3 * (size_t)std::max(N, G) * sizeof(double));
        HIPCHK(schpf::launch_predictive_rows(ppc_e[by].as<double>(), ppc_e[1 - by].as<double>(), side[by].n, side[1 - by].n, K,
                                             schpf::predictive_strip(side[by].n, cu_count), ppc_out.as<double>(), stream));
        double *const dst[3] = {zeros, rate, rate2};
        for (int i = 0; i < 3; ++i)
            if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], ppc_out.as<double>() + i * n, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    // schpf_debug_tables: a side's tables as the next sweep would read them, padding columns included.  Touches what
    // loss_terms touches before its sweep (refresh_tables) and nothing else
    void debug_tables(int s, void *tab_e, void *tab_log, void *tab_exp) override
    {
        if (s != SCHPF_BY_CELL && s != SCHPF_BY_GENE) throw std::invalid_argument("side must be SCHPF_BY_CELL or SCHPF_BY_GENE");
        refresh_tables();
        const Side &sd = side[s];
        const size_t bytes = (size_t)sd.n * KP * sizeof(T);
        void *const dst[3] = {tab_e, tab_log, tab_exp};
        const DevBuf *const src[3] = {&sd.tab_e, &sd.tab_log, &sd.tab_exp};
        for (int i = 0; i < 3; ++i)
            if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], src[i]->p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }

    // which tile plan the loss pass sweeps (policy.cpp loss_side)
    int loss_side() const
    {
        if (!mx.use_tile) return 0;
        const TileDev &tc = mx.axis[0].tile, &tg = mx.axis[1].tile;
        const double model[2] = {tc.llh_model, tg.llh_model};
        const int64_t tasks[2] = {tc.tasks.n, tg.tasks.n};
        // the policy's question about wave_out is whether the gene plan's pass fits; the LDS figure is the cell plan's
        return schpf::loss_side(problem(), tuning, mx.wave_out.bytes >= (size_t)tg.n_wave_out * sizeof(double), model, tasks,
                                tc.lds_bytes);
    }

    void upload_info(int64_t info[4]) override
    {
        info[0] = mx.nnz; info[1] = mx.n_rounded; info[2] = mx.n_zero;
        info[3] = (mx.facts(0).packed ? 1 : 0) | (mx.rows_ptr.p ? 2 : 0);   // bit 0: packed entries; bit 1: a row-sorted copy
    }

    // Shader clock the chip sustained under the sweep launches since the last read (tile plans; 0 launches: unknown).
    void profile_clock(double *shader_mhz, int64_t *launches) override
    {
        unsigned long long h[5] = {0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(h, clock_probe.p, sizeof h, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemsetAsync(clock_probe.p, 0, sizeof h, stream));
        HIPCHK(hipStreamSynchronize(stream));
        int khz = 0;   // rate of s_memrealtime
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
            (void)hipGetLastError();
            khz = 100000;
        }
        *launches = (int64_t)h[4];
        *shader_mhz = h[1] ? (double)h[0] / (double)h[1] * (double)khz * 1e-3 : 0.0;
    }

    // LDS bytes the tasks of a tile plan stage: every (sub-)window of a task's range exactly once -- the half-window
    // schedule fills all slots at the first epoch and afterwards only the slot the last epoch owned, never beyond the
    // task's last window (sweep_impl.h, the window loop)
    int64_t staged_bytes(int s) const
    {
        const TileDev &td = mx.axis[s].tile;
        const schpf::TilePlanHost &P = td.host;
        const int nm = td.n_virtual ? td.n_virtual : side[1 - s].n;
        int64_t rows = 0;
        for (size_t t = 0; t < P.task_w0.size(); ++t)
            for (int w = P.task_w0[t]; w < P.task_w1[t]; ++w) rows += std::max(0, std::min(P.win_rows, nm - w * P.win_rows));
        return rows * (int64_t)KP * (int64_t)sizeof(T);
    }
    // Bytes one iteration moves through the LDS and streams from HBM, from the plans (tile plans; else zeros):
    //   [0] LDS reads of the nonzeros alone: every nonzero reads one table row of KP values per orientation
    //   [1] ... of the stored step slots (padding slots execute the same reads)
    //   [2] [3] LDS writes of the window stagings, cell / gene side
    //   [4] entry stream of both plans in HBM   [5] partial rows written
    void sweep_bytes(int64_t info[8]) override
    {
        for (int i = 0; i < 8; ++i) info[i] = 0;
        if (!mx.use_tile || !mx.have_coo) return;
        const int64_t row = (int64_t)KP * (int64_t)sizeof(T);
        info[0] = 2 * mx.nnz * row;
        const TileDev &tc = mx.axis[0].tile, &tg = mx.axis[1].tile;
        info[1] = (tc.entry_slots + tg.entry_slots) * row;
        info[2] = staged_bytes(0);
        info[3] = staged_bytes(1);
        info[4] = (tc.entry_slots + tg.entry_slots) * (tc.packed ? 4 : 8);
        info[5] = (tc.part.n + tg.part.n) * row;
        // what the loss pass will sweep (loss_side, loss_tasks): so that a report can say which plan and cut the model chose
        const int ls = loss_side();
        const TileDev &tl = mx.axis[ls].tile;
        info[6] = ls;
        info[7] = tl.llh.n > 0 ? tl.llh.n : tl.tasks.n;
    }

    // per-side entries come in (cell, gene) pairs; [3], [14], [15] describe the cell plan
    void plan_info(int64_t info[16]) override
    {
        info[0] = KP; info[1] = KL; info[2] = LPC;
        for (int s = 0; s < 2; ++s) {
            const PlanFacts &pl = mx.facts(s);
            info[4 + s] = pl.windows; info[6 + s] = pl.part.n; info[8 + s] = pl.launch; info[10 + s] = pl.entry_slots;
        }
        info[3] = mx.axis[0].plan.host.chunk_len;
        info[12] = info[13] = info[14] = info[15] = 0;
        if (mx.use_tile) {   // tile-only: [3] negative, rows per LDS window; ring slots per side; slot bytes; waves per block
            const schpf::TilePlanHost &hc = mx.axis[0].tile.host;
            info[3] = -hc.win_rows; info[12] = hc.ring; info[13] = mx.axis[1].tile.host.ring;
            info[14] = hc.slot16 * 16; info[15] = hc.wpb;
        }
    }
};

}  // namespace

// ------------------------------------------------------------------------- C ABI
extern "C" {

const char *schpf_last_error(void) { return g_err.c_str(); }
const char *schpf_version(void)
{
    return "schpf_hip 0.3 (gfx950)";
}

int schpf_device_count(int *count)
{
    return guarded([&] {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
        *count = n;
    });
}

int schpf_create(schpf_ctx **out, int device, void *stream, int dtype, int ncells, int ngenes, int nfactors)
{
    if (!out) return fail("out is NULL");
    *out = nullptr;
    if (bad_dtype(dtype)) return fail("dtype must be SCHPF_F32 or SCHPF_F64");
    if (ncells < 1 || ngenes < 1) return fail("ncells and ngenes must be positive");
    return guarded([&] {
        int n = 0;
        HIPCHK(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) throw std::invalid_argument("no such HIP device");
        if (dtype == SCHPF_F64) *out = new Engine<double>(device, stream, dtype, ncells, ngenes, nfactors);
        else *out = new Engine<float>(device, stream, dtype, ncells, ngenes, nfactors);
    });
}
int schpf_destroy(schpf_ctx *ctx)
{
    return guarded([&] { delete ctx; });
}

#define CTX_CALL(body)                                       \
    if (!ctx) return fail("ctx is NULL");                    \
    return guarded([&] {                                     \
        HIPCHK(hipSetDevice(ctx->device));                   \
        body;                                                \
    })

int schpf_upload_coo(schpf_ctx *ctx, int64_t nnz, const int32_t *row, const int32_t *col, const void *val,
                     int val_kind)
{
    CTX_CALL(ctx->upload_coo(nnz, row, col, val, val_kind));
}
int schpf_set_hypers(schpf_ctx *ctx, double a, double c, double bp, double dp)
{
    if (!(a > 0 && c > 0 && bp > 0 && dp > 0)) return fail("hyperparameters must be positive");
    CTX_CALL(ctx->a = a; ctx->c = c; ctx->bp = bp; ctx->dp = dp; ctx->drop_graphs());
}
int schpf_set_state(schpf_ctx *ctx, int which, const void *shape, const void *rate)
{
    CTX_CALL(ctx->set_state(which, shape, rate));
}
int schpf_get_state(schpf_ctx *ctx, int which, void *shape, void *rate)
{
    CTX_CALL(ctx->get_state(which, shape, rate));
}
int schpf_set_state_device(schpf_ctx *ctx, int which, const void *shape, const void *rate)
{
    CTX_CALL(ctx->set_state(which, shape, rate, true));
}
int schpf_get_state_device(schpf_ctx *ctx, int which, void *shape, void *rate)
{
    CTX_CALL(ctx->get_state(which, shape, rate, true));
}
int schpf_upload_coo_device(schpf_ctx *ctx, int64_t nnz, const void *row, const void *col, int idx_kind, const void *val,
                            int val_kind)
{
    if (nnz > 0 && (!row || !col || !val)) return fail("row, col and val must be device pointers, not NULL");
    CTX_CALL(ctx->upload_device(nnz, row, -1, col, idx_kind, val, val_kind));
}
int schpf_upload_csr_device(schpf_ctx *ctx, int64_t nnz, const void *indptr, int indptr_kind, const void *indices,
                            int idx_kind, const void *val, int val_kind)
{
    if (!indptr || (nnz > 0 && (!indices || !val))) return fail("indptr, indices and val must be device pointers, not NULL");
    if (indptr_kind != SCHPF_IDX_I32 && indptr_kind != SCHPF_IDX_I64) return fail("unknown index kind");
    CTX_CALL(ctx->upload_device(nnz, indptr, indptr_kind, indices, idx_kind, val, val_kind));
}
int schpf_marginals(schpf_ctx *ctx, double *row_sums, double *col_sums)
{
    CTX_CALL(ctx->marginals(row_sums, col_sums));
}
int schpf_init_phi_host(schpf_ctx *ctx, const double *xphi) { CTX_CALL(ctx->init_phi_host(xphi)); }
int schpf_init_phi_device(schpf_ctx *ctx, uint64_t seed) { CTX_CALL(ctx->init_phi_device(seed)); }
int schpf_step(schpf_ctx *ctx, unsigned flags)
{
    if (flags & SCHPF_SHARDED) return fail("schpf_step is the single-GPU form; use step_local/step_finish");
    CTX_CALL(ctx->steps(flags, 1));
}
int schpf_step_local(schpf_ctx *ctx, unsigned flags) { CTX_CALL(ctx->step_local(flags)); }
int schpf_exchange_buffer(schpf_ctx *ctx, void **device_ptr, int64_t *count)
{
    CTX_CALL(ctx->exchange(device_ptr, count));
}
int schpf_step_finish(schpf_ctx *ctx, unsigned flags) { CTX_CALL(ctx->step_finish(flags)); }
int schpf_steps(schpf_ctx *ctx, unsigned flags, int n)
{
    if (flags & SCHPF_SHARDED) return fail("schpf_steps is the single-GPU form; use step_local/step_finish");
    CTX_CALL(ctx->steps(flags, n));
}
int schpf_loss_terms(schpf_ctx *ctx, double *llh_sum, double *gammaln_sum, int64_t *nnz)
{
    CTX_CALL(ctx->loss_terms(llh_sum, gammaln_sum, nnz));
}
int schpf_elbo_terms(schpf_ctx *ctx, double ap, double cp, double terms[5])
{
    if (!ctx) return fail("ctx is NULL");
    if (!terms) return fail("terms is NULL");
    CTX_CALL(ctx->elbo_terms(ap, cp, terms));
}
int schpf_loss_rows(schpf_ctx *ctx, int by, double *llh_sum, double *gammaln_sum, int64_t *count)
{
    if (!ctx) return fail("ctx is NULL");
    if (!llh_sum || !gammaln_sum || !count) return fail("output pointer is NULL");
    CTX_CALL(ctx->loss_rows(by, llh_sum, gammaln_sum, count));
}
int schpf_predictive_rows(schpf_ctx *ctx, int by, double *zeros, double *rate, double *rate2)
{
    CTX_CALL(ctx->predictive_rows(by, zeros, rate, rate2));
}
int schpf_synchronize(schpf_ctx *ctx) { CTX_CALL(HIPCHK(hipStreamSynchronize(ctx->stream))); }

int schpf_comm_unique_id(void *out128)
{
    if (!out128) return fail("out is NULL");
    return guarded([&] {
        RcclUniqueId id;
        RCCLCHK(rccl().GetUniqueId(&id));
        std::memcpy(out128, &id, sizeof id);
    });
}
int schpf_comm_init(schpf_ctx *ctx, const void *unique_id128, int rank, int world)
{
    if (!unique_id128) return fail("unique_id is NULL");
    // a cached hipGraph of a sharded stretch holds an all-reduce bound to the communicator it was captured with: every
    // cached graph goes before the communicator does
    CTX_CALL(ctx->drop_graphs(); ctx->comm_init(unique_id128, rank, world));
}
int schpf_comm_destroy(schpf_ctx *ctx) { CTX_CALL(ctx->drop_graphs(); ctx->comm_destroy()); }
int schpf_hint_sharded(schpf_ctx *ctx, int on) { CTX_CALL(ctx->expect_sharded = on != 0); }
int schpf_hint_transient(schpf_ctx *ctx, int on) { CTX_CALL(ctx->transient = on != 0); }
int schpf_keep_rows(schpf_ctx *ctx, int on) { CTX_CALL(ctx->want_rows = on != 0); }
int schpf_upload_rows(schpf_ctx *ctx, schpf_ctx *source, const int32_t *rows, int n_rows)
{
    if (!source) return fail("source is NULL");
    if (!rows && n_rows > 0) return fail("rows is NULL");
    CTX_CALL(ctx->upload_rows(source, rows, n_rows));
}
int schpf_steps_sharded(schpf_ctx *ctx, unsigned flags, int n)
{
    if (n < 0) return fail("n must be >= 0");
    CTX_CALL(ctx->steps_sharded(flags, n));
}
int schpf_loss_terms_all(schpf_ctx *ctx, double *llh_sum, double *gammaln_sum, int64_t *nnz)
{
    CTX_CALL(ctx->loss_terms_all(llh_sum, gammaln_sum, nnz));
}
int schpf_stream_handle(schpf_ctx *ctx, void **stream)
{
    if (!stream) return fail("stream is NULL");
    CTX_CALL(*stream = (void *)ctx->stream);
}

int schpf_profile_enable(schpf_ctx *ctx, int enable) { CTX_CALL(ctx->prof.on = enable != 0); }
int schpf_profile_read(schpf_ctx *ctx, double ms[4], int64_t launches[4])
{
    CTX_CALL(
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 4; ++i) { ms[i] = 0.0; launches[i] = 0; }
        for (auto &r : ctx->prof.recs) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
            ms[r.kind] += (double)t;
            launches[r.kind]++;
            ctx->prof.pool.push_back(r.a);
            ctx->prof.pool.push_back(r.b);
        }
        ctx->prof.recs.clear());
}
int schpf_profile_clock(schpf_ctx *ctx, double *shader_mhz, int64_t *launches)
{
    if (!shader_mhz || !launches) return fail("output pointer is NULL");
    CTX_CALL(ctx->profile_clock(shader_mhz, launches));
}
int schpf_sweep_bytes(schpf_ctx *ctx, int64_t info[8])
{
    if (!info) return fail("output pointer is NULL");
    CTX_CALL(ctx->sweep_bytes(info));
}
int schpf_plan_info(schpf_ctx *ctx, int64_t info[16])
{
    if (!info) return fail("output pointer is NULL");
    CTX_CALL(ctx->plan_info(info));
}
int schpf_upload_info(schpf_ctx *ctx, int64_t info[4])
{
    if (!info) return fail("output pointer is NULL");
    CTX_CALL(ctx->upload_info(info));
}
int schpf_debug_tables(schpf_ctx *ctx, int side, void *tab_e, void *tab_log, void *tab_exp)
{
    CTX_CALL(ctx->debug_tables(side, tab_e, tab_log, tab_exp));
}
}  // extern "C"
