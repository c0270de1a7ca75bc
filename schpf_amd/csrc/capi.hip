// C ABI of libschpf_hip.so (include/schpf_hip.h): context management, uploads, and the
// ordering of kernel launches that makes one CAVI iteration (scHPF_.py:657-714).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include "common.h"
#include "kernels.h"
#include "policy.h"
#include "rccl.h"
#include "upload_device.h"

using namespace schpf;

thread_local std::string schpf::g_err;

namespace {

// A major row's partial rows -- the K-vectors a sweep accumulates for it, and the records of a MODE_LLH_ROWS pass, which
// are addressed alike -- are first[row] + j * stride, j < count[row].  Tile plans: one per (row, task) (plan.h pfirst /
// pcount / pstride); gather plans: the row's consecutive chunks, stride 1
struct PartialRows { DevBuf rows, first, count; int64_t stride = 1, n = 0; };   // rows: [n, KP] of T

// What the engine asks of a side's plan whatever its kind (Side::active); the builders fill it
struct PlanFacts {
    PartialRows part;
    std::vector<int64_t> mptr;      // run pointers of the (major, minor)-sorted order, on the host (moved out of `host`)
    // (major, minor)-sorted position -> caller's COO position: on the device (device-built plans), the identity (the
    // input was already in that order), or on the host (host-built plans; moved out of `host`)
    DevBuf order_dev; bool order_identity = false; schpf::BigVec<int32_t> order;
    int64_t launch = 0;             // size of an iteration's sweep launch: tasks (tile) / wavefronts (gather)
    // doubles a loss / ELBO pass over this plan leaves in wave_out.  Not symmetric: gather plans only ever sweep the cell
    // side for it (loss_side), so a gather plan of the gene side leaves this 0
    int64_t n_wave_out = 0, entry_slots = 0;
    int windows = 0;
    bool packed = false;            // 8-byte entries (tile plans whose counts all fit 16 bits)
};

struct PlanDev : PlanFacts {
    schpf::SweepPlanHost host;  // entries and the per-slice arrays cleared after upload; order / mptr moved to the facts
    DevBuf entries, slice_off, slice_steps, chunk_major, chunk_natid, wave_slice;
};

// The tasks a tile sweep launches, one entry per task.  stage_end: only sub-range tasks have one (kernels.h task_stage_end)
struct TaskList {
    DevBuf block, w0, w1, stage_end, wave_off;
    DevBuf order;               // tasks by decreasing work: the slot list of a persistent single-side launch
    int64_t n = 0;
};

struct TileDev : PlanFacts {
    schpf::TilePlanHost host;   // entries/steps cleared after upload; order / mptr moved to the facts
    DevBuf entries, steps, block_rows;
    TaskList tasks;             // the iteration's
    // The loss pass (MODE_LLH) writes no partial rows, so its tasks may be cut finer than the iteration's: sub-ranges of
    // the tasks' window ranges, enough of them for a few rounds of the device (Engine::loss_tasks); n = 0: not cut
    TaskList llh;
    double llh_model = 0.0;     // modelled length of the loss pass on this plan, in step units (0: unknown)
    DevBuf minor_of;            // balanced windows (plan.h): [n_blocks * n_virtual] table row staged at a window position, or empty
    int n_virtual = 0;
    int threads = 512;
    size_t lds_bytes = 0;
};

// Everything the engine holds once per matrix axis.  Engine::side[0] is the cell axis (major = cell: xi, theta), side[1]
// the gene axis (eta, beta) -- the numbering of run_sweep, loss_side, order_of and the policy.  The records live inside
// the engine and never move: captured graphs bake the DevBuf::p pointers in.
struct Side {
    int n = 0;                         // rows of this axis: N / G
    DevBuf cap_shape, cap_rate;        // xi / eta                            [n]
    DevBuf shape, rate;                // theta / beta (C-contiguous)         [n, K]
    DevBuf tab_exp, tab_e, tab_log;    // tables, padding columns zero        [n, KP]
    DevBuf colpart;                    // the update kernel's column partials double[UPD_BLOCKS * K]
    DevBuf count;                      // ELBO: sum of the stored counts of each row of this axis, double[n]
    PlanDev plan;                      // gather plan with this axis as major
    TileDev tile;                      // tile plan (LDS-staged sweep) with this axis as major
    PlanFacts *active = &plan;         // whichever of the two the last upload built (Engine::choose_plan)
    bool dirty = true;                 // the tables and column sums are older than the parameters
    Side() = default;
    Side(const Side &) = delete; Side &operator=(const Side &) = delete;
};

// What one upload knows about itself.  Made by upload_coo / upload_rows, handed down the stages by reference, gone with
// the call: nothing of it is parked in the engine.
struct UploadJob {
    int64_t nnz = 0;
    bool balance = false;              // balanced windows for this matrix (policy.cpp balance_windows)
    bool batch_rows = false;           // gathered batch rows (upload_rows): no loss constants, no loss tasks
    bool packed_ok = true;             // every count fits the packed 16-bit entry format
    bool sorted[2] = {true, true};     // the COO is already in (row, col) / (col, row) order
    int ranges[2] = {0, 0}, half[2] = {-1, -1};   // task ranges per orientation (policy.cpp choose_ranges)
    schpf::TileShape shape[2];
    bool balanced[2] = {false, false}; // this orientation's plan is built on balanced windows
};

struct Profiler {
    bool on = false;
    struct Rec { int kind; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        return e;
    }
    ~Profiler()
    {
        for (auto &r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
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

}  // namespace

// ------------------------------------------------------------------------------------
struct schpf_ctx {
    int device = 0, dtype = SCHPF_F64, N = 0, G = 0, K = 0;
    int KP = 0, KL = 0, LPC = 1, NV = 1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    virtual ~schpf_ctx() { comm_destroy(); }
    virtual void upload_coo(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int kind) = 0;
    // an upload from device memory: a COO (indptr_kind < 0, rows = the row index per entry) or a CSR (rows = indptr)
    virtual void upload_device(int64_t nnz, const void *rows, int indptr_kind, const void *col, int idx_kind,
                               const void *val, int val_kind) = 0;
    virtual void marginals(double *row_sums, double *col_sums) = 0;
    // device: shape / rate are device pointers (a copy on the stream) instead of host pointers
    virtual void set_state(int which, const void *shape, const void *rate, bool device = false) = 0;
    virtual void get_state(int which, void *shape, void *rate, bool device = false) = 0;
    virtual void init_phi_host(const double *xphi) = 0;
    virtual void init_phi_device(uint64_t seed) = 0;
    virtual void step_local(unsigned flags) = 0;
    virtual void step_finish(unsigned flags) = 0;
    virtual void steps(unsigned flags, int n) = 0;
    virtual void upload_rows(schpf_ctx *source, const int32_t *rows, int n_rows) = 0;
    virtual void steps_sharded(unsigned flags, int n) = 0;
    virtual void loss_terms_all(double *llh, double *gl, int64_t *nnz) = 0;
    // cells sharded over GPUs: this rank's RCCL communicator and the stream its collectives run on
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_reduced = nullptr;
    void comm_init(const void *id, int rank, int world)
    {
        if (world < 1 || rank < 0 || rank >= world) throw std::invalid_argument("rank must be in [0, world)");
        comm_destroy();
        RcclUniqueId uid;
        std::memcpy(&uid, id, sizeof uid);
        RCCLCHK(rccl().CommInitRank(&comm, world, uid, rank));
        comm_rank = rank; comm_world = world;
        HIPCHK(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ev_packed, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_reduced, hipEventDisableTiming));
    }
    void comm_destroy()
    {
        if (comm) { (void)hipStreamSynchronize(comm_stream); (void)rccl().CommDestroy(comm); comm = nullptr; }
        if (comm_stream) { (void)hipStreamDestroy(comm_stream); comm_stream = nullptr; }
        if (ev_packed) { (void)hipEventDestroy(ev_packed); ev_packed = nullptr; }
        if (ev_reduced) { (void)hipEventDestroy(ev_reduced); ev_reduced = nullptr; }
    }
    virtual void exchange(void **p, int64_t *count) = 0;
    virtual void loss_terms(double *llh, double *gl, int64_t *nnz) = 0;
    virtual void elbo_terms(double ap, double cp, double terms[5]) = 0;
    virtual void loss_rows(int by, double *llh, double *gl, int64_t *count) = 0;
    virtual void plan_info(int64_t info[16]) = 0;
    virtual void debug_tables(int side, void *tab_e, void *tab_log, void *tab_exp) = 0;
    virtual void upload_info(int64_t info[4]) = 0;
    virtual void profile_clock(double *shader_mhz, int64_t *launches) = 0;
    virtual void sweep_bytes(int64_t info[8]) = 0;
    double a = 0.3, c = 0.3, bp = 1.0, dp = 1.0;   // kernel arguments of the captured launches: set_hypers drops the graphs
    bool expect_sharded = false;        // schpf_hint_sharded: a rank of a sharded fit (gene-side sums leave for an all-reduce)
    bool transient = false;             // schpf_hint_transient: the matrix is replaced every iteration, plan the cheapest way
    bool want_rows = false;             // schpf_keep_rows: keep a (row, col)-sorted device copy for upload_rows
    Profiler prof;
    // n iterations captured as one hipGraph (schpf_steps): the state is device-resident and nothing on
    // the host changes between two loss checks, so a fit replays one graph per check interval
    // The sum-of-beta buffers swap roles every iteration (beta_parity counts the swaps mod 2) and a
    // capture bakes the pointers in, so a graph is keyed by (flags, n, parity at its start): one cached
    // graph per parity.  A stretch with an odd count (check_freq = 5: graph of 4 + one eager iteration)
    // starts its calls at alternating parities and alternates between the two.
    struct CachedGraph { hipGraphExec_t exec = nullptr; unsigned flags = 0; int n = 0; };
    CachedGraph graphs[2];
    // what a captured graph bakes in has changed: hypers, the matrix, the communicator
    void drop_graphs()
    {
        for (CachedGraph &g : graphs) {
            if (g.exec) { (void)hipStreamSynchronize(stream); (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
            g.n = 0;
        }
    }
};

namespace {

template <typename T> struct Engine final : schpf_ctx {
    const schpf::Tuning tuning = schpf::tuning_from_env();   // the switches, read once at schpf_create
    Side side[2];                                   // 0: cells, 1: genes.  Below: what exists once, or for one axis only
    DevBuf exchange_buf;                            // gene side: [G*K + K] of T, the sums a sharded fit all-reduces + K sums of E[theta]
    DevBuf dense_cell;                              // cell side: [N*K] of T (t = 0 only; the genes' twin is the exchange buffer)
    DevBuf s_theta, s_beta, s_beta_next;            // double[K] column sums of E[theta], E[beta]; beta's double-buffered (beta_parity)
    DevBuf wave_out, scalars;                       // llh per wave; scalars[0]=llh sum
    // the loss pass's two results land in pinned host memory that the device writes directly: the reduction kernels
    // store there, the host reads after the stream has drained -- no copy of 24 bytes out of pageable memory per check
    double *loss_host = nullptr;
    DevBuf dual_order;                              // merged launch order of both plans' tasks (or empty)
    DevBuf dual_queue;                              // persistent dual launch: {next slot, workgroups done}, self-zeroing
    DevBuf clock_probe;                             // 5 x u64: shader cycles, constant-rate ticks, 2 start stamps, launches (sweep_impl.h)
    int64_t dual_slots = 0;
    bool use_tile = false, want_tile = true;
    int64_t nnz = 0;
    double gammaln_sum = 0.0;
    int64_t n_rounded = 0, n_zero = 0;              // upload facts: values rounded to float32; stored zeros
    DevBuf zero_row, zero_col;                      // positions of explicitly stored zeros (loss only)
    DevBuf elbo_part, elbo_sums;                    // ELBO: Gamma-term block partials, their sums (elbo_terms)
    // Per-row loss (loss_rows): scratch of its own, made at the first call, gone with the matrix.
    DevBuf rows_rec;                                // the MODE_LLH_ROWS sweep's records, ROW_REC doubles per partial-row slot / chunk
    DevBuf rows_out;                                // [n llh | n lgamma | n count (int64)] of the axis asked for
    // the stored zeros sorted by an axis' rows (upload order within a row): a segment per row that has any
    struct ZeroRows { DevBuf seg_major, seg_ptr, minor; int n_seg = 0; bool built = false; };
    ZeroRows zero_rows[2];
    bool have_coo = false;
    int pending_init = 0;  // 0 none, 1 dense accumulators, 2 chunk partials
    int beta_parity = 0;               // swaps of the sum-of-beta buffers mod 2: which cached graph fits (schpf_ctx::graphs)
    bool eager_since_upload = false;   // one eager iteration has run on this plan (kernel attributes are set)
    // small problems: the update kernels sum the other side's per-block column sums themselves and the
    // two reduce launches of an iteration are skipped; s_theta / s_beta are then brought up to date
    // only when a path that reads them comes along (sums_stale)
    bool sums_stale = false;
    // Minibatch CAVI without re-uploads (scHPF_.py:643-650): an engine that was told to keep_rows() holds, beside
    // its plans, the matrix once more as a (row, col)-sorted device copy; a batch engine's upload_rows(source,
    // rows) gathers its rows from there and builds its plans from device arrays -- no host slicing, no PCIe.
    bool rows_packed_ok = true;
    DevBuf rows_ptr, rows_col, rows_val;            // int64[N + 1], int32[nnz], float[nnz]; host copy of rows_ptr: the cell tile plan's mptr
    bool have_loss_constants = true;                // false after upload_rows (no lgamma sum / stored-zero list for a batch)
    int cu_count = 256;
    DevBuf gammaln_part;
    static constexpr int UPD_BLOCKS = 2048;
    static constexpr size_t TABLE_PAD = 256 * 1024;

    // The COO's index arrays start their trip over PCIe on a helper thread and a copy stream of its own
    // while the calling thread is still validating / converting the values and sampling the block loads:
    // the copy does not care whether the indices are in range, only the plan kernels do (and they run after
    // the validation has passed).
    struct EarlyIndexCopy {
        DevBuf d_row, d_col;
        std::thread worker;
        std::string error;
        double seconds = 0.0;
        bool started = false;
        void start(int device, int64_t n, const int32_t *row, const int32_t *col)
        {
            d_row.alloc((size_t)n * 4); d_col.alloc((size_t)n * 4);
            started = true;
            worker = std::thread([this, device, n, row, col] {
                const double t0 = now_s();
                hipStream_t cs = nullptr;
                hipError_t e = hipSetDevice(device);
                if (e == hipSuccess) e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
                if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_col.p, col, (size_t)n * 4, hipMemcpyHostToDevice, cs);
                if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_row.p, row, (size_t)n * 4, hipMemcpyHostToDevice, cs);
                if (e == hipSuccess) e = hipStreamSynchronize(cs);
                if (cs) (void)hipStreamDestroy(cs);
                if (e != hipSuccess) error = std::string("H2D of the COO indices failed: ") + hipGetErrorString(e);
                seconds = now_s() - t0;
            });
        }
        void join() { if (worker.joinable()) worker.join(); }
        ~EarlyIndexCopy() { join(); }
    };
    Engine(int device_, void *stream_, int dtype_, int N_, int G_, int K_)
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
    void choose_plan(bool tile)   // which kind of plan this upload builds, for both sides
    {
        use_tile = tile;
        for (Side &sd : side) sd.active = tile ? static_cast<PlanFacts *>(&sd.tile) : &sd.plan;
    }
    // the engine holds no count matrix any more: plans, row copy and captured graphs released; step / loss calls
    // raise until the next successful upload
    void forget_matrix()
    {
        have_coo = false;
        drop_graphs();
        HIPCHK(hipStreamSynchronize(stream));
        for (Side &sd : side) { sd.plan = PlanDev(); sd.tile = TileDev(); sd.count.release(); }
        dual_order.release(); dual_slots = 0;
        rows_ptr.release(); rows_col.release(); rows_val.release();
        zero_row.release(); zero_col.release();
        rows_rec.release(); rows_out.release();
        for (ZeroRows &z : zero_rows) z = ZeroRows();
        pending_init = 0;
        eager_since_upload = false;
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

    void build_plan(PlanDev &pd, int64_t nnz_, const int32_t *major, const int32_t *minor, const float *val,
                    int n_major, int n_minor, int windows, int chunk_len)
    {
        schpf::build_sweep_plan(nnz_, major, minor, val, n_major, n_minor, LPC, chunk_len, windows, true,
                                pd.host);
        auto &h = pd.host;
        pd.launch = h.n_waves;
        pd.entry_slots = (int64_t)h.entries.size() / 2;
        pd.windows = h.n_windows;
        // a row's partial rows are its chunks cptr[row] .. cptr[row + 1]
        std::vector<int32_t> first(h.cptr.begin(), h.cptr.end() - 1), count((size_t)n_major);
        for (int m = 0; m < n_major; ++m) count[(size_t)m] = h.cptr[(size_t)m + 1] - h.cptr[(size_t)m];
        pd.part.n = h.n_chunks;   // stride 1
        upload(pd.entries, h.entries, stream);
        upload(pd.slice_off, h.slice_off, stream);
        upload(pd.slice_steps, h.slice_steps, stream);
        upload(pd.chunk_major, h.chunk_major, stream);
        upload(pd.chunk_natid, h.chunk_natid, stream);
        upload(pd.wave_slice, h.wave_slice, stream);
        upload(pd.part.first, first, stream);
        upload(pd.part.count, count, stream);
        pd.part.rows.alloc((size_t)std::max<int64_t>(h.n_chunks, 1) * KP * sizeof(T), true, stream);
        HIPCHK(hipStreamSynchronize(stream));
        pd.mptr = std::move(h.mptr); pd.order = std::move(h.order);
        schpf::BigVec<uint32_t>().swap(h.entries);
        std::vector<int32_t>().swap(h.chunk_major);
        std::vector<int32_t>().swap(h.chunk_natid);
        std::vector<int32_t>().swap(h.wave_slice);
        std::vector<int64_t>().swap(h.slice_off);
        std::vector<int32_t>().swap(h.slice_steps);
    }

    // Tasks of the loss pass: the sub-ranges of the iteration's tasks that policy.cpp loss_cut chose, longest first
    void loss_tasks(TileDev &td, const UploadJob &job)
    {
        auto &h = td.host;
        td.llh = TaskList();
        const schpf::LossCut cut = schpf::loss_cut(problem(job), tuning, h);
        td.llh_model = cut.model;
        if (cut.parts <= 1) return;
        const int wpb = h.wpb, W = h.n_windows;
        const std::vector<int32_t> &wwork = cut.window_work;
        std::vector<int> cuts;
        std::vector<int32_t> blk, w0s, w1s, ends, order;
        std::vector<int64_t> woff;
        std::vector<double> work;
        for (int64_t t = 0; t < h.n_tasks; ++t) {
            const int b = h.task_block[(size_t)t], a1 = h.task_w1[(size_t)t];
            schpf::loss_cut_points(h, t, cut.parts, cuts);
            std::vector<int64_t> off((size_t)wpb);
            for (int v = 0; v < wpb; ++v) off[(size_t)v] = h.task_wave_off[(size_t)t * wpb + v];
            for (size_t p = 0; p + 1 < cuts.size(); ++p) {
                blk.push_back(b); w0s.push_back(cuts[p]); w1s.push_back(cuts[p + 1]); ends.push_back(a1);
                for (int v = 0; v < wpb; ++v) woff.push_back(off[(size_t)v]);
                double wk = 0.0;
                for (int w = cuts[p]; w < cuts[p + 1]; ++w) {
                    for (int v = 0; v < wpb; ++v)
                        off[(size_t)v] += schpf::tile_stored_steps(h, h.steps[((size_t)b * wpb + v) * W + w]) * h.gpw;
                    wk += wwork[(size_t)b * W + w];
                }
                work.push_back(wk);
            }
        }
        order.resize(blk.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return work[(size_t)x] > work[(size_t)y]; });
        TaskList &tl = td.llh;
        tl.n = (int64_t)blk.size();
        upload(tl.block, blk, stream); upload(tl.w0, w0s, stream); upload(tl.w1, w1s, stream);
        upload(tl.stage_end, ends, stream); upload(tl.wave_off, woff, stream); upload(tl.order, order, stream);
        HIPCHK(hipStreamSynchronize(stream));
    }

    // the small arrays of a tile plan (its entries and steps are on the device already)
    void finish_tile(TileDev &td, const UploadJob &job)
    {
        auto &h = td.host;
        const int wpb = h.wpb;
        td.threads = 64 * wpb;
        td.lds_bytes = h.ring > 1 ? (size_t)h.ring * h.slot16 * 16 : (size_t)h.win_rows * KP * sizeof(T);
        td.packed = h.packed;
        loss_tasks(td, job);
        TaskList &tl = td.tasks;
        td.launch = tl.n = h.n_tasks;
        td.n_wave_out = std::max<int64_t>(tl.n, td.llh.n) * wpb;
        td.windows = h.n_windows;
        td.part.stride = h.pstride; td.part.n = h.n_partial_rows;
        upload(td.block_rows, h.block_rows, stream);
        upload(tl.block, h.task_block, stream);
        upload(tl.w0, h.task_w0, stream);
        upload(tl.w1, h.task_w1, stream);
        upload(tl.wave_off, h.task_wave_off, stream);
        upload(tl.order, h.task_order, stream);
        upload(td.part.first, h.pfirst, stream);
        upload(td.part.count, h.pcount, stream);
        td.part.rows.alloc((size_t)std::max<int64_t>(h.n_partial_rows, 1) * KP * sizeof(T), true, stream);
        HIPCHK(hipStreamSynchronize(stream));
        td.mptr = std::move(h.mptr); td.order = std::move(h.order);
        std::vector<uint16_t>().swap(h.steps);
        std::vector<int64_t>().swap(h.task_wave_off);
    }

    // What the policy is told: the engine, and of the matrix what this upload says
    schpf::Problem problem(const UploadJob &job) const
    {
        return {N, G, K, (int)sizeof(T), job.nnz, cu_count, LPC, NV, KL, KP, expect_sharded, transient, want_rows,
                job.batch_rows, job.balance};
    }
    // ... and after the upload (loss_side, sweep_bytes): the matrix the engine holds.  policy.cpp loss_side reads the
    // engine's constants only, so the per-upload fields are simply unset
    schpf::Problem problem() const { return problem(UploadJob{nnz}); }

    // The shapes of both tile plans, once per upload, for whichever builder runs.  sample: the histograms of the COO's
    // sampled indices for the task-range model, from wherever the COO lies (policy.h); empty: no ranges (batch rows)
    void plan_shapes(UploadJob &job, const schpf::SampleHistograms &sample) const
    {
        if (!sample || !schpf::choose_ranges(problem(job), tuning, sample, job.ranges, job.half)) {
            job.ranges[0] = job.ranges[1] = 0;
            job.half[0] = job.half[1] = -1;
        }
        for (int s = 0; s < 2; ++s) {
            const schpf::TileShape &sh = job.shape[s] =
                schpf::tile_shape(problem(job), tuning, side[s].n, side[1 - s].n, job.ranges[s], job.half[s]);
            job.balanced[s] = job.balance && sh.ring <= 1 && sh.waves_per_block >= 12;   // the balanced kernels are 1024-thread ones
        }
    }

    // Both tile plans built by device passes over a COO that is in HBM (plan_device.hip): same plans, bit for bit, as
    // tiles_from_host_coo(); SCHPF_DEVICE_PLAN=0 selects the host builder for schpf_upload_coo.
    void tiles_from_device_coo(const UploadJob &job, const int32_t *d_row, const int32_t *d_col, const float *d_val)
    {
        // per side: its index array is the major one, the other side's the minor one
        const int32_t *const d_idx[2] = {d_row, d_col};
        const int64_t nz = job.nnz;
        auto build_side = [&](int si, hipStream_t st) {
            TileDev &td = side[si].tile;
            void *e = nullptr, *s = nullptr, *o = nullptr;
            size_t eb = 0;
            bool presorted = job.sorted[si];
            const int32_t *d_major = d_idx[si], *d_minor = d_idx[1 - si];
            const schpf::TileShape &sh = job.shape[si];
            const int n_major = side[si].n;
            int n_minor_plan = side[1 - si].n;
            DevBuf vminor;
            td.minor_of.release(); td.n_virtual = 0;
            if (job.balanced[si]) {
                const double tb = now_s();
                schpf::BalanceGeometry geo;
                void *mo = nullptr;
                // the balancing needs ~20 bytes per nonzero of scratch and 4 bytes per (block, minor row) for good: a matrix
                // that leaves no room for that is planned by index instead (the shape is valid for either)
                bool balanced = true;
                try {
                    vminor.alloc((size_t)nz * 4);
                    schpf::balance_windows_device((void *)st, nz, d_major, d_minor, n_major, n_minor_plan, sh,
                                                  vminor.as<int32_t>(), &mo, geo);
                } catch (const std::invalid_argument &) {
                    throw;
                } catch (const std::exception &e) {
                    (void)hipGetLastError();
                    balanced = false;
                    if (tuning.verbose)
                        fprintf(stderr, "[schpf_hip]   balanced windows, side %d: not built (%s); windows by index\n", si, e.what());
                }
                if (balanced) {
                    td.minor_of.adopt(mo, (size_t)geo.n_blocks * geo.n_virtual * 4);
                    td.n_virtual = geo.n_virtual;
                    d_minor = vminor.as<int32_t>();
                    n_minor_plan = geo.n_virtual;
                    presorted = false;
                } else vminor.release();
                if (tuning.verbose)
                    fprintf(stderr, "[schpf_hip]   balanced windows, side %d: %d sections of %d windows, %.3f s\n", si,
                            geo.n_sections, geo.D, now_s() - tb);
            }
            schpf::build_tile_plan_device((void *)st, nz, d_major, d_minor, d_val,
                                          presorted, job.packed_ok, n_major, n_minor_plan,
                                          sh, td.host, &e, &eb, &s, &o);
            td.entries.adopt(e, eb);
            td.steps.adopt(s, td.host.steps.size() * 2);
            td.order_dev.adopt(o, o ? (size_t)nz * 4 : 0);
            td.order_identity = presorted;
            td.entry_slots = (int64_t)(eb / 4) / (td.host.packed ? 1 : 2);
        };
        HIPCHK(hipStreamSynchronize(stream));   // the COO is on the device before either builder reads it
        // the two orientations are independent (the COO is only read): the gene side on a helper thread with a
        // stream of its own, so that the builders' host round trips (run pointers, step counts, allocations) and
        // their short kernels overlap instead of adding up
        on_both_sides(device, stream, true, build_side);
        for (Side &sd : side) finish_tile(sd.tile, job);
        build_dual_order();
    }

    // Both tile plans from the host builder (plan.cpp): the two orientations concurrently (each with its own thread
    // team), then uploaded one after the other on the context's stream
    void tiles_from_host_coo(const UploadJob &job, const int32_t *row, const int32_t *col, const float *val)
    {
        const int32_t *const idx[2] = {row, col};   // per side: its index array is the major one, the other's the minor one
        double secs[2] = {0.0, 0.0};
        // balanced windows: the builder runs on the block's virtual numbering of the minor rows (plan.h)
        std::vector<int32_t> mo[2];
        on_both_sides(device, stream, false, [&](int s, hipStream_t) {
            const double t0 = now_s();
            const int32_t *major = idx[s], *minor = idx[1 - s];
            const int n_major = side[s].n, n_minor = side[1 - s].n;
            const schpf::TileShape &sh = job.shape[s];
            TileDev &td = side[s].tile;
            td.n_virtual = 0;
            if (job.balanced[s]) {
                schpf::BigVec<int32_t> vminor;
                schpf::BalanceGeometry geo;
                schpf::balance_windows_host(job.nnz, major, minor, n_major, n_minor, sh, vminor, mo[s], geo);
                td.n_virtual = geo.n_virtual;
                schpf::build_tile_plan(job.nnz, major, vminor.data(), val, n_major, geo.n_virtual, sh, true, td.host);
            } else {
                schpf::build_tile_plan(job.nnz, major, minor, val, n_major, n_minor, sh, true, td.host);
            }
            secs[s] = now_s() - t0;
        });
        for (int s = 0; s < 2; ++s) {   // device half: upload the host-built arrays, allocate the partials
            TileDev &td = side[s].tile;
            const double t1 = now_s();
            auto &h = td.host;
            td.entry_slots = (int64_t)h.entries.size() / (h.packed ? 1 : 2);
            upload(td.entries, h.entries, stream);
            upload(td.steps, h.steps, stream);
            finish_tile(td, job);
            if (tuning.verbose)
                fprintf(stderr, "[schpf_hip]   tile plan %d x %d: host build %.3f s, H2D %.3f s (%.2f GB entries)\n",
                        h.n_major, h.n_minor, secs[s], now_s() - t1, h.entries.size() * 4e-9);
            schpf::BigVec<uint32_t>().swap(h.entries);
        }
        for (int s = 0; s < 2; ++s) {
            TileDev &td = side[s].tile;
            td.minor_of.release();
            mo[s].resize(mo[s].size() + 16, -1);   // a list is copied in 16-byte pieces: slack behind the last one
            if (td.n_virtual) upload(td.minor_of, mo[s], stream);
        }
        HIPCHK(hipStreamSynchronize(stream));
        build_dual_order();
    }

    void build_dual_order()
    {
        // Both sweeps of an iteration in one launch (kernels.h launch_tile_sweep_dual) when the two
        // plans agree on the workgroup shape: slots = all tasks of both plans, longest first.  Not symmetric: the kernel
        // takes (cell args, gene args) in that order and a slot names a cell task as `task`, a gene task as `~task`
        dual_slots = 0;
        dual_order.release();
        const TileDev &tc = side[0].tile, &tg = side[1].tile;
        if (tuning.dual && tc.threads == tg.threads && tc.packed == tg.packed && (tc.n_virtual != 0) == (tg.n_virtual != 0)) {
            const auto &hc = tc.host, &hg = tg.host;
            std::vector<int32_t> ord;
            ord.reserve((size_t)(hc.n_tasks + hg.n_tasks));
            size_t i = 0, j = 0;   // merge of two lists already sorted by decreasing work
            while (i < hc.task_order.size() || j < hg.task_order.size()) {
                const bool take_cell = j >= hg.task_order.size() ||
                    (i < hc.task_order.size() &&
                     hc.task_work[(size_t)hc.task_order[i]] >= hg.task_work[(size_t)hg.task_order[j]]);
                if (take_cell) ord.push_back(hc.task_order[i++]);
                else ord.push_back(~hg.task_order[j++]);
            }
            dual_slots = (int64_t)ord.size();
            if (dual_slots > 0) { upload(dual_order, ord, stream); HIPCHK(hipStreamSynchronize(stream)); }
        }
    }

    // The upload's constants, from the values on the device: sum lgamma(x + 1), the constant term of the loss
    // (hpf_numba.py:49-50), into scalars[1]; and the ELBO shift terms (elbo_terms), the stored counts of every cell and
    // every gene, summed over each plan's (major, minor)-sorted runs -- once per upload, N + G doubles.
    // Returns the wall time of the count sums.
    double loss_constants(const float *d_values)
    {
        const int nb = 512;
        if (!gammaln_part.p) gammaln_part.alloc(nb * sizeof(double));
        HIPCHK(schpf::launch_gammaln_sum(d_values, nnz, gammaln_part.as<double>(), nb, stream));
        HIPCHK(schpf::launch_sum_doubles(gammaln_part.as<double>(), nb, scalars.as<double>() + 1, stream));
        const double t0 = now_s();
        for (int s = 0; s < 2; ++s) {
            Side &sd = side[s];
            DevBuf scratch, mp;
            const int *ord = nullptr;
            if (!sd.active->order_identity) ord = order_of(s, scratch);
            upload(mp, major_ptr(s), stream);
            sd.count.alloc((size_t)sd.n * sizeof(double));
            HIPCHK(schpf::launch_count_sums(d_values, ord, mp.as<int64_t>(), sd.n, sd.count.as<double>(), stream));
            HIPCHK(hipStreamSynchronize(stream));   // scratch and mp die with this scope
        }
        return now_s() - t0;
    }

    static double now_s()
    {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }

    // The engine now holds the matrix whose plans were just built.  n_out: doubles a loss pass leaves in wave_out.
    // loss_constants: false for gathered batch rows, whose loss is the source engine's business (no lgamma sum, no
    // stored-zero list)
    void holds_matrix(int64_t n_out, bool loss_constants)
    {
        wave_out.alloc((size_t)std::max<int64_t>(n_out, 1) * sizeof(double), true, stream);
        HIPCHK(hipStreamSynchronize(stream));
        if (!loss_constants) {
            n_rounded = 0; n_zero = 0;
            zero_row.release(); zero_col.release();
        }
        have_loss_constants = loss_constants;
        have_coo = true;
        pending_init = 0;
        drop_graphs();
        eager_since_upload = false;
    }

    // This engine's matrix := the rows `rows` (in that order) of `source`'s, gathered on the device
    void upload_rows(schpf_ctx *source_, const int32_t *rows, int n_rows) override
    {
        Engine<T> *src = dynamic_cast<Engine<T> *>(source_);
        if (!src) throw std::invalid_argument("the source engine must have this engine's dtype");
        if (!src->rows_ptr.p || !src->have_coo) throw std::logic_error("the source keeps no rows (schpf_keep_rows before its upload)");
        if (src == this) throw std::invalid_argument("an engine cannot gather batch rows from itself");
        if (src->device != device) throw std::invalid_argument("source and batch engine must be on one device");
        if (src->G != G || src->K != K) throw std::invalid_argument("source and batch engine differ in genes or factors");
        if (n_rows != N) throw std::invalid_argument("n_rows must be the number of cells the batch engine was created with");
        if (!want_tile) throw std::invalid_argument("upload_rows needs the tile plan");
        const std::vector<int64_t> &sp = src->side[0].tile.mptr;   // host copy of src->rows_ptr
        std::vector<int64_t> dp((size_t)n_rows + 1, 0);
        for (int i = 0; i < n_rows; ++i) {
            if (rows[i] < 0 || rows[i] >= src->N) throw std::invalid_argument("batch row out of range");
            dp[(size_t)i + 1] = dp[(size_t)i] + (sp[(size_t)rows[i] + 1] - sp[(size_t)rows[i]]);
        }
        forget_matrix();                  // a failed plan build must not leave have_coo set over empty plans
        // a batch is planned every iteration, the cheapest way: no balanced windows, no task ranges, no loss tasks.
        // Its rows come in batch order with their columns ascending: sorted by (row, col) already
        UploadJob job;
        job.nnz = dp[(size_t)n_rows];
        job.batch_rows = true;
        job.packed_ok = src->rows_packed_ok;
        job.sorted[1] = false;
        nnz = job.nnz;
        std::vector<int32_t> rv(rows, rows + n_rows);
        DevBuf d_rows, d_dp, d_row, d_col, d_val;
        upload(d_rows, rv, stream);
        upload(d_dp, dp, stream);
        d_row.alloc((size_t)nnz * 4); d_col.alloc((size_t)nnz * 4); d_val.alloc((size_t)nnz * 4);
        HIPCHK(schpf::launch_gather_rows(d_rows.as<int>(), n_rows, src->rows_ptr.as<int64_t>(), src->rows_col.as<int>(),
                                         src->rows_val.as<float>(), d_dp.as<int64_t>(), d_row.as<int>(), d_col.as<int>(),
                                         d_val.as<float>(), stream));
        choose_plan(true);
        plan_shapes(job, nullptr);
        tiles_from_device_coo(job, d_row.as<int32_t>(), d_col.as<int32_t>(), d_val.as<float>());
        holds_matrix(side[0].tile.n_wave_out, false);
    }

    void upload_coo(int64_t nnz_, const int32_t *row, const int32_t *col, const void *val, int kind) override
    {
        const double t_start = now_s();
        if (nnz_ < 0 || nnz_ >= (int64_t)1 << 31) throw std::invalid_argument("nnz must be < 2^31");
        if (kind < SCHPF_VAL_I32 || kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
        // whatever the engine held is discarded on every path below: let go of it BEFORE anything new is allocated
        // (a re-upload onto a live engine would otherwise peak at the old plans + the new indices), and an upload
        // that fails leaves an engine without a matrix, not one with half of the old one
        forget_matrix();
        // balanced windows (plan.h): for uploads of a whole matrix; not for an engine that keeps a (row, col)-sorted copy
        // (the plans' own order is then the virtual one) nor for one whose matrix is replaced every iteration
        UploadJob job;
        job.nnz = nnz_;
        job.balance = want_tile && schpf::balance_windows(problem(job), tuning);
        EarlyIndexCopy early;
        const bool device_plans = want_tile && tuning.device_plan;
        if (device_plans) early.start(device, nnz_, row, col);
        schpf::BigVec<float> v((size_t)nnz_);   // no serial zero-fill: written by the threaded pass below
        n_rounded = 0;
        std::vector<int32_t> zrow, zcol;         // explicitly stored zeros (rare): see zero_rate_sum()
        {   // validate + convert, in parallel slabs (first offending entry per slab is reported)
            const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(schpf::host_threads(), nnz_ / 65536 + 1));
            std::vector<int64_t> bad_val((size_t)nth, -1), bad_idx((size_t)nth, -1), rounded((size_t)nth, 0);
            std::vector<std::vector<int32_t>> zr((size_t)nth), zc((size_t)nth);
            std::vector<char> wide((size_t)nth, 0);   // a count that does not fit the packed 16-bit entry format
            std::vector<std::thread> th;
            for (int t = 0; t < nth; ++t)
                th.emplace_back([&, t] {
                    const int64_t b = nnz_ * t / nth, e = nnz_ * (t + 1) / nth;
                    for (int64_t i = b; i < e; ++i) {
                        const double d = read_count(val, kind, i);
                        const float f = (float)d;
                        // the reference takes any X.data (hpf_numba.py:98-112 only multiplies by it); what
                        // cannot be a Poisson observation at all (negative, NaN, inf) is refused
                        if (!(d >= 0.0 && f <= 3.0e38f) && bad_val[(size_t)t] < 0) bad_val[(size_t)t] = i;
                        if ((row[i] < 0 || row[i] >= N || col[i] < 0 || col[i] >= G) && bad_idx[(size_t)t] < 0)
                            bad_idx[(size_t)t] = i;
                        else if (d == 0.0) { zr[(size_t)t].push_back(row[i]); zc[(size_t)t].push_back(col[i]); }
                        if ((double)f != d) ++rounded[(size_t)t];
                        v[(size_t)i] = f;
                        if (!(f <= 65535.0f) || f != (float)(uint32_t)f) wide[(size_t)t] = 1;
                    }
                });
            for (auto &x : th) x.join();
            for (int t = 0; t < nth; ++t) job.packed_ok = job.packed_ok && !wide[(size_t)t];
            for (int t = 0; t < nth; ++t) {
                if (bad_idx[(size_t)t] >= 0)
                    throw std::invalid_argument("COO index out of range at entry " + std::to_string(bad_idx[(size_t)t]));
                if (bad_val[(size_t)t] >= 0)
                    throw std::invalid_argument("X.data must be finite and >= 0; offending entry " +
                                                std::to_string(bad_val[(size_t)t]));
                n_rounded += rounded[(size_t)t];
                zrow.insert(zrow.end(), zr[(size_t)t].begin(), zr[(size_t)t].end());
                zcol.insert(zcol.end(), zc[(size_t)t].begin(), zc[(size_t)t].end());
            }
        }
        n_zero = (int64_t)zrow.size();
        upload(zero_row, zrow, stream);
        upload(zero_col, zcol, stream);
        const double t_valid = now_s();
        nnz = nnz_;
        choose_plan(want_tile);
        DevBuf d_val;   // the values on the device: beside the indices for the device builder, afterwards for the others
        if (device_plans) {
            plan_shapes(job, host_samples(job, row, col));
            schpf::coo_order_flags(nnz, row, col, job.sorted[0], job.sorted[1]);
            d_val.alloc((size_t)nnz * 4);
            if (nnz > 0) HIPCHK(hipMemcpyAsync(d_val.p, v.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, stream));
            early.join();                                  // the indices went up beside the validation pass
            if (!early.error.empty()) throw HipError(early.error);
            const double t1 = now_s();
            tiles_from_device_coo(job, static_cast<const int32_t *>(early.d_row.p), static_cast<const int32_t *>(early.d_col.p), d_val.as<float>());
            if (tuning.verbose)
                fprintf(stderr, "[schpf_hip]   tile plans on the device: ranges + H2D of the values %.3f s (indices: %.3f s on the "
                        "helper thread, from the start of the upload), both plans %.3f s (%.2f GB entries)\n",
                        t1 - t_valid, early.seconds, now_s() - t1, (side[0].tile.entries.bytes + side[1].tile.entries.bytes) * 1e-9);
        } else plans_from_host_coo(job, row, col, v.data());
        const double t_plans = now_s();
        // the device builder's values are still resident: no second trip over PCIe.  Host-built plans: they go up now
        if (!device_plans) upload(d_val, v, stream);
        const double count_seconds = finish_upload(job, device_plans ? static_cast<const int32_t *>(early.d_col.p) : nullptr, d_val.as<float>());
        d_val.release();
        if (tuning.verbose)
            fprintf(stderr, "[schpf_hip] upload_coo nnz=%lld: validate %.3f s, plans+H2D %.3f s, gammaln %.3f s (%d host threads); "
                    "ELBO count sums %.4f s of it\n",
                    (long long)nnz, t_valid - t_start, t_plans - t_valid, now_s() - t_plans, schpf::host_threads(),
                    count_seconds);
    }

    // the task-range model's samples from a COO on the host
    schpf::SampleHistograms host_samples(const UploadJob &job, const int32_t *row, const int32_t *col) const
    {
        return [this, &job, row, col](int64_t stride, std::vector<int32_t> hist[2]) {
            hist[0] = schpf::sample_histogram(job.nnz, row, N, stride);
            hist[1] = schpf::sample_histogram(job.nnz, col, G, stride);
        };
    }

    // Both plans from the host builders over a COO on the host: tile plans (SCHPF_DEVICE_PLAN=0) or gather plans
    void plans_from_host_coo(UploadJob &job, const int32_t *row, const int32_t *col, const float *val)
    {
        if (use_tile) {
            plan_shapes(job, host_samples(job, row, col));
            tiles_from_host_coo(job, row, col, val);
            return;
        }
        const int32_t *const idx[2] = {row, col};
        const int chunk = schpf::gather_chunk_len(problem(job));
        for (int s = 0; s < 2; ++s)   // windows: by the size of the minor side's table
            build_plan(side[s].plan, job.nnz, idx[s], idx[1 - s], val, side[s].n, side[1 - s].n,
                       schpf::pick_windows((size_t)side[1 - s].n * KP * sizeof(T)), chunk);
        side[0].plan.n_wave_out = side[0].plan.launch;   // one double per wavefront; the cell plan only (PlanFacts)
    }

    // What every whole-matrix upload does once its plans stand: the loss constants from the values on the device, the
    // (row, col)-sorted copy minibatches gather their rows from (d_col: the column indices on the device in the
    // caller's order, or nullptr where the plans were built on the host), and the engine holds the matrix.  Returns
    // the wall time of the count sums
    double finish_upload(const UploadJob &job, const int32_t *d_col, const float *d_val)
    {
        const double count_seconds = loss_constants(d_val);
        if (d_col && want_rows) {
            rows_col.alloc((size_t)nnz * 4); rows_val.alloc((size_t)nnz * 4);
            const TileDev &tc = side[0].tile;   // the cell plan's order; rows_ptr's host copy stays tc.mptr
            HIPCHK(schpf::launch_gather_by_order(tc.order_identity ? nullptr : tc.order_dev.as<int>(), d_col, d_val, nnz,
                                                 rows_col.as<int>(), rows_val.as<float>(), stream));
            upload(rows_ptr, tc.mptr, stream);
            rows_packed_ok = job.packed_ok;
            HIPCHK(hipStreamSynchronize(stream));
        }
        HIPCHK(hipMemcpyAsync(&gammaln_sum, scalars.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost,
                              stream));
        HIPCHK(hipStreamSynchronize(stream));
        holds_matrix(std::max(side[0].active->n_wave_out, side[1].active->n_wave_out), true);   // the loss pass sweeps either plan
        return count_seconds;
    }

    // The matrix is in HBM already (schpf_upload_coo_device / schpf_upload_csr_device): the stages
    // upload_coo runs on host threads -- validate + convert, the stored-zero list, the order flags, the task-range
    // samples -- as device passes (upload_device.h), arriving at tiles_from_device_coo with the job a host upload of the
    // same entries in the same order makes.  Nothing of O(nnz) crosses PCIe.  Host-built plans (SCHPF_PLAN=gather,
    // SCHPF_DEVICE_PLAN=0) are the cross-check: the converted triples are staged to the host for those builders.
    // Errors: the smallest offending entry; an index error goes before a value error.
    void upload_device(int64_t nnz_, const void *rows, int indptr_kind, const void *col, int idx_kind, const void *val,
                       int val_kind) override
    {
        const double t_start = now_s();
        const bool csr = indptr_kind >= 0;
        if (nnz_ < 0 || nnz_ >= (int64_t)1 << 31) throw std::invalid_argument("nnz must be < 2^31");
        if (val_kind < SCHPF_VAL_I32 || val_kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
        for (int k : {idx_kind, csr ? indptr_kind : idx_kind})
            if (k != SCHPF_IDX_I32 && k != SCHPF_IDX_I64) throw std::invalid_argument("unknown index kind");
        forget_matrix();
        UploadJob job;
        job.nnz = nnz_;
        job.balance = want_tile && schpf::balance_windows(problem(job), tuning);
        n_rounded = 0; n_zero = 0;
        // engine-owned int32 / float32 copies, only of what the caller did not hand over in that type already (an empty
        // matrix may come with NULL pointers: the builders then get the engine's own empty buffers)
        DevBuf own_row, own_col, own_val;
        if (csr) {
            if (!schpf::csr_indptr_valid(stream, rows, indptr_kind, N, nnz_))
                throw std::invalid_argument("CSR indptr must be non-decreasing from 0 to nnz");
            own_row.alloc((size_t)nnz_ * 4);
            schpf::csr_expand_rows(stream, rows, indptr_kind, N, nnz_, own_row.as<int32_t>());
        } else if (idx_kind != SCHPF_IDX_I32 || nnz_ == 0) own_row.alloc((size_t)nnz_ * 4);
        if (idx_kind != SCHPF_IDX_I32 || nnz_ == 0) own_col.alloc((size_t)nnz_ * 4);
        if (val_kind != SCHPF_VAL_F32 || nnz_ == 0) own_val.alloc((size_t)nnz_ * 4);
        const schpf::ConvertStats cs =
            schpf::convert_coo_device(stream, nnz_, csr ? own_row.p : rows, csr ? SCHPF_IDX_I32 : idx_kind, col, idx_kind, val,
                                      val_kind, N, G, csr ? nullptr : own_row.as<int32_t>(), own_col.as<int32_t>(),
                                      own_val.as<float>());
        if (cs.first_bad_index >= 0)
            throw std::invalid_argument("COO index out of range at entry " + std::to_string(cs.first_bad_index));
        if (cs.first_bad_value >= 0)
            throw std::invalid_argument("X.data must be finite and >= 0; offending entry " + std::to_string(cs.first_bad_value));
        const int32_t *d_row = own_row.p ? own_row.as<int32_t>() : static_cast<const int32_t *>(rows);
        const int32_t *d_col = own_col.p ? own_col.as<int32_t>() : static_cast<const int32_t *>(col);
        const float *d_val = own_val.p ? own_val.as<float>() : static_cast<const float *>(val);
        job.packed_ok = cs.packed_ok;
        job.sorted[0] = cs.sorted[0]; job.sorted[1] = cs.sorted[1];
        n_rounded = cs.rounded; n_zero = cs.zeros;
        zero_row.alloc((size_t)n_zero * 4); zero_col.alloc((size_t)n_zero * 4);
        schpf::compact_zeros_device(stream, nnz_, d_row, d_col, val, val_kind, n_zero, zero_row.as<int32_t>(), zero_col.as<int32_t>());
        const double t_valid = now_s();
        nnz = nnz_;
        choose_plan(want_tile);
        const bool device_plans = want_tile && tuning.device_plan;
        double t_shapes = t_valid;
        if (device_plans) {
            plan_shapes(job, [&](int64_t stride, std::vector<int32_t> hist[2]) {
                hist[0].resize((size_t)N); hist[1].resize((size_t)G);
                schpf::sample_histograms_device(stream, nnz, d_row, d_col, N, G, stride, hist[0].data(), hist[1].data());
            });
            t_shapes = now_s();
            tiles_from_device_coo(job, d_row, d_col, d_val);
        } else {
            schpf::BigVec<int32_t> h_row((size_t)nnz), h_col((size_t)nnz);
            schpf::BigVec<float> h_val((size_t)nnz);
            if (nnz > 0) {
                HIPCHK(hipMemcpyAsync(h_row.data(), d_row, (size_t)nnz * 4, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipMemcpyAsync(h_col.data(), d_col, (size_t)nnz * 4, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipMemcpyAsync(h_val.data(), d_val, (size_t)nnz * 4, hipMemcpyDeviceToHost, stream));
            }
            HIPCHK(hipStreamSynchronize(stream));
            plans_from_host_coo(job, h_row.data(), h_col.data(), h_val.data());
        }
        const double t_plans = now_s();
        const double count_seconds = finish_upload(job, device_plans ? d_col : nullptr, d_val);
        if (tuning.verbose)
            fprintf(stderr, "[schpf_hip] upload_%s_device nnz=%lld: %svalidate + convert + zeros %.3f s, order flags in it, task-range "
                    "samples %.3f s, plans %.3f s%s, gammaln %.3f s; ELBO count sums %.4f s of it\n",
                    csr ? "csr" : "coo", (long long)nnz, csr ? "row expansion + " : "", t_valid - t_start, t_shapes - t_valid,
                    t_plans - t_shapes, device_plans ? "" : " (staged to the host builders)", now_s() - t_plans, count_seconds);
    }

    // Row and column sums of the matrix the engine holds: the ELBO's count sums (loss_constants), N + G doubles
    void marginals(double *row_sums, double *col_sums) override
    {
        need_coo();
        need_loss_constants();
        double *const out[2] = {row_sums, col_sums};
        for (int s = 0; s < 2; ++s)
            if (out[s]) HIPCHK(hipMemcpyAsync(out[s], side[s].count.p, (size_t)side[s].n * sizeof(double), hipMemcpyDeviceToHost, stream));
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
        PlanDev &pd = side[s].plan;
        schpf::SweepArgs<T> a{};
        a.entries = pd.entries.as<uint4>();
        a.slice_off = pd.slice_off.as<int64_t>();
        a.slice_steps = pd.slice_steps.as<int>();
        a.chunk_major = pd.chunk_major.as<int>();
        a.chunk_natid = pd.chunk_natid.as<int>();
        a.wave_slice = pd.wave_slice.as<int>();
        table_args(a, s, mode);
        a.partials = pd.part.rows.as<T>();
        a.wave_out = wave_out.as<double>();
        a.K = K;
        return a;
    }

    // tl: the side's task list the launch walks (TileDev::tasks, or llh for a cut loss pass)
    schpf::TileArgs<T> tile_args(int s, int mode, const TaskList &tl)
    {
        TileDev &td = side[s].tile;
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
        a.wave_out = wave_out.as<double>();
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
        if (use_tile) {
            TileDev &td = side[s].tile;
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
            if (rows) a.wave_out = rows_rec.as<double>();
            HIPCHK(schpf::launch_tile_sweep<T>(a, NV, LPC, mode, td.packed ? 1 : 0, tl.n, td.threads, lds, stream));
        } else {
            PlanDev &pd = side[s].plan;
            auto a = sweep_args(s, mode);
            if (mode == schpf::MODE_LLH_ROWS) a.wave_out = rows_rec.as<double>();
            if (mode == schpf::MODE_RANDOM)
                HIPCHK(schpf::launch_random_phi<T>(a, NV, LPC, seed, s == 0 ? 1 : 0, pd.launch, stream));
            else
                HIPCHK(schpf::launch_sweep<T>(a, NV, LPC, mode, pd.launch, stream));
        }
    }

    // where the update kernel finds a side's accumulated partial rows (SRC_STRIDED)
    void partial_source(int s, schpf::UpdateArgs<T> &u)
    {
        const PartialRows &pr = side[s].active->part;
        u.partials = pr.rows.as<T>(); u.pfirst = pr.first.as<int>(); u.pcount = pr.count.as<int>(); u.pstride = pr.stride;
    }

    void need_coo() const
    {
        if (!have_coo) throw std::logic_error("no count matrix uploaded (schpf_upload_coo)");
    }
    void need_loss_constants() const
    {
        if (!have_loss_constants)
            throw std::logic_error("this engine holds gathered batch rows (schpf_upload_rows): evaluate the loss on the source");
    }
    // run pointers of a side's (major, minor)-sorted order, on the host
    const std::vector<int64_t> &major_ptr(int s) const { return side[s].active->mptr; }
    // doubles a loss / ELBO pass over side s (= loss_side()) leaves in wave_out
    int64_t n_wave_out(int s) const { return side[s].active->n_wave_out; }

    // (major, minor)-sorted position -> position in the caller's COO, on the device
    const int *order_of(int s, DevBuf &scratch)
    {
        const PlanFacts &pl = *side[s].active;
        if (pl.order_dev.p) return pl.order_dev.as<int>();
        if (pl.order_identity) {
            std::vector<int32_t> iota((size_t)nnz);
            for (int64_t j = 0; j < nnz; ++j) iota[(size_t)j] = (int32_t)j;
            upload(scratch, iota, stream);
            HIPCHK(hipStreamSynchronize(stream));   // iota dies with this scope
            return scratch.as<int>();
        }
        upload(scratch, pl.order, stream);
        return scratch.as<int>();
    }

    void init_phi_host(const double *xphi) override
    {
        need_coo();
        DevBuf dx, ord, mp;
        dx.alloc((size_t)nnz * K * sizeof(double));
        HIPCHK(hipMemcpyAsync(dx.p, xphi, (size_t)nnz * K * sizeof(double), hipMemcpyHostToDevice, stream));
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
        if (pending_init == 0 && dual_slots > 0 && do_gene && do_cell && !freeze) {   // dual_slots: tile plans only
            // both sweeps read the same old tables: one launch (timed as kind 0, see schpf_profile_read)
            ScopedTimer tm(prof, stream, 0);
            // Not symmetric: the kernel takes (cell args, gene args) in that order; dual_order names gene tasks as ~task
            const TileDev &tc = side[0].tile, &tg = side[1].tile;
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
            HIPCHK(schpf::launch_tile_sweep_dual<T>(ac, ag, dual_order.as<int>(), NV, LPC, tc.packed ? 1 : 0,
                                                    dual_slots, tc.threads, lds, queue, resident, stream));
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
            const PartialRows &pr = side[1].active->part;
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
        HIPCHK(schpf::launch_sum_doubles(wave_out.as<double>(), n_wave_out(ls), res, stream));
        // explicitly stored zeros look like padding to the sweeps (weight 0, which is what they
        // contribute to the shape updates, hpf_numba.py:97-112), but the reference's loss counts
        // them: x log r - r - lgamma(x+1) = -r (hpf_numba.py:43-50)
        if (n_zero > 0)
            HIPCHK(schpf::launch_zero_rate_sum<T>(zero_row.as<int>(), zero_col.as<int>(), n_zero, side[0].tab_e.as<T>(),
                                                  side[1].tab_e.as<T>(), K, KP, res + 2, stream));
        tm.stop();
        double h[3] = {0.0, 0.0, 0.0};
        if (!loss_host) HIPCHK(hipMemcpyAsync(h, scalars.p, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (loss_host) { h[0] = loss_host[0]; h[2] = loss_host[2]; }
        *llh = n_zero > 0 ? h[0] - h[2] : h[0];
        *gl = gammaln_sum;
        *nnz_out = nnz;
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
        HIPCHK(schpf::launch_sum_doubles(wave_out.as<double>(), n_wave_out(ls), sums + 2 * W, stream));
        const double cap_prior_shape[2] = {ap, cp};
        for (int s = 0; s < 2; ++s) {   // cells, then genes: both through the one elbo_part scratch
            const Side &sd = side[s];
            HIPCHK(schpf::launch_elbo_gamma<T>(sd.shape.as<T>(), sd.rate.as<T>(), sd.cap_shape.as<T>(), sd.cap_rate.as<T>(),
                                               sd.tab_log.as<T>(), sd.count.as<double>(), sd.n, K, KP, prior_shape(s),
                                               cap_prior_shape[s], cap_prior_rate(s), elbo_part.as<double>(), nb[s], stream));
            HIPCHK(schpf::launch_colsum_reduce(elbo_part.as<double>(), nb[s], W, sums + s * W, nullptr, 0, stream));
        }
        std::vector<double> h((size_t)(2 * W + 1));
        HIPCHK(hipMemcpyAsync(h.data(), sums, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        double rate = 0.0;
        for (int k = 0; k < K; ++k) rate += h[(size_t)k] * h[(size_t)(W + k)];
        terms[0] = h[(size_t)(2 * W)] + h[(size_t)(K + 1)] + h[(size_t)(W + K + 1)];
        terms[1] = gammaln_sum;
        terms[2] = rate;
        terms[3] = h[(size_t)K];
        terms[4] = h[(size_t)(W + K)];
    }

    // The stored zeros grouped by the rows of axis s, once per upload: sorted by row, upload order kept within a row, so
    // that one thread per row adds them in the same order on every call
    void build_zero_rows(int s)
    {
        ZeroRows &z = zero_rows[s];
        if (z.built) return;
        std::vector<int32_t> idx[2] = {std::vector<int32_t>((size_t)n_zero), std::vector<int32_t>((size_t)n_zero)};
        d2h(idx[0].data(), zero_row, (size_t)n_zero * 4, stream);
        d2h(idx[1].data(), zero_col, (size_t)n_zero * 4, stream);
        const std::vector<int32_t> &major = idx[s], &minor = idx[1 - s];
        std::vector<int64_t> perm((size_t)n_zero);
        for (int64_t i = 0; i < n_zero; ++i) perm[(size_t)i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return major[(size_t)x] < major[(size_t)y]; });
        std::vector<int32_t> seg_major, seg_ptr, mn((size_t)n_zero);
        for (int64_t j = 0; j < n_zero; ++j) {
            const int32_t m = major[(size_t)perm[(size_t)j]];
            if (seg_major.empty() || seg_major.back() != m) { seg_major.push_back(m); seg_ptr.push_back((int32_t)j); }
            mn[(size_t)j] = minor[(size_t)perm[(size_t)j]];
        }
        seg_ptr.push_back((int32_t)n_zero);
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
        const int64_t n_rec = std::max(side[0].active->part.n, side[1].active->part.n);   // one scratch for either axis
        const size_t rec_bytes = (size_t)std::max<int64_t>(n_rec, 1) * schpf::ROW_REC * sizeof(double);
        if (rows_rec.bytes < rec_bytes) rows_rec.alloc(rec_bytes);
        if (rows_out.bytes < n_max * 24) rows_out.alloc(n_max * 24);
        if (n_zero > 0) build_zero_rows(s);
        refresh_tables();
        double *d_llh = rows_out.as<double>(), *d_gl = d_llh + n;
        int64_t *d_cnt = reinterpret_cast<int64_t *>(d_gl + n);
        ScopedTimer tm(prof, stream, 2);
        run_sweep(s, schpf::MODE_LLH_ROWS);
        const PartialRows &pr = sd.active->part;
        HIPCHK(schpf::launch_row_records_reduce(rows_rec.as<double>(), pr.first.as<int>(), pr.count.as<int>(),
                                                pr.stride, sd.n, d_llh, d_gl, d_cnt, stream));
        if (n_zero > 0) {
            const ZeroRows &z = zero_rows[s];
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
        if (!use_tile) return 0;
        const TileDev &tc = side[0].tile, &tg = side[1].tile;
        const double model[2] = {tc.llh_model, tg.llh_model};
        const int64_t tasks[2] = {tc.tasks.n, tg.tasks.n};
        // the policy's question about wave_out is whether the gene plan's pass fits; the LDS figure is the cell plan's
        return schpf::loss_side(problem(), tuning, wave_out.bytes >= (size_t)tg.n_wave_out * sizeof(double), model, tasks,
                                tc.lds_bytes);
    }

    void upload_info(int64_t info[4]) override
    {
        info[0] = nnz; info[1] = n_rounded; info[2] = n_zero;
        info[3] = (side[0].active->packed ? 1 : 0) | (rows_ptr.p ? 2 : 0);   // bit 0: packed entries; bit 1: a row-sorted copy
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
        const TileDev &td = side[s].tile;
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
        if (!use_tile || !have_coo) return;
        const int64_t row = (int64_t)KP * (int64_t)sizeof(T);
        info[0] = 2 * nnz * row;
        const TileDev &tc = side[0].tile, &tg = side[1].tile;
        info[1] = (tc.entry_slots + tg.entry_slots) * row;
        info[2] = staged_bytes(0);
        info[3] = staged_bytes(1);
        info[4] = (tc.entry_slots + tg.entry_slots) * (tc.packed ? 4 : 8);
        info[5] = (tc.part.n + tg.part.n) * row;
        // what the loss pass will sweep (loss_side, loss_tasks): so that a report can say which plan and cut the model chose
        const int ls = loss_side();
        const TileDev &tl = side[ls].tile;
        info[6] = ls;
        info[7] = tl.llh.n > 0 ? tl.llh.n : tl.tasks.n;
    }

    // per-side entries come in (cell, gene) pairs; [3], [14], [15] describe the cell plan
    void plan_info(int64_t info[16]) override
    {
        info[0] = KP; info[1] = KL; info[2] = LPC;
        for (int s = 0; s < 2; ++s) {
            const PlanFacts &pl = *side[s].active;
            info[4 + s] = pl.windows; info[6 + s] = pl.part.n; info[8 + s] = pl.launch; info[10 + s] = pl.entry_slots;
        }
        info[3] = side[0].plan.host.chunk_len;
        info[12] = info[13] = info[14] = info[15] = 0;
        if (use_tile) {   // tile-only: [3] negative, rows per LDS window; ring slots per side; slot bytes; waves per block
            const schpf::TilePlanHost &hc = side[0].tile.host;
            info[3] = -hc.win_rows; info[12] = hc.ring; info[13] = side[1].tile.host.ring;
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
