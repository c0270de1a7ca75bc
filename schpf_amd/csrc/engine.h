// What an engine is made of beside its typed model state (capi.hip Engine<T>): the context the C ABI hands out, the record
// of the matrix it holds, and the upload pipeline that builds that record (upload.hip), compiled once for both dtypes.
#pragma once
#include <chrono>
#include <cstring>

#include "common.h"
#include "policy.h"
#include "rccl.h"

namespace schpf {

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A major row's partial rows -- the K-vectors a sweep accumulates for it, and the records of a MODE_LLH_ROWS pass, which
// are addressed alike -- are first[row] + j * stride, j < count[row].  Tile plans: one per (row, task) (plan.h pfirst /
// pcount / pstride); gather plans: the row's consecutive chunks, stride 1
struct PartialRows { DevBuf rows, first, count; int64_t stride = 1, n = 0; };   // rows: [n, KP] of the model dtype

// What the engine asks of an axis' plan whatever its kind (Matrix::facts); the builders fill it
struct PlanFacts {
    PartialRows part;
    std::vector<int64_t> mptr;      // run pointers of the (major, minor)-sorted order, on the host (moved out of `host`)
    // (major, minor)-sorted position -> caller's COO position: on the device (device-built plans), the identity (the
    // input was already in that order), or on the host (host-built plans; moved out of `host`)
    DevBuf order_dev; bool order_identity = false; BigVec<int32_t> order;
    int64_t launch = 0;             // size of an iteration's sweep launch: tasks (tile) / wavefronts (gather)
    // doubles a loss / ELBO pass over this plan leaves in wave_out.  Not symmetric: gather plans only ever sweep the cell
    // side for it (loss_side), so a gather plan of the gene side leaves this 0
    int64_t n_wave_out = 0, entry_slots = 0;
    int windows = 0;
    bool packed = false;            // 8-byte entries (tile plans whose counts all fit 16 bits)
};

struct PlanDev : PlanFacts {
    SweepPlanHost host;  // entries and the per-slice arrays cleared after upload; order / mptr moved to the facts
    DevBuf entries, slice_off, slice_steps, chunk_major, chunk_natid, wave_slice;
};

// The tasks a tile sweep launches, one entry per task.  stage_end: only sub-range tasks have one (kernels.h task_stage_end)
struct TaskList {
    DevBuf block, w0, w1, stage_end, wave_off;
    DevBuf order;               // tasks by decreasing work: the slot list of a persistent single-side launch
    int64_t n = 0;
};

struct TileDev : PlanFacts {
    TilePlanHost host;          // entries/steps cleared after upload; order / mptr moved to the facts
    DevBuf entries, steps, block_rows;
    TaskList tasks;             // the iteration's
    // The loss pass (MODE_LLH) writes no partial rows, so its tasks may be cut finer than the iteration's: sub-ranges of
    // the tasks' window ranges, enough of them for a few rounds of the device (Uploader::loss_tasks); n = 0: not cut
    TaskList llh;
    double llh_model = 0.0;     // modelled length of the loss pass on this plan, in step units (0: unknown)
    DevBuf minor_of;            // balanced windows (plan.h): [n_blocks * n_virtual] table row staged at a window position, or empty
    int n_virtual = 0;
    int threads = 512;
    size_t lds_bytes = 0;
};

// The matrix an engine holds: everything an upload makes and the next upload replaces, as one record.  A fresh record is
// "no matrix".  Axis 0 is the cell axis (major = cell), axis 1 the gene axis -- the numbering of Engine::side.
//
// What the cached graphs (schpf_ctx::graphs) rely on.  A captured stretch bakes device pointers in.  Those of the model
// state (Engine<T>: Side's buffers, the exchange buffer, column sums, dual_queue, clock_probe) never change after
// schpf_create.  Those of this record change only in Uploader::forget_matrix, which drops the graphs first, and during
// the upload that follows it, when no graph exists and none can be captured (have_coo is false until the record is
// complete; an upload that fails leaves a fresh record).  rows_rec, rows_out and zero_rows -- and the engine's elbo_part / elbo_sums and ppc_e / ppc_out -- may be made or grown by the
// call that needs them: only the loss, ELBO, per-row and predictive passes read them, and those are never captured.
struct Matrix {
    struct Axis {
        DevBuf count;               // ELBO: sum of the stored counts of each row of this axis, double[n]
        PlanDev plan;               // gather plan with this axis as major
        TileDev tile;               // tile plan (LDS-staged sweep) with this axis as major
    } axis[2];
    bool use_tile = false;          // which kind of plan the upload built, for both axes
    PlanFacts &facts(int s) { return use_tile ? static_cast<PlanFacts &>(axis[s].tile) : axis[s].plan; }
    const PlanFacts &facts(int s) const { return const_cast<Matrix *>(this)->facts(s); }
    bool have_coo = false;          // the record is complete: step / loss calls may run
    bool have_loss_constants = true;   // false after upload_rows (no lgamma sum / stored-zero list for a batch)
    int64_t nnz = 0;
    int64_t n_rounded = 0, n_zero = 0;   // values rounded to float32; explicitly stored zeros
    double gammaln_sum = 0.0;       // sum lgamma(x + 1), the constant term of the loss
    DevBuf gammaln_part;            // its block partials, and behind them the sum
    DevBuf dual_order;              // merged launch order of both tile plans' tasks (or empty)
    int64_t dual_slots = 0;
    DevBuf wave_out;                // what a loss / ELBO pass leaves per wave
    DevBuf zero_row, zero_col;      // positions of the stored zeros (loss only)
    // Minibatch CAVI without re-uploads (scHPF_.py:643-650): an engine that was told to keep_rows() holds, beside its
    // plans, the matrix once more as a (row, col)-sorted device copy; a batch engine's upload_rows(source, rows) gathers
    // its rows from there.  int64[N + 1], int32[nnz], float[nnz]; host copy of rows_ptr: the cell tile plan's mptr
    DevBuf rows_ptr, rows_col, rows_val;
    bool rows_packed_ok = true;
    // Per-row loss (loss_rows): scratch made at the first call
    DevBuf rows_rec;                // the MODE_LLH_ROWS sweep's records, ROW_REC doubles per partial-row slot / chunk
    DevBuf rows_out;                // [n llh | n lgamma | n count (int64)] of the axis asked for
    // the stored zeros sorted by an axis' rows (upload order within a row): a segment per row that has any
    struct ZeroRows { DevBuf seg_major, seg_ptr, minor; int n_seg = 0; bool built = false; } zero_rows[2];
};

// What one upload knows about itself.  Made by upload_coo / upload_device / upload_rows, handed down the stages by
// reference, gone with the call: nothing of it is parked in the engine.
struct UploadJob {
    int64_t nnz = 0;
    bool balance = false;              // balanced windows for this matrix (policy.cpp balance_windows)
    bool batch_rows = false;           // gathered batch rows (upload_rows): no loss constants, no loss tasks
    bool packed_ok = true;             // every count fits the packed 16-bit entry format
    bool sorted[2] = {true, true};     // the COO is already in (row, col) / (col, row) order
    int ranges[2] = {0, 0}, half[2] = {-1, -1};   // task ranges per orientation (policy.cpp choose_ranges)
    TileShape shape[2];
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

}  // namespace schpf

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
        using namespace schpf;
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
        if (comm) { (void)hipStreamSynchronize(comm_stream); (void)schpf::rccl().CommDestroy(comm); comm = nullptr; }
        if (comm_stream) { (void)hipStreamDestroy(comm_stream); comm_stream = nullptr; }
        if (ev_packed) { (void)hipEventDestroy(ev_packed); ev_packed = nullptr; }
        if (ev_reduced) { (void)hipEventDestroy(ev_reduced); ev_reduced = nullptr; }
    }
    virtual void exchange(void **p, int64_t *count) = 0;
    virtual void loss_terms(double *llh, double *gl, int64_t *nnz) = 0;
    virtual void elbo_terms(double ap, double cp, double terms[5]) = 0;
    virtual void loss_rows(int by, double *llh, double *gl, int64_t *count) = 0;
    virtual void predictive_rows(int by, double *zeros, double *rate, double *rate2) = 0;
    virtual void plan_info(int64_t info[16]) = 0;
    virtual void debug_tables(int side, void *tab_e, void *tab_log, void *tab_exp) = 0;
    virtual void upload_info(int64_t info[4]) = 0;
    virtual void profile_clock(double *shader_mhz, int64_t *launches) = 0;
    virtual void sweep_bytes(int64_t info[8]) = 0;
    double a = 0.3, c = 0.3, bp = 1.0, dp = 1.0;   // kernel arguments of the captured launches: set_hypers drops the graphs
    bool expect_sharded = false;        // schpf_hint_sharded: a rank of a sharded fit (gene-side sums leave for an all-reduce)
    bool transient = false;             // schpf_hint_transient: the matrix is replaced every iteration, plan the cheapest way
    bool want_rows = false;             // schpf_keep_rows: keep a (row, col)-sorted device copy for upload_rows
    schpf::Profiler prof;
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

namespace schpf {

// The part of an engine that needs nothing of the model dtype but its size: the matrix it holds and the three uploads
// that replace it (upload.hip).  Engine<T> (capi.hip) adds the model state and the launches that read both.
struct Uploader : schpf_ctx {
    const Tuning tuning = tuning_from_env();   // the switches, read once at schpf_create
    const size_t elem;                  // bytes of a model value: 4 / 8
    int cu_count = 256;
    bool want_tile = true;
    Matrix mx;
    int pending_init = 0;               // 0 none, 1 dense accumulators, 2 chunk partials
    bool eager_since_upload = false;    // one eager iteration has run on this plan (kernel attributes are set)

    explicit Uploader(size_t elem_) : elem(elem_) {}
    int rows_of(int s) const { return s == 0 ? N : G; }   // rows of an axis

    void upload_coo(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int kind) final;
    void upload_device(int64_t nnz, const void *rows, int indptr_kind, const void *col, int idx_kind, const void *val,
                       int val_kind) final;
    void upload_rows(schpf_ctx *source, const int32_t *rows, int n_rows) final;

    // the engine holds no count matrix any more: the record and the captured graphs released; step / loss calls raise
    // until the next successful upload
    void forget_matrix();
    // What the policy is told: the engine, and of the matrix what this upload says
    Problem problem(const UploadJob &job) const
    {
        return {N, G, K, (int)elem, job.nnz, cu_count, LPC, NV, KL, KP, expect_sharded, transient, want_rows,
                job.batch_rows, job.balance};
    }
    // ... and after the upload (loss_side, sweep_bytes): the matrix the engine holds.  policy.cpp loss_side reads the
    // engine's constants only, so the per-upload fields are simply unset
    Problem problem() const { return problem(UploadJob{mx.nnz}); }
    // run pointers of an axis' (major, minor)-sorted order, on the host
    const std::vector<int64_t> &major_ptr(int s) const { return mx.facts(s).mptr; }
    // (major, minor)-sorted position -> position in the caller's COO, on the device
    const int *order_of(int s, DevBuf &scratch);

private:   // the stages of an upload, in upload.hip
    void build_plan(PlanDev &pd, int64_t nnz, const int32_t *major, const int32_t *minor, const float *val, int n_major,
                    int n_minor, int windows, int chunk_len);
    void loss_tasks(TileDev &td, const UploadJob &job);
    void finish_tile(TileDev &td, const UploadJob &job);
    void plan_shapes(UploadJob &job, const SampleHistograms &sample) const;
    SampleHistograms host_samples(const UploadJob &job, const int32_t *row, const int32_t *col) const;
    void tiles_from_device_coo(const UploadJob &job, const int32_t *d_row, const int32_t *d_col, const float *d_val);
    void tiles_from_host_coo(const UploadJob &job, const int32_t *row, const int32_t *col, const float *val);
    void plans_from_host_coo(UploadJob &job, const int32_t *row, const int32_t *col, const float *val);
    void build_dual_order();
    double loss_constants(const float *d_values);
    double finish_upload(const UploadJob &job, const int32_t *d_col, const float *d_val);
    void holds_matrix(int64_t n_out, bool loss_constants);
};

}  // namespace schpf
