// The upload pipeline (engine.h Uploader): from a caller's matrix -- a COO on the host, a COO or CSR in device memory, rows
// of another engine's row-sorted copy -- to the record an engine holds of it: validated values, both plans, the loss
// constants.  Nothing here depends on the model dtype beyond the size of a value.
#include <algorithm>
#include <thread>

#include "engine.h"
#include "kernels.h"
#include "upload_device.h"

namespace schpf {

namespace {

constexpr int GAMMALN_BLOCKS = 512;

// An upload that does not get as far as holds_matrix leaves a fresh record, not half of a new one.  No graph exists
// then: forget_matrix dropped them and nothing can capture one without a matrix
struct FreshUnlessHeld {
    Matrix &mx;
    ~FreshUnlessHeld() { if (!mx.have_coo) mx = Matrix(); }
};

// The COO's index arrays start their trip over PCIe on a helper thread and a copy stream of its own
// while the calling thread is still validating / converting the values and sampling the block loads:
// the copy does not care whether the indices are in range, only the plan kernels do (and they run after
// the validation has passed).
struct EarlyIndexCopy {
    DevBuf d_row, d_col;
    std::thread worker;
    std::string error;
    double seconds = 0.0;
    void start(int device, int64_t n, const int32_t *row, const int32_t *col)
    {
        d_row.alloc((size_t)n * 4); d_col.alloc((size_t)n * 4);
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

}  // namespace

// In this order: no graph outlives the pointers it bakes in, and nothing is in flight on what the old record frees
void Uploader::forget_matrix()
{
    drop_graphs();
    HIPCHK(hipStreamSynchronize(stream));
    mx = Matrix();
    pending_init = 0;
    eager_since_upload = false;
}

const int *Uploader::order_of(int s, DevBuf &scratch)
{
    const PlanFacts &pl = mx.facts(s);
    if (pl.order_dev.p) return pl.order_dev.as<int>();
    if (pl.order_identity) {
        std::vector<int32_t> iota((size_t)mx.nnz);
        for (int64_t j = 0; j < mx.nnz; ++j) iota[(size_t)j] = (int32_t)j;
        upload(scratch, iota, stream);
        HIPCHK(hipStreamSynchronize(stream));   // iota dies with this scope
        return scratch.as<int>();
    }
    upload(scratch, pl.order, stream);
    return scratch.as<int>();
}

void Uploader::build_plan(PlanDev &pd, int64_t nnz_, const int32_t *major, const int32_t *minor, const float *val,
                          int n_major, int n_minor, int windows, int chunk_len)
{
    build_sweep_plan(nnz_, major, minor, val, n_major, n_minor, LPC, chunk_len, windows, true, pd.host);
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
    pd.part.rows.alloc((size_t)std::max<int64_t>(h.n_chunks, 1) * KP * elem, true, stream);
    HIPCHK(hipStreamSynchronize(stream));
    pd.mptr = std::move(h.mptr); pd.order = std::move(h.order);
    BigVec<uint32_t>().swap(h.entries);
    std::vector<int32_t>().swap(h.chunk_major);
    std::vector<int32_t>().swap(h.chunk_natid);
    std::vector<int32_t>().swap(h.wave_slice);
    std::vector<int64_t>().swap(h.slice_off);
    std::vector<int32_t>().swap(h.slice_steps);
}

// Tasks of the loss pass: the sub-ranges of the iteration's tasks that policy.cpp loss_cut chose, longest first
void Uploader::loss_tasks(TileDev &td, const UploadJob &job)
{
    auto &h = td.host;
    td.llh = TaskList();
    const LossCut cut = loss_cut(problem(job), tuning, h);
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
        loss_cut_points(h, t, cut.parts, cuts);
        std::vector<int64_t> off((size_t)wpb);
        for (int v = 0; v < wpb; ++v) off[(size_t)v] = h.task_wave_off[(size_t)t * wpb + v];
        for (size_t p = 0; p + 1 < cuts.size(); ++p) {
            blk.push_back(b); w0s.push_back(cuts[p]); w1s.push_back(cuts[p + 1]); ends.push_back(a1);
            for (int v = 0; v < wpb; ++v) woff.push_back(off[(size_t)v]);
            double wk = 0.0;
            for (int w = cuts[p]; w < cuts[p + 1]; ++w) {
                for (int v = 0; v < wpb; ++v)
                    off[(size_t)v] += tile_stored_steps(h, h.steps[((size_t)b * wpb + v) * W + w]) * h.gpw;
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
void Uploader::finish_tile(TileDev &td, const UploadJob &job)
{
    auto &h = td.host;
    const int wpb = h.wpb;
    td.threads = 64 * wpb;
    td.lds_bytes = h.ring > 1 ? (size_t)h.ring * h.slot16 * 16 : (size_t)h.win_rows * KP * elem;
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
    td.part.rows.alloc((size_t)std::max<int64_t>(h.n_partial_rows, 1) * KP * elem, true, stream);
    HIPCHK(hipStreamSynchronize(stream));
    td.mptr = std::move(h.mptr); td.order = std::move(h.order);
    std::vector<uint16_t>().swap(h.steps);
    std::vector<int64_t>().swap(h.task_wave_off);
}

// The shapes of both tile plans, once per upload, for whichever builder runs.  sample: the histograms of the COO's
// sampled indices for the task-range model, from wherever the COO lies (policy.h); empty: no ranges (batch rows)
void Uploader::plan_shapes(UploadJob &job, const SampleHistograms &sample) const
{
    if (!sample || !choose_ranges(problem(job), tuning, sample, job.ranges, job.half)) {
        job.ranges[0] = job.ranges[1] = 0;
        job.half[0] = job.half[1] = -1;
    }
    for (int s = 0; s < 2; ++s) {
        const TileShape &sh = job.shape[s] =
            tile_shape(problem(job), tuning, rows_of(s), rows_of(1 - s), job.ranges[s], job.half[s]);
        job.balanced[s] = job.balance && sh.ring <= 1 && sh.waves_per_block >= 12;   // the balanced kernels are 1024-thread ones
    }
}

// Both tile plans built by device passes over a COO that is in HBM (plan_device.hip): same plans, bit for bit, as
// tiles_from_host_coo(); SCHPF_DEVICE_PLAN=0 selects the host builder for schpf_upload_coo.
void Uploader::tiles_from_device_coo(const UploadJob &job, const int32_t *d_row, const int32_t *d_col, const float *d_val)
{
    // per side: its index array is the major one, the other side's the minor one
    const int32_t *const d_idx[2] = {d_row, d_col};
    const int64_t nz = job.nnz;
    auto build_side = [&](int si, hipStream_t st) {
        TileDev &td = mx.axis[si].tile;
        void *e = nullptr, *s = nullptr, *o = nullptr;
        size_t eb = 0;
        bool presorted = job.sorted[si];
        const int32_t *d_major = d_idx[si], *d_minor = d_idx[1 - si];
        const TileShape &sh = job.shape[si];
        const int n_major = rows_of(si);
        int n_minor_plan = rows_of(1 - si);
        DevBuf vminor;
        td.minor_of.release(); td.n_virtual = 0;
        if (job.balanced[si]) {
            const double tb = now_s();
            BalanceGeometry geo;
            void *mo = nullptr;
            // the balancing needs ~20 bytes per nonzero of scratch and 4 bytes per (block, minor row) for good: a matrix
            // that leaves no room for that is planned by index instead (the shape is valid for either)
            bool balanced = true;
            try {
                vminor.alloc((size_t)nz * 4);
                balance_windows_device((void *)st, nz, d_major, d_minor, n_major, n_minor_plan, sh, vminor.as<int32_t>(),
                                       &mo, geo);
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
        build_tile_plan_device((void *)st, nz, d_major, d_minor, d_val, presorted, job.packed_ok, n_major, n_minor_plan, sh,
                               td.host, &e, &eb, &s, &o);
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
    for (Matrix::Axis &ax : mx.axis) finish_tile(ax.tile, job);
    build_dual_order();
}

// Both tile plans from the host builder (plan.cpp): the two orientations concurrently (each with its own thread
// team), then uploaded one after the other on the context's stream
void Uploader::tiles_from_host_coo(const UploadJob &job, const int32_t *row, const int32_t *col, const float *val)
{
    const int32_t *const idx[2] = {row, col};   // per side: its index array is the major one, the other's the minor one
    double secs[2] = {0.0, 0.0};
    // balanced windows: the builder runs on the block's virtual numbering of the minor rows (plan.h)
    std::vector<int32_t> mo[2];
    on_both_sides(device, stream, false, [&](int s, hipStream_t) {
        const double t0 = now_s();
        const int32_t *major = idx[s], *minor = idx[1 - s];
        const int n_major = rows_of(s), n_minor = rows_of(1 - s);
        const TileShape &sh = job.shape[s];
        TileDev &td = mx.axis[s].tile;
        td.n_virtual = 0;
        if (job.balanced[s]) {
            BigVec<int32_t> vminor;
            BalanceGeometry geo;
            balance_windows_host(job.nnz, major, minor, n_major, n_minor, sh, vminor, mo[s], geo);
            td.n_virtual = geo.n_virtual;
            build_tile_plan(job.nnz, major, vminor.data(), val, n_major, geo.n_virtual, sh, true, td.host);
        } else {
            build_tile_plan(job.nnz, major, minor, val, n_major, n_minor, sh, true, td.host);
        }
        secs[s] = now_s() - t0;
    });
    for (int s = 0; s < 2; ++s) {   // device half: upload the host-built arrays, allocate the partials
        TileDev &td = mx.axis[s].tile;
        const double t1 = now_s();
        auto &h = td.host;
        td.entry_slots = (int64_t)h.entries.size() / (h.packed ? 1 : 2);
        upload(td.entries, h.entries, stream);
        upload(td.steps, h.steps, stream);
        finish_tile(td, job);
        if (tuning.verbose)
            fprintf(stderr, "[schpf_hip]   tile plan %d x %d: host build %.3f s, H2D %.3f s (%.2f GB entries)\n",
                    h.n_major, h.n_minor, secs[s], now_s() - t1, h.entries.size() * 4e-9);
        BigVec<uint32_t>().swap(h.entries);
    }
    for (int s = 0; s < 2; ++s) {
        TileDev &td = mx.axis[s].tile;
        td.minor_of.release();
        mo[s].resize(mo[s].size() + 16, -1);   // a list is copied in 16-byte pieces: slack behind the last one
        if (td.n_virtual) upload(td.minor_of, mo[s], stream);
    }
    HIPCHK(hipStreamSynchronize(stream));
    build_dual_order();
}

void Uploader::build_dual_order()
{
    // Both sweeps of an iteration in one launch (kernels.h launch_tile_sweep_dual) when the two
    // plans agree on the workgroup shape: slots = all tasks of both plans, longest first.  Not symmetric: the kernel
    // takes (cell args, gene args) in that order and a slot names a cell task as `task`, a gene task as `~task`
    mx.dual_slots = 0;
    mx.dual_order.release();
    const TileDev &tc = mx.axis[0].tile, &tg = mx.axis[1].tile;
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
        mx.dual_slots = (int64_t)ord.size();
        if (mx.dual_slots > 0) { upload(mx.dual_order, ord, stream); HIPCHK(hipStreamSynchronize(stream)); }
    }
}

// The upload's constants, from the values on the device: sum lgamma(x + 1), the constant term of the loss
// (hpf_numba.py:49-50), behind its block partials; and the ELBO shift terms (elbo_terms), the stored counts of every cell and
// every gene, summed over each plan's (major, minor)-sorted runs -- once per upload, N + G doubles.
// Returns the wall time of the count sums.
double Uploader::loss_constants(const float *d_values)
{
    mx.gammaln_part.alloc((GAMMALN_BLOCKS + 1) * sizeof(double));
    double *part = mx.gammaln_part.as<double>();
    HIPCHK(launch_gammaln_sum(d_values, mx.nnz, part, GAMMALN_BLOCKS, stream));
    HIPCHK(launch_sum_doubles(part, GAMMALN_BLOCKS, part + GAMMALN_BLOCKS, stream));
    const double t0 = now_s();
    for (int s = 0; s < 2; ++s) {
        DevBuf &count = mx.axis[s].count, scratch, mp;
        const int *ord = nullptr;
        if (!mx.facts(s).order_identity) ord = order_of(s, scratch);
        upload(mp, major_ptr(s), stream);
        count.alloc((size_t)rows_of(s) * sizeof(double));
        HIPCHK(launch_count_sums(d_values, ord, mp.as<int64_t>(), rows_of(s), count.as<double>(), stream));
        HIPCHK(hipStreamSynchronize(stream));   // scratch and mp die with this scope
    }
    return now_s() - t0;
}

// The engine now holds the matrix whose plans were just built: the record is complete.  n_out: doubles a loss pass
// leaves in wave_out.  loss_constants: false for gathered batch rows, whose loss is the source engine's business (no
// lgamma sum, no stored-zero list).  Graphs, pending_init and eager_since_upload are as forget_matrix left them: an
// upload runs no iteration
void Uploader::holds_matrix(int64_t n_out, bool loss_constants)
{
    mx.wave_out.alloc((size_t)std::max<int64_t>(n_out, 1) * sizeof(double), true, stream);
    HIPCHK(hipStreamSynchronize(stream));
    mx.have_loss_constants = loss_constants;
    mx.have_coo = true;
}

// This engine's matrix := the rows `rows` (in that order) of `source`'s, gathered on the device
void Uploader::upload_rows(schpf_ctx *source_, const int32_t *rows, int n_rows)
{
    Uploader *src = static_cast<Uploader *>(source_);   // every context is an engine (schpf_create)
    if (src->dtype != dtype) throw std::invalid_argument("the source engine must have this engine's dtype");
    if (!src->mx.rows_ptr.p || !src->mx.have_coo) throw std::logic_error("the source keeps no rows (schpf_keep_rows before its upload)");
    if (src == this) throw std::invalid_argument("an engine cannot gather batch rows from itself");
    if (src->device != device) throw std::invalid_argument("source and batch engine must be on one device");
    if (src->G != G || src->K != K) throw std::invalid_argument("source and batch engine differ in genes or factors");
    if (n_rows != N) throw std::invalid_argument("n_rows must be the number of cells the batch engine was created with");
    if (!want_tile) throw std::invalid_argument("upload_rows needs the tile plan");
    const std::vector<int64_t> &sp = src->mx.axis[0].tile.mptr;   // host copy of its rows_ptr
    std::vector<int64_t> dp((size_t)n_rows + 1, 0);
    for (int i = 0; i < n_rows; ++i) {
        if (rows[i] < 0 || rows[i] >= src->N) throw std::invalid_argument("batch row out of range");
        dp[(size_t)i + 1] = dp[(size_t)i] + (sp[(size_t)rows[i] + 1] - sp[(size_t)rows[i]]);
    }
    forget_matrix();
    FreshUnlessHeld guard{mx};
    // a batch is planned every iteration, the cheapest way: no balanced windows, no task ranges, no loss tasks.
    // Its rows come in batch order with their columns ascending: sorted by (row, col) already
    UploadJob job;
    job.nnz = dp[(size_t)n_rows];
    job.batch_rows = true;
    job.packed_ok = src->mx.rows_packed_ok;
    job.sorted[1] = false;
    mx.nnz = job.nnz;
    std::vector<int32_t> rv(rows, rows + n_rows);
    DevBuf d_rows, d_dp, d_row, d_col, d_val;
    upload(d_rows, rv, stream);
    upload(d_dp, dp, stream);
    d_row.alloc((size_t)mx.nnz * 4); d_col.alloc((size_t)mx.nnz * 4); d_val.alloc((size_t)mx.nnz * 4);
    HIPCHK(launch_gather_rows(d_rows.as<int>(), n_rows, src->mx.rows_ptr.as<int64_t>(), src->mx.rows_col.as<int>(),
                              src->mx.rows_val.as<float>(), d_dp.as<int64_t>(), d_row.as<int>(), d_col.as<int>(),
                              d_val.as<float>(), stream));
    mx.use_tile = true;
    plan_shapes(job, nullptr);
    tiles_from_device_coo(job, d_row.as<int32_t>(), d_col.as<int32_t>(), d_val.as<float>());
    holds_matrix(mx.axis[0].tile.n_wave_out, false);
}

void Uploader::upload_coo(int64_t nnz_, const int32_t *row, const int32_t *col, const void *val, int kind)
{
    const double t_start = now_s();
    if (nnz_ < 0 || nnz_ >= (int64_t)1 << 31) throw std::invalid_argument("nnz must be < 2^31");
    if (kind < SCHPF_VAL_I32 || kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
    // whatever the engine held is discarded on every path below: let go of it BEFORE anything new is allocated
    // (a re-upload onto a live engine would otherwise peak at the old plans + the new indices), and an upload
    // that fails leaves an engine without a matrix, not one with half of the old one
    forget_matrix();
    FreshUnlessHeld guard{mx};
    // balanced windows (plan.h): for uploads of a whole matrix; not for an engine that keeps a (row, col)-sorted copy
    // (the plans' own order is then the virtual one) nor for one whose matrix is replaced every iteration
    UploadJob job;
    job.nnz = nnz_;
    job.balance = want_tile && balance_windows(problem(job), tuning);
    EarlyIndexCopy early;
    const bool device_plans = want_tile && tuning.device_plan;
    if (device_plans) early.start(device, nnz_, row, col);
    BigVec<float> v((size_t)nnz_);   // no serial zero-fill: written by the threaded pass below
    std::vector<int32_t> zrow, zcol;         // explicitly stored zeros (rare): see zero_rate_sum()
    {   // validate + convert, in parallel slabs (first offending entry per slab is reported)
        const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), nnz_ / 65536 + 1));
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
            mx.n_rounded += rounded[(size_t)t];
            zrow.insert(zrow.end(), zr[(size_t)t].begin(), zr[(size_t)t].end());
            zcol.insert(zcol.end(), zc[(size_t)t].begin(), zc[(size_t)t].end());
        }
    }
    mx.n_zero = (int64_t)zrow.size();
    upload(mx.zero_row, zrow, stream);
    upload(mx.zero_col, zcol, stream);
    const double t_valid = now_s();
    mx.nnz = nnz_;
    mx.use_tile = want_tile;
    DevBuf d_val;   // the values on the device: beside the indices for the device builder, afterwards for the others
    if (device_plans) {
        plan_shapes(job, host_samples(job, row, col));
        coo_order_flags(mx.nnz, row, col, job.sorted[0], job.sorted[1]);
        d_val.alloc((size_t)mx.nnz * 4);
        if (mx.nnz > 0) HIPCHK(hipMemcpyAsync(d_val.p, v.data(), (size_t)mx.nnz * 4, hipMemcpyHostToDevice, stream));
        early.join();                                  // the indices went up beside the validation pass
        if (!early.error.empty()) throw HipError(early.error);
        const double t1 = now_s();
        tiles_from_device_coo(job, early.d_row.as<int32_t>(), early.d_col.as<int32_t>(), d_val.as<float>());
        if (tuning.verbose)
            fprintf(stderr, "[schpf_hip]   tile plans on the device: ranges + H2D of the values %.3f s (indices: %.3f s on the "
                    "helper thread, from the start of the upload), both plans %.3f s (%.2f GB entries)\n",
                    t1 - t_valid, early.seconds, now_s() - t1, (mx.axis[0].tile.entries.bytes + mx.axis[1].tile.entries.bytes) * 1e-9);
    } else plans_from_host_coo(job, row, col, v.data());
    const double t_plans = now_s();
    // the device builder's values are still resident: no second trip over PCIe.  Host-built plans: they go up now
    if (!device_plans) upload(d_val, v, stream);
    const double count_seconds = finish_upload(job, device_plans ? early.d_col.as<int32_t>() : nullptr, d_val.as<float>());
    d_val.release();
    if (tuning.verbose)
        fprintf(stderr, "[schpf_hip] upload_coo nnz=%lld: validate %.3f s, plans+H2D %.3f s, gammaln %.3f s (%d host threads); "
                "ELBO count sums %.4f s of it\n",
                (long long)mx.nnz, t_valid - t_start, t_plans - t_valid, now_s() - t_plans, host_threads(),
                count_seconds);
}

// the task-range model's samples from a COO on the host
SampleHistograms Uploader::host_samples(const UploadJob &job, const int32_t *row, const int32_t *col) const
{
    return [this, &job, row, col](int64_t stride, std::vector<int32_t> hist[2]) {
        hist[0] = sample_histogram(job.nnz, row, N, stride);
        hist[1] = sample_histogram(job.nnz, col, G, stride);
    };
}

// Both plans from the host builders over a COO on the host: tile plans (SCHPF_DEVICE_PLAN=0) or gather plans
void Uploader::plans_from_host_coo(UploadJob &job, const int32_t *row, const int32_t *col, const float *val)
{
    if (mx.use_tile) {
        plan_shapes(job, host_samples(job, row, col));
        tiles_from_host_coo(job, row, col, val);
        return;
    }
    const int32_t *const idx[2] = {row, col};
    const int chunk = gather_chunk_len(problem(job));
    for (int s = 0; s < 2; ++s)   // windows: by the size of the minor side's table
        build_plan(mx.axis[s].plan, job.nnz, idx[s], idx[1 - s], val, rows_of(s), rows_of(1 - s),
                   pick_windows((size_t)rows_of(1 - s) * KP * elem), chunk);
    mx.axis[0].plan.n_wave_out = mx.axis[0].plan.launch;   // one double per wavefront; the cell plan only (PlanFacts)
}

// What every whole-matrix upload does once its plans stand: the loss constants from the values on the device, the
// (row, col)-sorted copy minibatches gather their rows from (d_col: the column indices on the device in the
// caller's order, or nullptr where the plans were built on the host), and the engine holds the matrix.  Returns
// the wall time of the count sums
double Uploader::finish_upload(const UploadJob &job, const int32_t *d_col, const float *d_val)
{
    const double count_seconds = loss_constants(d_val);
    if (d_col && want_rows) {
        mx.rows_col.alloc((size_t)mx.nnz * 4); mx.rows_val.alloc((size_t)mx.nnz * 4);
        const TileDev &tc = mx.axis[0].tile;   // the cell plan's order; rows_ptr's host copy stays tc.mptr
        HIPCHK(launch_gather_by_order(tc.order_identity ? nullptr : tc.order_dev.as<int>(), d_col, d_val, mx.nnz,
                                      mx.rows_col.as<int>(), mx.rows_val.as<float>(), stream));
        upload(mx.rows_ptr, tc.mptr, stream);
        mx.rows_packed_ok = job.packed_ok;
        HIPCHK(hipStreamSynchronize(stream));
    }
    HIPCHK(hipMemcpyAsync(&mx.gammaln_sum, mx.gammaln_part.as<double>() + GAMMALN_BLOCKS, sizeof(double),
                          hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    holds_matrix(std::max(mx.facts(0).n_wave_out, mx.facts(1).n_wave_out), true);   // the loss pass sweeps either plan
    return count_seconds;
}

// The matrix is in HBM already (schpf_upload_coo_device / schpf_upload_csr_device): the stages
// upload_coo runs on host threads -- validate + convert, the stored-zero list, the order flags, the task-range
// samples -- as device passes (upload_device.h), arriving at tiles_from_device_coo with the job a host upload of the
// same entries in the same order makes.  Nothing of O(nnz) crosses PCIe.  Host-built plans (SCHPF_PLAN=gather,
// SCHPF_DEVICE_PLAN=0) are the cross-check: the converted triples are staged to the host for those builders.
// Errors: the smallest offending entry; an index error goes before a value error.
void Uploader::upload_device(int64_t nnz_, const void *rows, int indptr_kind, const void *col, int idx_kind,
                             const void *val, int val_kind)
{
    const double t_start = now_s();
    const bool csr = indptr_kind >= 0;
    if (nnz_ < 0 || nnz_ >= (int64_t)1 << 31) throw std::invalid_argument("nnz must be < 2^31");
    if (val_kind < SCHPF_VAL_I32 || val_kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
    for (int k : {idx_kind, csr ? indptr_kind : idx_kind})
        if (k != SCHPF_IDX_I32 && k != SCHPF_IDX_I64) throw std::invalid_argument("unknown index kind");
    forget_matrix();
    FreshUnlessHeld guard{mx};
    UploadJob job;
    job.nnz = nnz_;
    job.balance = want_tile && balance_windows(problem(job), tuning);
    // engine-owned int32 / float32 copies, only of what the caller did not hand over in that type already (an empty
    // matrix may come with NULL pointers: the builders then get the engine's own empty buffers)
    DevBuf own_row, own_col, own_val;
    if (csr) {
        if (!csr_indptr_valid(stream, rows, indptr_kind, N, nnz_))
            throw std::invalid_argument("CSR indptr must be non-decreasing from 0 to nnz");
        own_row.alloc((size_t)nnz_ * 4);
        csr_expand_rows(stream, rows, indptr_kind, N, nnz_, own_row.as<int32_t>());
    } else if (idx_kind != SCHPF_IDX_I32 || nnz_ == 0) own_row.alloc((size_t)nnz_ * 4);
    if (idx_kind != SCHPF_IDX_I32 || nnz_ == 0) own_col.alloc((size_t)nnz_ * 4);
    if (val_kind != SCHPF_VAL_F32 || nnz_ == 0) own_val.alloc((size_t)nnz_ * 4);
    const ConvertStats cs =
        convert_coo_device(stream, nnz_, csr ? own_row.p : rows, csr ? SCHPF_IDX_I32 : idx_kind, col, idx_kind, val,
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
    mx.n_rounded = cs.rounded; mx.n_zero = cs.zeros;
    mx.zero_row.alloc((size_t)mx.n_zero * 4); mx.zero_col.alloc((size_t)mx.n_zero * 4);
    compact_zeros_device(stream, nnz_, d_row, d_col, val, val_kind, mx.n_zero, mx.zero_row.as<int32_t>(), mx.zero_col.as<int32_t>());
    const double t_valid = now_s();
    mx.nnz = nnz_;
    mx.use_tile = want_tile;
    const bool device_plans = want_tile && tuning.device_plan;
    double t_shapes = t_valid;
    if (device_plans) {
        plan_shapes(job, [&](int64_t stride, std::vector<int32_t> hist[2]) {
            hist[0].resize((size_t)N); hist[1].resize((size_t)G);
            sample_histograms_device(stream, mx.nnz, d_row, d_col, N, G, stride, hist[0].data(), hist[1].data());
        });
        t_shapes = now_s();
        tiles_from_device_coo(job, d_row, d_col, d_val);
    } else {
        BigVec<int32_t> h_row((size_t)mx.nnz), h_col((size_t)mx.nnz);
        BigVec<float> h_val((size_t)mx.nnz);
        if (mx.nnz > 0) {
            HIPCHK(hipMemcpyAsync(h_row.data(), d_row, (size_t)mx.nnz * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(h_col.data(), d_col, (size_t)mx.nnz * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(h_val.data(), d_val, (size_t)mx.nnz * 4, hipMemcpyDeviceToHost, stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        plans_from_host_coo(job, h_row.data(), h_col.data(), h_val.data());
    }
    const double t_plans = now_s();
    const double count_seconds = finish_upload(job, device_plans ? d_col : nullptr, d_val);
    if (tuning.verbose)
        fprintf(stderr, "[schpf_hip] upload_%s_device nnz=%lld: %svalidate + convert + zeros %.3f s, order flags in it, task-range "
                "samples %.3f s, plans %.3f s%s, gammaln %.3f s; ELBO count sums %.4f s of it\n",
                csr ? "csr" : "coo", (long long)mx.nnz, csr ? "row expansion + " : "", t_valid - t_start, t_shapes - t_valid,
                t_plans - t_shapes, device_plans ? "" : " (staged to the host builders)", now_s() - t_plans, count_seconds);
}

}  // namespace schpf
