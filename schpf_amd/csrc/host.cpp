// Host-only entry points of the C ABI (include/schpf_hip.h): the marginals of a COO, the two plan expanders the tests
// check the host builders with, the serial restatements of count thinning (thin.hip), of the nearest-neighbour search
// (knn.hip), of the neighbour graphs (knn_graph.hip), of the Louvain clustering (louvain.hip), of the connected
// components and the cluster graph (components.hip), of the shortest-path distances (geodesic.hip), of the rank sums
// (rank_sums.hip), of the simulated doublets (doublets.hip) with the draw of their parents and of the axis statistics and
// the submatrix (qc.hip), of the Pearson residual sums per gene (residual_var.hip), of the transpose to gene-major
// (transpose.hip), and the SCHPF_BACKTRACE crash handler.  The restatements that read a caller's CSR validate it with
// check_count_csr or check_graph_csr and check_labels, below, and then do their arithmetic.
// Nothing here touches the device.
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <queue>
#include <thread>

#include "common.h"
#include "csr_words.h"
#include "doublets.h"
#include "group_stats.h"
#include "philox.h"
#include "policy.h"
#include "qc.h"
#include "residual_var.h"
#include "special.h"
#include "transpose.h"

using namespace schpf;

// SCHPF_BACKTRACE=1 (debugging aid, read when the library is loaded): a SIGSEGV / SIGBUS / SIGABRT prints the native call
// stack (glibc backtrace: module + offset per frame, resolvable with addr2line against this .so) before the previous
// handler -- Python's faulthandler under pytest -- runs.  The GPU boxes have no debugger.
namespace {
struct sigaction g_prev_segv, g_prev_bus, g_prev_abrt;
void crash_trace(int sig, siginfo_t *info, void *uctx)
{
    void *frames[64];
    const int n = backtrace(frames, 64);
    const char msg[] = "[schpf_hip] fatal signal, native stack:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    struct sigaction *prev = sig == SIGSEGV ? &g_prev_segv : sig == SIGBUS ? &g_prev_bus : &g_prev_abrt;
    sigaction(sig, prev, nullptr);          // hand over: the previous handler (or the default action) sees the re-raised signal
    raise(sig);
    (void)info; (void)uctx;
}
struct CrashTraceInstaller {
    CrashTraceInstaller()
    {
        const char *e = getenv("SCHPF_BACKTRACE");
        if (!e || !*e || *e == '0') return;
        void *frame[1];
        (void)backtrace(frame, 1);   // the first call loads libgcc and allocates: here, not inside a signal handler
        struct sigaction sa;
        std::memset(&sa, 0, sizeof sa);
        sa.sa_sigaction = crash_trace;
        sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
        sigaction(SIGSEGV, &sa, &g_prev_segv);
        sigaction(SIGBUS, &sa, &g_prev_bus);
        sigaction(SIGABRT, &sa, &g_prev_abrt);
    }
} g_crash_trace_installer;
}  // namespace

// The validation every restatement of a CSR consumer shares, one routine per family: the rule the kernels of
// csr_device.h and graph_device.h check, as serial loops that throw the refusal of the smallest offender
namespace {

// A count CSR (int64 indptr, int32 columns) to `level` under the prefix of operator `op`.  The indptr first: the walk over
// the entries relies on it, as the device fetches its verdict before the entry check is launched.  Then one pass finds the
// smallest offending entry, row and entry of the column range, the column order and the values, refused in that order.
// Returns the largest value (0 below CSR_COUNTS)
uint64_t check_count_csr(const char *op, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                         const void *val, int val_kind, CsrLevel level)
{
    for (int64_t r = 0; r <= ncells; ++r)
        if ((r == 0 && indptr[0] != 0) || (r == ncells ? indptr[r] != nnz : indptr[r + 1] < indptr[r]))
            throw std::invalid_argument(csr_bad_indptr(op, r));
    int64_t bad_index = -1, bad_order = -1, bad_value = -1;
    uint64_t vmax = 0;
    for (int64_t r = 0; r < ncells; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if ((indices[e] < 0 || indices[e] >= ngenes) && bad_index < 0) bad_index = e;
            if (level >= CSR_ORDER && e > indptr[r] && indices[e - 1] >= indices[e] && bad_order < 0) bad_order = r;
            if (level < CSR_COUNTS) continue;
            const double v = read_count(val, val_kind, e);
            if (schpf::thin_value_bad(v)) {
                if (bad_value < 0) bad_value = e;
            } else {
                vmax = std::max(vmax, (uint64_t)v);
            }
        }
    if (bad_index >= 0) throw std::invalid_argument(csr_bad_index(op, bad_index));
    if (bad_order >= 0) throw std::invalid_argument(csr_bad_order(op, bad_order));
    if (bad_value >= 0) throw std::invalid_argument(csr_bad_value(op, bad_value));
    return vmax;
}

// How an operator of the graph and gene-major family words the refusals of its matrix, and whether it asks for ascending
// columns (the wording of `columns` says so)
struct GraphWords {
    std::string (*indptr)(int64_t), (*columns)(int64_t), (*values)(int64_t);
    bool ascending;
};
const GraphWords LOUVAIN_WORDS{louvain_bad_indptr, louvain_bad_columns, louvain_bad_values, true};
const GraphWords GRAPH_WORDS{louvain_bad_indptr, graph_bad_columns, louvain_bad_values, false};
const GraphWords RANK_SUMS_WORDS{rank_sums_bad_indptr, rank_sums_bad_cells, rank_sums_bad_values, true};
const GraphWords HVG_WORDS{hvg_bad_indptr, hvg_bad_cells, hvg_bad_values, true};

// A CSR of n rows with int64 indptr, int32 columns in [0, bound) and values that are finite and >= 0 (data == nullptr: none
// are asked).  In this order: indptr starts at 0 and does not decrease; refuse_nnz(indptr[n]), the operator's own refusal
// of the entries' number and pointers; the columns; the values.  Each names its smallest offending row.  Returns indptr[n]
template <typename V, typename RefuseNnz>
int64_t check_graph_csr(const GraphWords &words, int64_t n, int64_t bound, const int64_t *indptr, const int32_t *indices, const V *data,
                        RefuseNnz &&refuse_nnz)
{
    if (n == 0) return 0;
    if (indptr[0] != 0) throw std::invalid_argument(words.indptr(0));
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) throw std::invalid_argument(words.indptr(i));
    refuse_nnz(indptr[n]);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e)
            if (indices[e] < 0 || indices[e] >= bound || (words.ascending && e > indptr[i] && indices[e - 1] >= indices[e]))
                throw std::invalid_argument(words.columns(i));
    for (int64_t i = 0; data && i < n; ++i)
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e)
            if (!(data[e] >= V(0) && std::isfinite(data[e]))) throw std::invalid_argument(words.values(i));
    return indptr[n];
}
void refuse_if(const char *why)
{
    if (why) throw std::invalid_argument(why);
}

// every label in [-1, ngroups): the smallest offender in the operator's words
void check_labels(int64_t n, const int32_t *labels, int64_t ngroups, std::string (*words)(int64_t))
{
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] < -1 || labels[i] >= ngroups) throw std::invalid_argument(words(i));
}

}  // namespace

extern "C" {

int schpf_coo_marginals(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int kind,
                        int ncells, int ngenes, double *row_sums, double *col_sums)
{
    return guarded([&] {
        if (nnz < 0 || ncells < 0 || ngenes < 0) throw std::invalid_argument("negative size");
        if (kind < SCHPF_VAL_I32 || kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
        // per-thread partial sums over contiguous slabs, added up in thread order: exact for counts
        // (integers far below 2^53) and run-to-run deterministic for anything else
        const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(schpf::host_threads(), 16), nnz / 65536 + 1));
        std::vector<std::vector<double>> pr((size_t)nth), pc((size_t)nth);
        std::vector<int64_t> bad((size_t)nth, -1);
        std::vector<std::thread> th;
        for (int t = 0; t < nth; ++t)
            th.emplace_back([&, t] {
                pr[(size_t)t].assign((size_t)ncells, 0.0);
                pc[(size_t)t].assign((size_t)ngenes, 0.0);
                double *r = pr[(size_t)t].data(), *g = pc[(size_t)t].data();
                const int64_t b = nnz * t / nth, e = nnz * (t + 1) / nth;
                for (int64_t i = b; i < e; ++i) {
                    if (row[i] < 0 || row[i] >= ncells || col[i] < 0 || col[i] >= ngenes) {
                        if (bad[(size_t)t] < 0) bad[(size_t)t] = i;
                        continue;
                    }
                    const double d = read_count(val, kind, i);
                    r[row[i]] += d;
                    g[col[i]] += d;
                }
            });
        for (auto &x : th) x.join();
        for (int t = 0; t < nth; ++t)
            if (bad[(size_t)t] >= 0)
                throw std::invalid_argument("COO index out of range at entry " + std::to_string(bad[(size_t)t]));
        for (int i = 0; i < ncells; ++i) { double s = 0.0; for (int t = 0; t < nth; ++t) s += pr[(size_t)t][(size_t)i]; row_sums[i] = s; }
        for (int i = 0; i < ngenes; ++i) { double s = 0.0; for (int t = 0; t < nth; ++t) s += pc[(size_t)t][(size_t)i]; col_sums[i] = s; }
    });
}

int schpf_debug_plan_expand(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val,
                            int n_major, int n_minor, int lpc, int chunk_len, int n_windows,
                            int32_t *out_major, int32_t *out_minor, float *out_val, int32_t *out_natid,
                            int32_t *out_wave, int32_t *out_cptr, int64_t stats[4])
{
    return guarded([&] {
        schpf::SweepPlanHost P;
        schpf::build_sweep_plan(nnz, major, minor, val, n_major, n_minor, lpc, chunk_len, n_windows, false, P);
        std::vector<int32_t> wave_of_slice((size_t)P.n_slices, -1);
        for (int64_t w = 0; w < P.n_waves; ++w)
            if (P.wave_slice[(size_t)w] >= 0) {
                if (wave_of_slice[(size_t)P.wave_slice[(size_t)w]] != -1)
                    throw std::logic_error("slice scheduled twice");
                wave_of_slice[(size_t)P.wave_slice[(size_t)w]] = (int32_t)w;
            }
        int64_t n = 0;
        for (int64_t s = 0; s < P.n_slices; ++s) {
            if (wave_of_slice[(size_t)s] < 0) throw std::logic_error("slice never scheduled");
            const uint32_t *base = P.entries.data() + (size_t)P.slice_off[(size_t)s] * 4;
            for (int step = 0; step < P.slice_steps[(size_t)s]; ++step)
                for (int slot = 0; slot < P.cpw; ++slot)
                    for (int u = 0; u < 2; ++u) {
                        const uint32_t *e = base + ((size_t)step * P.cpw + slot) * 4 + (size_t)u * 2;
                        float f;
                        std::memcpy(&f, &e[1], 4);
                        if (f == 0.0f) continue;
                        if (n >= nnz) throw std::logic_error("plan stores more nonzeros than given");
                        out_major[n] = P.chunk_major[(size_t)s * P.cpw + slot];
                        out_minor[n] = (int32_t)e[0];
                        out_val[n] = f;
                        out_natid[n] = P.chunk_natid[(size_t)s * P.cpw + slot];
                        out_wave[n] = wave_of_slice[(size_t)s];
                        ++n;
                    }
        }
        if (n != nnz) throw std::logic_error("plan lost nonzeros");
        for (int m = 0; m <= n_major; ++m) out_cptr[m] = P.cptr[(size_t)m];
        stats[0] = P.n_chunks; stats[1] = P.n_slices; stats[2] = P.n_waves;
        stats[3] = (int64_t)P.entries.size() / 2;
    });
}

int schpf_debug_tile_expand(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val,
                            int n_major, int n_minor, int lpc, int waves_per_block, int win_rows,
                            int target_tasks, int ring, int slot_bytes, int32_t *out_major, int32_t *out_minor,
                            float *out_val, int32_t *out_prow, int32_t *out_task, int32_t *out_pfirst,
                            int32_t *out_pcount, int64_t stats[8])
{
    return guarded([&] {
        const schpf::Tuning tn = schpf::tuning_from_env();   // per call: tests change the switches between calls
        schpf::TilePlanHost P;
        schpf::TileShape sh;
        sh.lpc = lpc; sh.waves_per_block = waves_per_block; sh.win_rows = win_rows; sh.target_tasks = target_tasks;
        sh.row_slots = tn.debug_row_slots;   // 160-byte table rows
        sh.ring = ring < 0 ? -ring : ring; sh.sync_stage = sh.ring > 1 ? 1 : 0; sh.slot_bytes = slot_bytes;
        // SCHPF_DEBUG_SINGLE=1: steps count nonzeros (plan.h; window schedule only)
        sh.single = tn.debug_single && sh.ring <= 1;
        sh.bank_order = tn.bank_order;
        sh.taper = tn.taper.value_or(0) / 100.0;
        sh.verbose = tn.verbose;
        if (sh.taper > 0.0) sh.slots = 1;   // tapered ranges are for orientations with more tasks than workgroups (plan.h)
        // SCHPF_DEBUG_BALANCE=1: balanced windows (plan.h) -- the plan is built on the blocks' virtual numbering of the
        // minor rows and every entry is mapped back through minor_of
        std::vector<int32_t> minor_of;
        schpf::BalanceGeometry geo;
        const bool balanced = tn.debug_balance && sh.ring <= 1;
        if (balanced) {
            schpf::BigVec<int32_t> vminor;
            schpf::balance_windows_host(nnz, major, minor, n_major, n_minor, sh, vminor, minor_of, geo);
            schpf::build_tile_plan(nnz, major, vminor.data(), val, n_major, geo.n_virtual, sh, false, P);
        } else
        schpf::build_tile_plan(nnz, major, minor, val, n_major, n_minor, sh, false, P);
        const int W = P.n_windows, gpw = P.gpw, wpb = P.wpb, gpb = P.gpb;
        // the LDS model of plan.cpp::bank_order: the lane groups of a pass read one row each per half step; rows of
        // one class (16-byte position mod 16, / lpc) are served one after the other
        const std::vector<int> pass_of = schpf::tile_pass_of(lpc, gpw);
        const int n_classes = std::max(1, 16 / std::max(1, lpc));
        int lpc_shift = 0;
        while ((1 << lpc_shift) < lpc) ++lpc_shift;
        int64_t lds_reads = 0, lds_extra = 0;
        int64_t n = 0;
        for (int64_t t = 0; t < P.n_tasks; ++t) {
            const int b = P.task_block[(size_t)t];
            for (int v = 0; v < wpb; ++v) {
                int64_t off = P.task_wave_off[(size_t)t * wpb + v];
                for (int w = P.task_w0[(size_t)t]; w < P.task_w1[(size_t)t]; ++w) {
                    const int steps = P.steps[((size_t)b * wpb + v) * W + w];
                    // the kernel's walk: `single` plans execute `steps` nonzeros (the slot halves 0 .. steps - 1)
                    const int n_half = P.single ? steps : 2 * steps;
                    for (int p = 0; 2 * p < n_half; ++p)
                        for (int u = 0; u < 2 && 2 * p + u < n_half; ++u) {
                          int in_class[4][16] = {};
                          for (int grp = 0; grp < gpw; ++grp) {
                                float f;
                                uint32_t off16;
                                if (P.packed) {
                                    const uint32_t *e = P.entries.data() + ((size_t)off + (size_t)p * gpw + grp) * 2;
                                    off16 = (e[0] >> (16 * u)) & 0xFFFFu;
                                    f = (float)((e[1] >> (16 * u)) & 0xFFFFu);
                                } else {
                                    const uint32_t *e = P.entries.data() + ((size_t)off + (size_t)p * gpw + grp) * 4 + (size_t)u * 2;
                                    off16 = e[0];
                                    std::memcpy(&f, &e[1], 4);
                                }
                                int mn;   // the kernel's reconstruction (sweep_impl.h entry_minor)
                                if (P.ring > 1) {
                                    const int slot = (int)(off16 / (uint32_t)P.slot16);
                                    const int r = (int)((off16 - (uint32_t)slot * P.slot16) / (uint32_t)P.row_slots);
                                    const int ahead = (slot - w % P.ring + P.ring) % P.ring;
                                    // readable in epoch w: sub-windows w .. w + look, inside the task
                                    if (slot >= P.ring || ahead > P.look || w + ahead >= P.task_w1[(size_t)t])
                                        throw std::logic_error("ring plan: an entry points outside the readable slots");
                                    if (f == 0.0f && off16 != (uint32_t)(w % P.ring) * (uint32_t)P.slot16)
                                        throw std::logic_error("ring plan: padding must point at the epoch's own slot");
                                    mn = (w + ahead) * P.win_rows + r;
                                } else {
                                    mn = w * P.win_rows + (int)(off16 / (uint32_t)P.row_slots);
                                }
                                if (f == 0.0f) continue;
                                in_class[pass_of[(size_t)grp]][((off16 & 15u) >> lpc_shift) & (unsigned)(n_classes - 1)]++;
                                if (schpf::tile_off16(P, mn) != off16) throw std::logic_error("tile plan: bad LDS position");
                                if (n >= nnz) throw std::logic_error("tile plan stores more nonzeros than given");
                                const int g = v * gpw + grp;
                                out_major[n] = P.block_rows[(size_t)b * gpb + g];
                                out_minor[n] = balanced ? minor_of[(size_t)b * geo.n_virtual + (size_t)mn] : (int32_t)mn;
                                out_val[n] = f;
                                out_prow[n] = (int32_t)(t * gpb + g);
                                out_task[n] = (int32_t)t;
                                ++n;
                          }
                          for (int ps = 0; ps < 4; ++ps) {
                              int worst = 0;
                              for (int c = 0; c < 16; ++c) worst = std::max(worst, in_class[ps][c]);
                              if (worst) { lds_reads++; lds_extra += worst - 1; }
                          }
                        }
                    off += schpf::tile_stored_steps(P, steps) * gpw;
                }
            }
        }
        if (n != nnz) throw std::logic_error("tile plan lost nonzeros");
        for (int m = 0; m < n_major; ++m) { out_pfirst[m] = P.pfirst[(size_t)m]; out_pcount[m] = P.pcount[(size_t)m]; }
        stats[0] = P.n_tasks; stats[1] = P.n_blocks; stats[2] = P.n_windows; stats[3] = P.pstride;
        stats[4] = (int64_t)P.entries.size() / (P.packed ? 1 : 2); stats[5] = P.windows_per_task;
        stats[6] = lds_reads; stats[7] = lds_extra;
    });
}

// Which half of its step slot every nonzero of a window-schedule tile plan lies in: the plan is built as in
// schpf_debug_tile_expand and walked as the kernel walks it.  The paired float64 sweep treats the two halves of a slot
// in different lanes (sweep_impl.h pair_own_sum), and its tests place nonzeros in one half or the other on purpose
int schpf_debug_tile_halves(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val, int n_major,
                            int n_minor, int lpc, int waves_per_block, int win_rows, int target_tasks,
                            int32_t *out_major, int32_t *out_minor, int32_t *out_half)
{
    if (!major || !minor || !val || !out_major || !out_minor || !out_half) return fail("NULL argument");
    return guarded([&] {
        const schpf::Tuning tn = schpf::tuning_from_env();
        schpf::TilePlanHost P;
        schpf::TileShape sh;
        sh.lpc = lpc; sh.waves_per_block = waves_per_block; sh.win_rows = win_rows; sh.target_tasks = target_tasks;
        sh.row_slots = tn.debug_row_slots;
        sh.bank_order = tn.bank_order;
        schpf::build_tile_plan(nnz, major, minor, val, n_major, n_minor, sh, false, P);
        const int W = P.n_windows, gpw = P.gpw, wpb = P.wpb, gpb = P.gpb;
        int64_t n = 0;
        for (int64_t t = 0; t < P.n_tasks; ++t) {
            const int b = P.task_block[(size_t)t];
            for (int v = 0; v < wpb; ++v) {
                int64_t off = P.task_wave_off[(size_t)t * wpb + v];
                for (int w = P.task_w0[(size_t)t]; w < P.task_w1[(size_t)t]; ++w) {
                    const int steps = P.steps[((size_t)b * wpb + v) * W + w];
                    for (int p = 0; p < steps; ++p)
                        for (int u = 0; u < 2; ++u)
                            for (int grp = 0; grp < gpw; ++grp) {
                                const size_t slot = (size_t)off + (size_t)p * gpw + grp;
                                uint32_t off16, bits;
                                if (P.packed) {
                                    const uint32_t *e = P.entries.data() + slot * 2;
                                    off16 = (e[0] >> (16 * u)) & 0xFFFFu;
                                    bits = (e[1] >> (16 * u)) & 0xFFFFu;
                                } else {
                                    const uint32_t *e = P.entries.data() + slot * 4 + (size_t)u * 2;
                                    off16 = e[0];
                                    bits = e[1] & 0x7FFFFFFFu;   // a float: zero is padding
                                }
                                if (bits == 0) continue;
                                if (n >= nnz) throw std::logic_error("tile plan stores more nonzeros than given");
                                out_major[n] = P.block_rows[(size_t)b * gpb + v * gpw + grp];
                                out_minor[n] = w * P.win_rows + (int)(off16 / (uint32_t)P.row_slots);
                                out_half[n] = u;
                                ++n;
                            }
                    off += schpf::tile_stored_steps(P, steps) * gpw;
                }
            }
        }
        if (n != nnz) throw std::logic_error("tile plan lost nonzeros");
    });
}

// the shape the engine would sweep `nfactors` factors with: choose_config itself, asked with a Tuning that sets the
// plan and nothing else (no environment is read)
int schpf_debug_choose_config(int dtype, int nfactors, int plan, int out[5])
{
    if (!out) return fail("out is NULL");
    if (bad_dtype(dtype)) return fail("dtype must be SCHPF_F32 or SCHPF_F64");
    if (plan < 0 || plan > 2) return fail("plan must be 0 (auto), 1 (tile) or 2 (gather)");
    return guarded([&] {
        schpf::Tuning tn;
        tn.plan = plan == 1 ? schpf::Tuning::PLAN_TILE : plan == 2 ? schpf::Tuning::PLAN_GATHER : schpf::Tuning::PLAN_AUTO;
        const schpf::Config c = schpf::choose_config(nfactors, dtype == SCHPF_F32 ? 4 : 8, tn);
        out[0] = c.tile ? 1 : 0; out[1] = c.LPC; out[2] = c.NV; out[3] = c.KL; out[4] = c.KP;
    });
}

int schpf_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    if (!counter || !key || !out) return fail("counter, key and out must not be NULL");
    const schpf::Philox4 b = schpf::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    for (int w = 0; w < 4; ++w) out[w] = b.w[w];
    return 0;
}

// the kernels of thin.hip restated as one serial loop over the entries: the same predicates, the same draw (philox.h)
int schpf_debug_thin_counts(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int val_kind,
                            double frac, uint64_t seed, int32_t *train, int32_t *test, int64_t stats[4])
{
    if (!stats) return fail("stats is NULL");
    if (nnz < 0 || nnz >= (1ll << 31)) return fail("nnz must be in [0, 2^31)");
    if (nnz > 0 && (!row || !col || !val || !train || !test)) return fail("row, col, val, train and test must not be NULL");
    return guarded([&] {
        if (val_kind < SCHPF_VAL_I32 || val_kind > SCHPF_VAL_F64) throw std::invalid_argument("unknown value kind");
        uint32_t T = 0;
        if (!schpf::thin_threshold(frac, &T)) throw std::invalid_argument("frac must be in (0, 1) and at least 2^-32");
        for (int k = 0; k < 4; ++k) stats[k] = 0;
        int64_t first_bad_index = -1, first_bad_value = -1;
        for (int64_t e = 0; e < nnz; ++e) {
            if (schpf::thin_index_bad(row[e]) || schpf::thin_index_bad(col[e])) {
                if (first_bad_index < 0) first_bad_index = e;
            } else if (schpf::thin_value_bad(read_count(val, val_kind, e))) {
                if (first_bad_value < 0) first_bad_value = e;
            }
        }
        // an index error before a value error, the rule of schpf_upload_coo_device; an invalid matrix is not drawn
        if (first_bad_index >= 0)
            throw std::invalid_argument("COO index out of range at entry " + std::to_string(first_bad_index));
        if (first_bad_value >= 0)
            throw std::invalid_argument("thinning needs integer counts in [0, 2^24]; offending entry " +
                                        std::to_string(first_bad_value));
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        for (int64_t e = 0; e < nnz; ++e) {
            const uint32_t x = (uint32_t)read_count(val, val_kind, e);
            const uint32_t hits = schpf::thin_draw((uint32_t)row[e], (uint32_t)col[e], x, k0, k1, T);
            train[e] = (int32_t)(x - hits);
            test[e] = (int32_t)hits;
            stats[0] += x > hits;
            stats[1] += hits > 0;
            stats[2] += x - hits;
            stats[3] += hits;
        }
    });
}

// knn.hip restated: per query row a plain loop over the pairs -- one subtraction and one std::fma per factor,
// in factor order -- and a partial sort on the key (d2, r).  The query rows, independent of each other, are dealt to the
// host threads
int schpf_debug_knn(int dtype, int n_query, int n_ref, int nfactors, const void *query, const void *ref, int k,
                    int64_t self_first, int32_t *idx, double *d2)
{
    if (const char *why = knn_bad_args(dtype, n_query, n_ref, nfactors, query, ref, k, self_first, idx, d2)) return fail("%s", why);
    if (n_query == 0) return 0;
    return guarded([&] {
        const size_t K = (size_t)nfactors;
        auto value = [&](const void *x, size_t i) { return dtype == SCHPF_F32 ? (double)((const float *)x)[i] : ((const double *)x)[i]; };
        auto refuse = [&](const void *x, int n, const char *side) {
            for (int r = 0; r < n; ++r)
                for (size_t f = 0; f < K; ++f)
                    if (!std::isfinite(value(x, (size_t)r * K + f)))
                        throw std::invalid_argument("scores must be finite; offending row " + std::to_string(r) + " of " + side);
        };
        refuse(query, n_query, "query");
        refuse(ref, n_ref, "ref");
        std::vector<double> rd((size_t)n_ref * K);
        for (size_t i = 0; i < rd.size(); ++i) rd[i] = value(ref, i);
        const int nth = std::max(1, std::min(std::min(schpf::host_threads(), 16), n_query));
        std::vector<std::thread> th;
        for (int t = 0; t < nth; ++t)
            th.emplace_back([&, t] {
                std::vector<std::pair<double, int32_t>> keys;
                std::vector<double> qd(K);
                for (int q = t; q < n_query; q += nth) {
                    for (size_t f = 0; f < K; ++f) qd[f] = value(query, (size_t)q * K + f);
                    keys.clear();
                    for (int r = 0; r < n_ref; ++r) {
                        if (self_first >= 0 && (int64_t)r == self_first + q) continue;   // by index, not by distance
                        double s = 0.0;
                        for (size_t f = 0; f < K; ++f) {
                            const double d = qd[f] - rd[(size_t)r * K + f];
                            s = std::fma(d, d, s);
                        }
                        keys.emplace_back(s, r);
                    }
                    std::partial_sort(keys.begin(), keys.begin() + k, keys.end());   // pairs compare as the key does
                    for (int j = 0; j < k; ++j) {
                        d2[(size_t)q * k + j] = keys[(size_t)j].first;
                        idx[(size_t)q * k + j] = keys[(size_t)j].second;
                    }
                }
            });
        for (auto &x : th) x.join();
    });
}

// knn_graph.hip restated: the definition of include/schpf_hip.h line by line, one row after the other, then
// one std::sort of the 2 n k (row, col, direction) records
int schpf_debug_knn_graph(int method, int n, int k, const int32_t *idx, const double *dist, int64_t *indptr,
                          int32_t *indices, double *data, double *rho, double *sigma)
{
    if (const char *why = graph_bad_args(method, n, k, idx, dist, indptr, indices, data)) return fail("%s", why);
    if (n == 0) return 0;
    return guarded([&] {
        const bool umap = method == SCHPF_GRAPH_UMAP;
        const size_t K = (size_t)k;
        std::vector<int32_t> sorted((size_t)n * K);
        for (int i = 0; i < n; ++i) {
            int32_t *s = sorted.data() + (size_t)i * K;
            std::copy(idx + (size_t)i * K, idx + (size_t)i * K + K, s);
            std::sort(s, s + K);
            bool wrong = s[0] < 0 || s[K - 1] >= n;
            for (size_t j = 0; j < K; ++j) wrong |= s[j] == i || (j > 0 && s[j] == s[j - 1]);
            if (wrong) throw std::invalid_argument(graph_bad_lists(i));
        }
        std::vector<double> w, rho_v, sigma_v;
        if (umap) {
            for (int i = 0; i < n; ++i)
                for (size_t j = 0; j < K; ++j)
                    if (!(dist[(size_t)i * K + j] >= 0.0 && std::isfinite(dist[(size_t)i * K + j])))
                        throw std::invalid_argument(graph_bad_distances(i));
            w.resize((size_t)n * K);
            rho_v.resize((size_t)n);
            sigma_v.resize((size_t)n);
            const double target = std::log2((double)(k + 1));
            auto W = [](double e, double s) {
                const double t = e / s;
                return t > 708.0 ? 0.0 : schpf::fast_exp(-t);
            };
            for (int i = 0; i < n; ++i) {
                const double *d = dist + (size_t)i * K;
                double r = HUGE_VAL, sum = 0.0;
                for (size_t j = 0; j < K; ++j) {
                    if (d[j] > 0.0 && d[j] < r) r = d[j];
                    sum += d[j];
                }
                if (r == HUGE_VAL) r = 0.0;
                double lo = 0.0, hi = HUGE_VAL, mid = 1.0;
                for (int round = 0; round < 64; ++round) {
                    double psum = 0.0;
                    for (size_t j = 0; j < K; ++j) {
                        const double e = d[j] - r;
                        psum += e > 0.0 ? W(e, mid) : 1.0;
                    }
                    if (std::fabs(psum - target) < 1e-5) break;
                    if (psum > target) {
                        hi = mid;
                        mid = (lo + hi) / 2.0;
                    } else {
                        lo = mid;
                        mid = hi == HUGE_VAL ? mid * 2.0 : (lo + hi) / 2.0;
                    }
                }
                double s = mid;
                if (r > 0.0) {
                    const double mean = sum / (double)k;
                    const double least = 1e-3 * mean;
                    if (s < least) s = least;
                }
                for (size_t j = 0; j < K; ++j) {
                    const double e = d[j] - r;
                    w[(size_t)i * K + j] = e <= 0.0 ? 1.0 : W(e, s);
                }
                rho_v[(size_t)i] = r;
                sigma_v[(size_t)i] = s;
            }
        }
        struct Rec { uint64_t key; double w; };
        std::vector<Rec> rec(2 * (size_t)n * K);
        for (size_t e = 0; e < (size_t)n * K; ++e) {
            const uint64_t i = e / K, j = (uint64_t)idx[e];
            const double v = umap ? w[e] : 0.0;
            rec[2 * e] = Rec{(i * (uint64_t)n + j) << 1, v};
            rec[2 * e + 1] = Rec{((j * (uint64_t)n + i) << 1) | 1, v};
        }
        std::sort(rec.begin(), rec.end(), [](const Rec &a, const Rec &b) { return a.key < b.key; });   // all keys differ
        int64_t nnz = 0;
        int64_t row_done = -1;
        for (size_t p = 0; p < rec.size();) {
            const uint64_t cell = rec[p].key >> 1;
            const bool both = p + 1 < rec.size() && (rec[p + 1].key >> 1) == cell;
            const bool out = !(rec[p].key & 1), in = (rec[p].key & 1) || both;
            const int64_t row = (int64_t)(cell / (uint64_t)n), col = (int64_t)(cell % (uint64_t)n);
            while (row_done < row) indptr[++row_done] = nnz;
            indices[nnz] = (int32_t)col;
            if (umap) {
                const double a = out ? rec[p].w : 0.0;
                const double b = !out ? rec[p].w : both ? rec[p + 1].w : 0.0;
                data[nnz] = std::fma(-a, b, a + b);
            } else {
                const int32_t *x = sorted.data() + (size_t)row * K, *y = sorted.data() + (size_t)col * K;
                int m = (out ? 1 : 0) + (in ? 1 : 0);
                for (size_t ix = 0, iy = 0; ix < K && iy < K;) {
                    if (x[ix] == y[iy]) { ++m; ++ix; ++iy; }
                    else if (x[ix] < y[iy]) ++ix;
                    else ++iy;
                }
                data[nnz] = (double)m / (double)(2 * (k + 1) - m);
            }
            ++nnz;
            p += both ? 2 : 1;
        }
        indptr[n] = nnz;
        if (umap && rho) std::copy(rho_v.begin(), rho_v.end(), rho);
        if (umap && sigma) std::copy(sigma_v.begin(), sigma_v.end(), sigma);
    });
}

// louvain.hip restated: the definition of include/schpf_hip.h line by line -- one vertex after the other
// within a round, every vertex reading the communities as the round found them, and one std::sort per aggregation
int schpf_debug_louvain(int n, const int64_t *indptr, const int32_t *indices, const double *data, double gamma,
                        int32_t *labels, int64_t stats[4])
{
    if (const char *why = louvain_bad_args(n, indptr, gamma, labels, stats)) return fail("%s", why);
    return guarded([&] {
        if (n == 0) {
            std::fill(stats, stats + 4, (int64_t)0);
            return;
        }
        const int64_t nnz = check_graph_csr(LOUVAIN_WORDS, n, n, indptr, indices, data,
                                            [&](int64_t entries) { refuse_if(louvain_bad_nnz(entries, indices, data)); });
        double wmax = 0.0;
        for (int64_t e = 0; e < nnz; ++e) wmax = data[e] > wmax ? data[e] : wmax;
        std::vector<int32_t> lab((size_t)n);
        for (int i = 0; i < n; ++i) lab[(size_t)i] = i;
        int64_t n_comm = n, levels = 0, rounds = 0, w2_first = 0;
        if (nnz > 0 && wmax > 0.0) {
            // the level's graph
            int64_t nl = n;
            std::vector<int64_t> ip(indptr, indptr + n + 1), q((size_t)nnz);
            std::vector<int32_t> ix(indices, indices + nnz);
            for (int64_t e = 0; e < nnz; ++e) q[(size_t)e] = std::llrint(std::ldexp(data[e] / wmax, 30));
            auto score = [gamma](int64_t k, int64_t base, int64_t w2, int64_t among) {
                const double p = (double)k * (double)base;
                const double t = p / (double)w2;
                return std::fma(-gamma, t, (double)among);
            };
            for (int level = 0; level < LOUVAIN_LEVELS; ++level) {
                std::vector<int64_t> k((size_t)nl, 0);
                int64_t w2 = 0;
                for (int64_t i = 0; i < nl; ++i) {
                    for (int64_t e = ip[(size_t)i]; e < ip[(size_t)i + 1]; ++e) k[(size_t)i] += q[(size_t)e];
                    w2 += k[(size_t)i];
                }
                if (level == 0) w2_first = w2;
                std::vector<int32_t> c((size_t)nl), next;
                for (int64_t i = 0; i < nl; ++i) c[(size_t)i] = (int32_t)i;
                std::vector<int64_t> tot(k);
                bool level_moved = false;
                std::vector<std::pair<int32_t, int64_t>> seen;   // (community, weight) of a row's entries
                for (int r = 0; r < LOUVAIN_ROUNDS; ++r) {
                    ++rounds;
                    next = c;
                    int64_t moves = 0;
                    for (int64_t i = 0; i < nl; ++i) {
                        const int64_t ki = k[(size_t)i];
                        if (((((uint64_t)i * 2654435761ull) >> 16) & 1) != (uint64_t)(r & 1) || ki <= 0) continue;
                        const int32_t a = c[(size_t)i];
                        seen.clear();
                        for (int64_t e = ip[(size_t)i]; e < ip[(size_t)i + 1]; ++e)
                            if (ix[(size_t)e] != i) seen.emplace_back(c[(size_t)ix[(size_t)e]], q[(size_t)e]);
                        std::sort(seen.begin(), seen.end());
                        int64_t among_own = 0;
                        bool have = false;
                        double best = 0.0;
                        int32_t best_d = 0;
                        for (size_t x = 0; x < seen.size();) {
                            const int32_t d = seen[x].first;
                            int64_t among = 0;
                            for (; x < seen.size() && seen[x].first == d; ++x) among += seen[x].second;
                            if (d == a) {
                                among_own = among;
                                continue;
                            }
                            const double s = score(ki, tot[(size_t)d], w2, among);
                            if (!have || s > best) {   // d ascends: an equal score keeps the smaller id
                                have = true;
                                best = s;
                                best_d = d;
                            }
                        }
                        if (have && best > score(ki, tot[(size_t)a] - ki, w2, among_own)) {
                            next[(size_t)i] = best_d;
                            ++moves;
                        }
                    }
                    if (moves == 0) break;
                    level_moved = true;
                    c.swap(next);
                    std::fill(tot.begin(), tot.end(), (int64_t)0);
                    for (int64_t i = 0; i < nl; ++i) tot[(size_t)c[(size_t)i]] += k[(size_t)i];
                }
                if (!level_moved) break;
                ++levels;
                // the communities that still have members, renumbered in ascending id
                std::vector<int32_t> renum((size_t)nl, 0);
                for (int64_t i = 0; i < nl; ++i) renum[(size_t)c[(size_t)i]] = 1;
                int32_t n_next = 0;
                for (int64_t d = 0; d < nl; ++d) {
                    const int32_t present = renum[(size_t)d];
                    renum[(size_t)d] = n_next;
                    n_next += present;
                }
                struct Rec { uint64_t key; int64_t q; };
                std::vector<Rec> rec(q.size());
                for (int64_t i = 0; i < nl; ++i)
                    for (int64_t e = ip[(size_t)i]; e < ip[(size_t)i + 1]; ++e)
                        rec[(size_t)e] = Rec{(uint64_t)renum[(size_t)c[(size_t)i]] * (uint64_t)n_next +
                                                 (uint64_t)renum[(size_t)c[(size_t)ix[(size_t)e]]], q[(size_t)e]};
                std::sort(rec.begin(), rec.end(), [](const Rec &x, const Rec &y) { return x.key < y.key; });
                ip.assign((size_t)n_next + 1, 0);
                ix.clear();
                q.clear();
                for (size_t p = 0; p < rec.size();) {
                    const uint64_t key = rec[p].key;
                    int64_t sum = 0;
                    for (; p < rec.size() && rec[p].key == key; ++p) sum += rec[p].q;
                    ix.push_back((int32_t)(key % (uint64_t)n_next));
                    q.push_back(sum);
                    ++ip[(size_t)(key / (uint64_t)n_next) + 1];
                }
                for (int32_t d = 0; d < n_next; ++d) ip[(size_t)d + 1] += ip[(size_t)d];
                for (int i = 0; i < n; ++i) lab[(size_t)i] = renum[(size_t)c[(size_t)lab[(size_t)i]]];
                nl = n_next;
                n_comm = n_next;
            }
        }
        std::copy(lab.begin(), lab.end(), labels);
        stats[0] = n_comm;
        stats[1] = levels;
        stats[2] = rounds;
        stats[3] = w2_first;
    });
}

// components.hip restated: a serial union-find that keeps the smaller vertex as the root, then the numbering
// by first member.  stats[4..5], the rounds of the device, are 0 here
int schpf_debug_components(int n, const int64_t *indptr, const int32_t *indices, const int32_t *within, int32_t *comp,
                           int64_t stats[6])
{
    if (const char *why = components_bad_args(n, indptr, comp, stats)) return fail("%s", why);
    return guarded([&] {
        if (n == 0) {
            std::fill(stats, stats + 6, (int64_t)0);
            return;
        }
        check_graph_csr(GRAPH_WORDS, n, n, indptr, indices, (const double *)nullptr,
                        [&](int64_t entries) { refuse_if(components_bad_nnz(entries, indices)); });
        if (within)
            for (int i = 0; i < n; ++i)
                if (within[i] < -1) throw std::invalid_argument(components_bad_within(i));
        std::vector<int32_t> p((size_t)n);
        for (int i = 0; i < n; ++i) p[(size_t)i] = i;
        auto find = [&p](int32_t x) {
            while (p[(size_t)x] != x) {
                p[(size_t)x] = p[(size_t)p[(size_t)x]];   // path halving
                x = p[(size_t)x];
            }
            return x;
        };
        int64_t edges = 0;
        for (int i = 0; i < n; ++i)
            for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                const int32_t j = indices[e];
                if (j == i || (within && !(within[i] >= 0 && within[i] == within[j]))) continue;
                ++edges;
                const int32_t a = find(i), b = find(j);
                if (a != b) p[(size_t)std::max(a, b)] = std::min(a, b);
            }
        // a root is the smallest vertex of its tree, so the roots are met in the order of the numbering
        std::vector<int32_t> number((size_t)n), size;
        for (int i = 0; i < n; ++i) {
            const int32_t r = find(i);
            if (r == i) {
                number[(size_t)i] = (int32_t)size.size();
                size.push_back(0);
            }
            ++size[(size_t)number[(size_t)r]];
        }
        int64_t largest = 0, single = 0;
        for (int32_t s : size) {
            largest = std::max<int64_t>(largest, s);
            single += s == 1;
        }
        for (int i = 0; i < n; ++i) comp[i] = number[(size_t)find(i)];
        stats[0] = (int64_t)size.size();
        stats[1] = largest;
        stats[2] = single;
        stats[3] = edges;
        stats[4] = stats[5] = 0;
    });
}

// The cluster graph of components.hip restated: one walk over the entries
int schpf_debug_cluster_graph(int n, const int64_t *indptr, const int32_t *indices, const double *data, const int32_t *labels,
                              int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight, double *wmax)
{
    if (const char *why = cluster_graph_bad_args(n, indptr, labels, ngroups, group_cells, count, wmax)) return fail("%s", why);
    return guarded([&] {
        const int64_t G = ngroups;
        const int64_t nnz = check_graph_csr(GRAPH_WORDS, n, n, indptr, indices, data,
                                            [&](int64_t entries) { refuse_if(components_bad_nnz(entries, indices)); });
        check_labels(n, labels, G, cluster_graph_bad_labels);
        double largest = data || nnz == 0 ? 0.0 : 1.0;
        for (int64_t e = 0; data && e < nnz; ++e) largest = data[e] > largest ? data[e] : largest;
        std::fill(group_cells, group_cells + G, (int64_t)0);
        std::fill(count, count + G * G, (int64_t)0);
        if (weight) std::fill(weight, weight + G * G, (int64_t)0);
        for (int i = 0; i < n; ++i) {
            const int64_t a = labels[i];
            if (a >= 0) ++group_cells[a];
            for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                const int64_t b = labels[indices[e]];
                if (indices[e] == i || a < 0 || b < 0) continue;
                ++count[a * G + b];
                if (weight) weight[a * G + b] += data && largest > 0.0 ? std::llrint(std::ldexp(data[e] / largest, 30)) : (int64_t)1 << 30;
            }
        }
        *wmax = largest;
    });
}

// geodesic.hip restated: a serial binary-heap Dijkstra per root set over the edges i -> j, and j -> i of an
// undirected graph, with the one addition d[u] + w per edge.  Floating-point addition is monotone and no length is
// negative, so a vertex leaves the heap with the greatest fixed point of the definition.  stats[1..2], the rounds and the
// lowering writes of the device, are 0 here
int schpf_debug_geodesic(int n, const int64_t *indptr, const int32_t *indices, const double *data, int directed, int nsets,
                         const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3])
{
    if (const char *why = geodesic_bad_args(n, nsets, indptr, set_ptr, dist, stats)) return fail("%s", why);
    return guarded([&] {
        if (n == 0 || nsets == 0) {
            std::fill(stats, stats + 3, (int64_t)0);
            return;
        }
        check_graph_csr(GRAPH_WORDS, n, n, indptr, indices, data, [&](int64_t entries) { refuse_if(components_bad_nnz(entries, indices)); });
        if (set_ptr[0] != 0) throw std::invalid_argument(geodesic_bad_set_ptr(0));
        for (int r = 0; r < nsets; ++r)
            if (set_ptr[r + 1] < set_ptr[r]) throw std::invalid_argument(geodesic_bad_set_ptr(r));
        if (set_ptr[nsets] > 0 && !roots) throw std::invalid_argument("roots must not be NULL");
        for (int r = 0; r < nsets; ++r)
            for (int64_t e = set_ptr[r]; e < set_ptr[r + 1]; ++e)
                if (roots[e] < 0 || roots[e] >= n) throw std::invalid_argument(geodesic_bad_roots(r));

        // the edges that leave every vertex: its stored entries, and for an undirected graph the entries stored at others
        const size_t N = (size_t)n;
        std::vector<int64_t> start(N + 1, 0);
        for (int i = 0; i < n; ++i)
            for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                if (indices[e] == i) continue;
                ++start[(size_t)i + 1];
                if (!directed) ++start[(size_t)indices[e] + 1];
            }
        for (size_t v = 0; v < N; ++v) start[v + 1] += start[v];
        std::vector<int32_t> head((size_t)start[N]);
        std::vector<double> length((size_t)start[N]);
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < n; ++i)
            for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                const int32_t j = indices[e];
                if (j == i) continue;
                const double w = data ? data[e] : 1.0;
                head[(size_t)fill[(size_t)i]] = j;
                length[(size_t)fill[(size_t)i]++] = w;
                if (!directed) {
                    head[(size_t)fill[(size_t)j]] = i;
                    length[(size_t)fill[(size_t)j]++] = w;
                }
            }

        const double inf = std::numeric_limits<double>::infinity();
        typedef std::pair<double, int32_t> Item;
        int64_t finite = 0;
        for (int r = 0; r < nsets; ++r) {
            double *d = dist + (size_t)r * N;
            std::fill(d, d + N, inf);
            std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
            for (int64_t e = set_ptr[r]; e < set_ptr[r + 1]; ++e)
                if (d[roots[e]] != 0.0) {
                    d[roots[e]] = 0.0;
                    heap.push(Item(0.0, roots[e]));
                }
            while (!heap.empty()) {
                const Item top = heap.top();
                heap.pop();
                const int32_t u = top.second;
                if (top.first > d[u]) continue;   // an entry that a later, lower one has overtaken
                ++finite;
                for (int64_t e = start[(size_t)u]; e < start[(size_t)u + 1]; ++e) {
                    const double cand = top.first + length[(size_t)e];   // the one addition of the definition
                    if (cand < d[head[(size_t)e]]) {
                        d[head[(size_t)e]] = cand;
                        heap.push(Item(cand, head[(size_t)e]));
                    }
                }
            }
        }
        stats[0] = finite;
        stats[1] = stats[2] = 0;
    });
}

// rank_sums.hip restated: the definition of include/schpf_hip.h gene by gene -- the positive entries of a
// gene sorted by value with one std::sort, then one walk over the runs of equal values
int schpf_debug_rank_sums(int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                          const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties, int64_t *nexpr,
                          int64_t *rank2)
{
    if (const char *why = rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, n, zeros, ties, nexpr, rank2))
        return fail("%s", why);
    return guarded([&] {
        const int64_t N = ncells, J = ngenes, G = ngroups;
        if (N == 0 || J == 0) {
            if (n) std::fill(n, n + G, (int64_t)0);
            if (zeros) std::fill(zeros, zeros + J, (int64_t)0);
            if (ties) std::fill(ties, ties + J, (int64_t)0);
            if (nexpr) std::fill(nexpr, nexpr + G * J, (int64_t)0);
            if (rank2) std::fill(rank2, rank2 + G * J, (int64_t)0);
            return;
        }
        check_graph_csr(RANK_SUMS_WORDS, J, N, indptr, indices, data, [&](int64_t entries) { refuse_if(rank_sums_bad_nnz(entries, indices, data)); });
        check_labels(N, labels, G, rank_sums_bad_labels);

        std::vector<int64_t> cnt((size_t)G, 0), z((size_t)J), tie((size_t)J), expr((size_t)(G * J), 0), r((size_t)(G * J), 0);
        for (int64_t i = 0; i < N; ++i)
            if (labels[i] >= 0) ++cnt[(size_t)labels[i]];
        std::vector<std::pair<float, int32_t>> pos;   // (value, group of the cell) of a gene's positive entries
        for (int64_t j = 0; j < J; ++j) {
            pos.clear();
            for (int64_t e = indptr[j]; e < indptr[j + 1]; ++e)
                if (data[e] > 0.0f) pos.emplace_back(data[e], labels[indices[e]]);
            std::sort(pos.begin(), pos.end());
            const int64_t zj = N - (int64_t)pos.size();
            z[(size_t)j] = zj;
            tie[(size_t)j] = zj * zj * zj - zj;
            for (int64_t g = 0; g < G; ++g) r[(size_t)(g * J + j)] = cnt[(size_t)g] * (zj + 1);
            for (size_t x = 0; x < pos.size();) {
                size_t y = x;
                while (y < pos.size() && pos[y].first == pos[x].first) ++y;
                const int64_t t = (int64_t)(y - x), r2 = 2 * (zj + (int64_t)x) + t + 1;
                tie[(size_t)j] += t * t * t - t;
                for (; x < y; ++x) {
                    const int32_t g = pos[x].second;
                    if (g < 0) continue;
                    ++expr[(size_t)(g * J + j)];
                    r[(size_t)(g * J + j)] += r2 - zj - 1;
                }
            }
        }
        std::copy(cnt.begin(), cnt.end(), n);
        std::copy(z.begin(), z.end(), zeros);
        std::copy(tie.begin(), tie.end(), ties);
        std::copy(expr.begin(), expr.end(), nexpr);
        std::copy(r.begin(), r.end(), rank2);
    });
}

// pair_rank_sums.hip restated: the definition of include/schpf_hip.h gene by gene -- the positive entries of
// the cells that are in a group sorted by (value, group) with one std::sort, cut into every group's list of distinct values
// with their counts, then for every pair one merge of its two lists
int schpf_debug_pair_rank_sums(int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                               const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n, int64_t *nexpr,
                               int64_t *u2, int64_t *ties)
{
    if (const char *why = pair_rank_sums_bad_args(ncells, ngenes, ngroups, indptr, labels, pairs, npairs, n, nexpr, u2, ties))
        return fail("%s", why);
    return guarded([&] {
        const int64_t N = ncells, J = ngenes, G = ngroups, P = npairs;
        if (N == 0 || J == 0) {
            if (n) std::fill(n, n + G, (int64_t)0);
            if (nexpr) std::fill(nexpr, nexpr + G * J, (int64_t)0);
            if (u2) std::fill(u2, u2 + P * J, (int64_t)0);
            if (ties) std::fill(ties, ties + P * J, (int64_t)0);
            return;
        }
        check_graph_csr(RANK_SUMS_WORDS, J, N, indptr, indices, data, [&](int64_t entries) { refuse_if(rank_sums_bad_nnz(entries, indices, data)); });
        check_labels(N, labels, G, rank_sums_bad_labels);
        for (int64_t p = 0; p < P; ++p) {
            const int64_t a = pairs[2 * p], b = pairs[2 * p + 1];
            if (a < 0 || a >= G || b < 0 || b >= G || a == b) throw std::invalid_argument(pair_rank_sums_bad_pairs(p));
        }

        std::vector<int64_t> cnt((size_t)G, 0), expr((size_t)(G * J), 0), u((size_t)(P * J), 0), tie((size_t)(P * J), 0);
        for (int64_t i = 0; i < N; ++i)
            if (labels[i] >= 0) ++cnt[(size_t)labels[i]];
        std::vector<std::pair<float, int32_t>> pos;                          // (value, group) of a gene's positive entries
        std::vector<std::vector<std::pair<float, int64_t>>> list((size_t)G);   // per group: (distinct value, cells), ascending
        for (int64_t j = 0; j < J; ++j) {
            pos.clear();
            for (int64_t e = indptr[j]; e < indptr[j + 1]; ++e)
                if (data[e] > 0.0f && labels[indices[e]] >= 0) pos.emplace_back(data[e], labels[indices[e]]);
            std::sort(pos.begin(), pos.end());
            for (size_t x = 0; x < pos.size();) {
                size_t y = x;
                while (y < pos.size() && pos[y] == pos[x]) ++y;
                list[(size_t)pos[x].second].emplace_back(pos[x].first, (int64_t)(y - x));
                expr[(size_t)(pos[x].second * J + j)] += (int64_t)(y - x);
                x = y;
            }
            for (int64_t p = 0; p < P; ++p) {
                const int64_t a = pairs[2 * p], b = pairs[2 * p + 1];
                const auto &la = list[(size_t)a], &lb = list[(size_t)b];
                const int64_t za = cnt[(size_t)a] - expr[(size_t)(a * J + j)], zb = cnt[(size_t)b] - expr[(size_t)(b * J + j)];
                const int64_t t0 = za + zb;
                int64_t below_b = zb, sum = za * zb, cubes = t0 * t0 * t0 - t0;
                for (size_t x = 0, y = 0; x < la.size() || y < lb.size();) {   // the distinct values of a and b, ascending
                    const bool in_a = x < la.size() && (y == lb.size() || la[x].first <= lb[y].first);
                    const bool in_b = y < lb.size() && (x == la.size() || lb[y].first <= la[x].first);
                    const int64_t ca = in_a ? la[x].second : 0, cb = in_b ? lb[y].second : 0, t = ca + cb;
                    sum += ca * (2 * below_b + cb);
                    cubes += t * t * t - t;
                    below_b += cb;
                    x += in_a;
                    y += in_b;
                }
                u[(size_t)(p * J + j)] = sum;
                tie[(size_t)(p * J + j)] = cubes;
            }
            for (const auto &e : pos) list[(size_t)e.second].clear();
        }
        std::copy(cnt.begin(), cnt.end(), n);
        std::copy(expr.begin(), expr.end(), nexpr);
        if (P) std::copy(u.begin(), u.end(), u2);
        if (P) std::copy(tie.begin(), tie.end(), ties);
    });
}

// residual_var.hip restated: the definition of include/schpf_hip.h as it stands -- every gene walks all N
// cells, the zeros included, and knows nothing of the split into distinct totals.  The same refusals in the same order
int schpf_debug_residual_var(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                             const float *data, double inv_theta, double clip, double *sum, double *sumsq, int64_t *cell_total,
                             int64_t *gene_total)
{
    if (const char *why = hvg_bad_args(ncells, ngenes, nnz, indptr, indices, data, inv_theta, clip, sum, sumsq)) return fail("%s", why);
    return guarded([&] {
        const int64_t N = ncells, J = ngenes;
        if (J == 0 && nnz != 0) throw std::invalid_argument(hvg_bad_indptr(0));
        // the values are judged by hvg_count below, while they are summed
        check_graph_csr(HVG_WORDS, J, N, indptr, indices, (const float *)nullptr, [&](int64_t last) {
            if (last != nnz) throw std::invalid_argument(hvg_bad_indptr(J - 1));
        });
        std::vector<int64_t> n((size_t)N, 0), s((size_t)J, 0);
        int64_t T = 0;
        for (int64_t j = 0; j < J; ++j)
            for (int64_t e = indptr[j]; e < indptr[j + 1]; ++e) {
                int64_t x;
                if (!hvg_count(data[e], x)) throw std::invalid_argument(hvg_bad_values(j));
                n[(size_t)indices[e]] += x;
                s[(size_t)j] += x;
                T += x;
            }
        std::vector<double> s1((size_t)J, 0.0), s2((size_t)J, 0.0);
        for (int64_t j = 0; j < J; ++j) {
            const double q = hvg_share(s[(size_t)j], T);
            int64_t e = indptr[j];
            for (int64_t c = 0; c < N; ++c) {
                int64_t x = 0;
                if (e < indptr[j + 1] && indices[e] == c) hvg_count(data[e++], x);
                const double mu = (double)n[(size_t)c] * q;
                if (!(mu > 0.0)) continue;   // r = 0
                const double r = ((double)x - mu) / std::sqrt(mu * (1.0 + mu * inv_theta));
                const double clipped = std::min(clip, std::max(-clip, r));
                s1[(size_t)j] += clipped;
                s2[(size_t)j] += clipped * clipped;
            }
        }
        std::copy(s1.begin(), s1.end(), sum);
        std::copy(s2.begin(), s2.end(), sumsq);
        if (cell_total) std::copy(n.begin(), n.end(), cell_total);
        if (gene_total) std::copy(s.begin(), s.end(), gene_total);
    });
}

// the draw of doublets.h, one simulated row after the other: row first + t for t < n_sim
int schpf_doublet_parents(int64_t first, int64_t n_sim, int64_t ncells, uint64_t seed, int32_t *parents)
{
    if (const char *why = doublet_parents_bad_args(first, n_sim, ncells, parents)) return fail("%s", why);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int64_t t = 0; t < n_sim; ++t)
        doublet_parents_of((uint64_t)first + (uint64_t)t, (uint32_t)ncells, k0, k1, parents + 2 * t, parents + 2 * t + 1);
    return 0;
}

// doublets.hip restated: the same refusals in the same order, then every pair as a two-pointer merge of its parents
int schpf_debug_doublet_rows(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                             const void *val, int val_kind, int64_t n_pairs, const int32_t *parents, int64_t *out_indptr,
                             int32_t *out_indices, int32_t *out_values, int64_t capacity)
{
    if (const char *why = doublet_rows_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_pairs, parents, out_indptr, out_indices,
                                                out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        if (n_pairs == 0 || nnz == 0) {
            if (out_indptr) std::fill(out_indptr, out_indptr + n_pairs + 1, (int64_t)0);
            return;
        }
        check_count_csr("doublets", ncells, ngenes, nnz, indptr, indices, val, val_kind, CSR_COUNTS);
        for (int64_t s = 0; s < n_pairs; ++s)
            if (parents[2 * s] < 0 || parents[2 * s] >= ncells || parents[2 * s + 1] < 0 || parents[2 * s + 1] >= ncells)
                throw std::invalid_argument(doublet_bad_parent(s));

        // the lengths first: out_indptr is written, the entries only where the capacity will do
        std::vector<int64_t> ptr((size_t)n_pairs + 1, 0);
        for (int64_t s = 0; s < n_pairs; ++s) {
            int64_t i = indptr[parents[2 * s]], j = indptr[parents[2 * s + 1]], n = 0;
            const int64_t i_end = indptr[parents[2 * s] + 1], j_end = indptr[parents[2 * s + 1] + 1];
            while (i < i_end && j < j_end) {
                const int32_t ci = indices[i], cj = indices[j];
                i += ci <= cj;
                j += cj <= ci;
                ++n;
            }
            ptr[(size_t)s + 1] = ptr[(size_t)s] + n + (i_end - i) + (j_end - j);
        }
        const int64_t total = ptr[(size_t)n_pairs];
        std::copy(ptr.begin(), ptr.end(), out_indptr);
        if (out_indices && capacity < total) throw std::invalid_argument(csr_bad_capacity(capacity, total));
        if (!out_indices) return;
        for (int64_t s = 0; s < n_pairs; ++s) {
            int64_t i = indptr[parents[2 * s]], j = indptr[parents[2 * s + 1]], o = ptr[(size_t)s];
            const int64_t i_end = indptr[parents[2 * s] + 1], j_end = indptr[parents[2 * s + 1] + 1];
            while (i < i_end || j < j_end) {
                const bool take_a = i < i_end && (j == j_end || indices[i] <= indices[j]);
                const bool take_b = j < j_end && (i == i_end || indices[j] <= indices[i]);
                out_indices[o] = take_a ? indices[i] : indices[j];
                out_values[o] = (take_a ? (int32_t)read_count(val, val_kind, i) : 0) + (take_b ? (int32_t)read_count(val, val_kind, j) : 0);
                i += take_a;
                j += take_b;
                ++o;
            }
        }
    });
}

// qc.hip restated: the same refusals in the same order, then one entry after the other
int schpf_debug_axis_stats(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                           const void *val, int val_kind, int n_sets, const uint32_t *gene_flags, int64_t *cell_n,
                           int64_t *cell_total, int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq)
{
    if (const char *why = qc_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_sets, gene_flags, cell_n, cell_total,
                                            cell_set_total, gene_n, gene_total, gene_sumsq))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        const size_t N = (size_t)ncells, J = (size_t)ngenes, S = (size_t)n_sets;
        if (nnz > 0) {
            const uint64_t vmax = check_count_csr("qc", ncells, ngenes, nnz, indptr, indices, val, val_kind, CSR_COUNTS);
            if (qc_sumsq_overflows(vmax, ncells)) throw std::invalid_argument(csr_bad_sumsq("qc", vmax, ncells));
        }
        for (int64_t *p : {cell_n, cell_total}) std::fill(p, p + N, (int64_t)0);
        if (N && S) std::fill(cell_set_total, cell_set_total + N * S, (int64_t)0);
        for (int64_t *p : {gene_n, gene_total, gene_sumsq}) std::fill(p, p + J, (int64_t)0);
        if (nnz == 0) return;
        for (int64_t r = 0; r < ncells; ++r)
            for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
                const int64_t v = (int64_t)read_count(val, val_kind, e), j = indices[e];
                if (v == 0) continue;   // a stored zero is no expression
                ++cell_n[r];
                cell_total[r] += v;
                for (int s = 0; s < n_sets; ++s)
                    if ((gene_flags[j] >> s) & 1u) cell_set_total[(size_t)s * N + (size_t)r] += v;
                ++gene_n[j];
                gene_total[j] += v;
                gene_sumsq[j] += v * v;
            }
    });
}

int schpf_debug_submatrix(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                          const void *val, int val_kind, int64_t n_rows, const int32_t *rows, const uint8_t *gene_keep,
                          int64_t *out_ngenes, int64_t *out_indptr, int32_t *out_indices, void *out_values, int64_t capacity)
{
    if (const char *why = qc_submatrix_bad_args(ncells, ngenes, nnz, indptr, indices, val, n_rows, rows, out_ngenes, out_indptr,
                                                out_indices, out_values, capacity))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        const bool empty = nnz == 0 || n_rows == 0;
        if (!empty) check_count_csr("qc", ncells, ngenes, nnz, indptr, indices, val, val_kind, CSR_RANGE);
        for (int64_t s = 0; rows && s < n_rows; ++s)
            if (rows[s] < 0 || rows[s] >= ncells) throw std::invalid_argument(qc_bad_rows(s));
        std::vector<int32_t> colmap((size_t)ngenes + 1, 0);   // the kept genes before gene j
        for (int64_t j = 0; j < ngenes; ++j) colmap[(size_t)j + 1] = colmap[(size_t)j] + (!gene_keep || gene_keep[j] != 0);
        std::vector<int64_t> ptr((size_t)n_rows + 1, 0);
        for (int64_t s = 0; !empty && s < n_rows; ++s) {
            const int64_t r = rows ? rows[s] : s;
            int64_t n = 0;
            for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) n += colmap[(size_t)indices[e] + 1] != colmap[(size_t)indices[e]];
            ptr[(size_t)s + 1] = ptr[(size_t)s] + n;
        }
        const int64_t total = ptr[(size_t)n_rows];
        if (out_indices && capacity < total) throw std::invalid_argument(csr_bad_capacity(capacity, total));
        *out_ngenes = colmap[(size_t)ngenes];
        std::copy(ptr.begin(), ptr.end(), out_indptr);
        if (!out_indices || total == 0) return;
        const size_t width = value_size(val_kind);
        for (int64_t s = 0, o = 0; s < n_rows; ++s) {
            const int64_t r = rows ? rows[s] : s;
            for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
                const size_t j = (size_t)indices[e];
                if (colmap[j + 1] == colmap[j]) continue;
                out_indices[o] = colmap[j];
                std::memcpy((char *)out_values + (size_t)o * width, (const char *)val + (size_t)e * width, width);   // the bytes as they are
                ++o;
            }
        }
    });
}

// group_stats.hip restated: the same refusals in the same order, then one entry after the other, the rows as
// they are stored
int schpf_debug_group_stats(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                            const void *val, int val_kind, const int32_t *labels, int64_t ngroups, int64_t *group_cells,
                            int64_t *nexpr, int64_t *total, int64_t *sumsq)
{
    if (const char *why = group_stats_bad_args(ncells, ngenes, nnz, indptr, indices, val, labels, ngroups, group_cells, nexpr, total))
        return fail("%s", why);
    return guarded([&] {
        if (csr_kinds_bad(SCHPF_IDX_I64, SCHPF_IDX_I32, val_kind)) throw std::invalid_argument("unknown index or value kind");
        const size_t G = (size_t)ngroups, J = (size_t)ngenes;
        uint64_t vmax = 0;
        if (nnz > 0) vmax = check_count_csr("group_stats", ncells, ngenes, nnz, indptr, indices, val, val_kind, CSR_COUNTS);
        check_labels(ncells, labels, ngroups, group_stats_bad_labels);
        if (sumsq && qc_sumsq_overflows(vmax, ncells)) throw std::invalid_argument(csr_bad_sumsq("group_stats", vmax, ncells));
        std::fill(group_cells, group_cells + G, (int64_t)0);
        for (int64_t *p : {nexpr, total, sumsq})
            if (p && J) std::fill(p, p + G * J, (int64_t)0);
        for (int64_t i = 0; i < ncells; ++i)
            if (labels[i] >= 0) ++group_cells[labels[i]];
        if (nnz == 0) return;
        for (int64_t r = 0; r < ncells; ++r) {
            if (labels[r] < 0) continue;
            const size_t row = (size_t)labels[r] * J;
            for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
                const int64_t v = (int64_t)read_count(val, val_kind, e);
                if (v == 0) continue;   // a stored zero is no expression
                const size_t at = row + (size_t)indices[e];
                ++nexpr[at];
                total[at] += v;
                if (sumsq) sumsq[at] += v * v;
            }
        }
    });
}


// transpose.hip restated: the same refusals in the same order, then a serial counting transpose, one entry
// after the other in stored order
int schpf_debug_transpose(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                          const void *val, int val_kind, int out_val_kind, int64_t *out_indptr, int32_t *out_cells,
                          void *out_values, int64_t *out_source)
{
    if (const char *why = transpose_bad_args(ncells, ngenes, nnz, indptr, SCHPF_IDX_I64, indices, SCHPF_IDX_I32, val, val_kind,
                                             out_val_kind, out_indptr, out_cells, out_values))
        return fail("%s", why);
    return guarded([&] {
        const size_t J = (size_t)ngenes;
        if (transpose_empty(ncells, ngenes, nnz)) {
            std::fill(out_indptr, out_indptr + J + 1, (int64_t)0);
            return;
        }
        check_count_csr("transpose", ncells, ngenes, nnz, indptr, indices, val, val_kind, CSR_ORDER);
        std::vector<int64_t> next(J + 1, 0);   // next[j + 1]: the entries of gene j, then where its next entry goes
        for (int64_t e = 0; e < nnz; ++e) ++next[(size_t)indices[e] + 1];
        for (size_t j = 0; j < J; ++j) next[j + 1] += next[j];
        std::copy(next.begin(), next.end(), out_indptr);
        const size_t width = value_size(val_kind);
        for (int64_t r = 0; r < ncells; ++r)
            for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
                const int64_t o = next[(size_t)indices[e]]++;
                out_cells[o] = (int32_t)r;
                if (out_val_kind != val_kind) static_cast<float *>(out_values)[o] = transpose_value(read_count(val, val_kind, e));
                else std::memcpy((char *)out_values + (size_t)o * width, (const char *)val + (size_t)e * width, width);   // the bytes as they are
                if (out_source) out_source[o] = e;
            }
    });
}

}  // extern "C"
