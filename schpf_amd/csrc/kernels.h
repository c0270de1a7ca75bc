// Kernel argument blocks and host-callable launchers (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace schpf {

enum { MODE_PHI = 0, MODE_LLH = 1, MODE_RANDOM = 2, MODE_ELBO = 3, MODE_LLH_ROWS = 4 };
// MODE_LLH_ROWS leaves one record of ROW_REC doubles per lane group (tile sweep: per partial-row slot task * gpb + g;
// gather sweep: per chunk) in wave_out: {sum x log r - r, sum lgamma(x + 1), entries with x > 0}
enum { ROW_REC = 3 };
// where gamma_update_kernel takes a row's accumulated sums from: nowhere (tables from the stored parameters), a dense
// [n, K] matrix, or the row's partial rows
enum { SRC_NONE = 0, SRC_DENSE = 1, SRC_STRIDED = 2 };

template <typename T> struct SweepArgs {
    const uint4 *entries;       // sliced-ELL nonzeros {minor0, val0, minor1, val1}
    const int64_t *slice_off;   // [n_slices] in uint4 units
    const int *slice_steps;     // [n_slices]
    const int *chunk_major;     // [n_slices * CPW]
    const int *chunk_natid;     // [n_slices * CPW]
    const int *wave_slice;      // [n_waves]
    const T *tab_major;         // [n_major, KP] exp-shifted E[log] (PHI, ELBO) or E[x] (LLH)
    const T *tab_minor;         // [n_minor, KP]
    const T *log_major;         // [n_major, KP] E[log x] (fallback only)
    const T *log_minor;         // [n_minor, KP]
    T *partials;                // [n_chunks, KP]
    double *wave_out;           // [n_waves] (LLH, ELBO); [n_chunks * ROW_REC] (LLH_ROWS)
    int K;
};

// LDS-staged sweep over a tile plan (plan.h, TilePlanHost)
template <typename T> struct TileArgs {
    const void *entries;           // uint4 {off16_0, val0, off16_1, val1} or packed uint2 (plan.h)
    const uint16_t *steps;         // [(block * wpb + wave) * n_windows + window]
    const int *block_rows;         // [n_blocks * gpb]
    const int *task_block, *task_w0, *task_w1;
    // loss pass over SUB-ranges of the tasks (upload.hip loss_tasks): where the sub-task's parent task ends -- entries of
    // the half-window schedule may point one sub-window beyond the sub-task, and that one is staged too; nullptr: task_w1
    const int *task_stage_end;
    const int64_t *task_wave_off;  // [task * wpb + wave] first uint4 of the wave's entries in the task
    const int *task_order;         // [launch slot] -> task (longest first); nullptr = identity
    const T *tab_major;            // [n_major, KP]
    const T *tab_minor;            // [n_minor, KP]  (staged window by window)
    const T *log_major, *log_minor;
    T *partials;                   // [n_tasks * gpb, KP]
    double *wave_out;              // [n_tasks * wpb] (LLH, ELBO); [n_tasks * gpb * ROW_REC] (LLH_ROWS)
    int K, n_minor, n_windows, win_rows, wpb;
    // balanced windows (plan.h): block b stages window w from the table rows minor_of[b * n_virtual + w * win_rows + j]
    // (-1: none); n_minor is then n_virtual.  nullptr: windows are index ranges of the table
    const int *minor_of;
    int n_virtual;
    int llh_tab_off;               // MODE_LLH / MODE_ELBO: byte offset in LDS of the logarithm table (behind the window; LlhAccumulator::TABLE_BYTES)
    int ring, slot_bytes;          // ring mode (plan.h): slots in the LDS ring (<= 1: window mode), bytes per slot
    int sync_stage;                // ring mode: half-window schedule (slots refilled at the epoch boundary)
    int single;                    // steps[] count nonzeros, (steps + 1) / 2 slots are stored (plan.h)
    uint64_t seed;                 // MODE_RANDOM
    int major_is_cell;
    // persistent launch (sweep_impl.h tile_sweep_kernel): `resident` workgroups draw the n_tasks slots of
    // task_order from queue[0]; queue == nullptr: one workgroup per task
    int *queue;
    int n_tasks, resident;
    // shader-clock probe (capi.hip profile_clock): workgroup 0 adds the shader cycles (s_memtime) and the constant-rate
    // ticks (s_memrealtime) of its stay in the launch to probe[0], probe[1], and one to probe[4]; probe[2..3] hold its
    // start stamps.  nullptr: off.  The dual launch reads the cell-side argument block's pointer
    unsigned long long *clock_probe;
};

// Fixed-order sum of n values `stride` apart, four loads in flight (the partial rows of one
// major row live far apart in HBM/L2; a rolled loop would pay one memory latency per term).
template <typename T> __device__ __forceinline__ double sum_strided(const T *__restrict__ p, int n, size_t stride)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = 0;
    for (; c + 4 <= n; c += 4) {
        const T v0 = p[0], v1 = p[stride], v2 = p[2 * stride], v3 = p[3 * stride];
        s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
        p += 4 * stride;
    }
    for (; c < n; ++c, p += stride) s0 += (double)*p;
    return (s0 + s1) + (s2 + s3);
}

template <typename T> struct UpdateArgs {
    int n, K, KP, rows_per_block;
    const T *partials;          // SRC_STRIDED:  [partial rows, KP]
    const T *dense;             // SRC_DENSE:    [n, K]
    const int *pfirst, *pcount; // SRC_STRIDED:  a row's partial rows are pfirst[row] + j * pstride, j < pcount[row]
    int64_t pstride;            //               (a gather plan's: its consecutive chunks, pstride = 1)
    double prior_shape;         // a or c
    const T *cap_shape;         // xi / eta shape [n]
    const T *cap_rate;          // xi / eta rate BEFORE this update [n]
    const double *s_other;      // [K] sum over the other loading of E[x] ...
    const T *s_other_t;         // ... or (non-null) the same in the model dtype: the all-reduced tail of the exchange buffer
    const double *s_other_part; // ... or (s_other_nb > 0) its per-block partials [s_other_nb, K], summed here:
    int s_other_nb;             //     small problems skip the separate reduce launch (capi.hip fuse_sums)
    double cap_prior_rate;      // bp or dp
    T *shape, *rate;            // [n, K] in/out
    T *cap_rate_out;            // [n]
    T *tab_e, *tab_log, *tab_exp;  // [n, KP]
    double *colsum_part;        // [nblocks, K]
};

// (vectors per lane, lanes per row) pairs the sweeps are instantiated for (sweep_impl.h SCHPF_DISPATCH*)
inline bool tile_combo_ok(int nv, int lpc)
{
    if (lpc == 1) return nv >= 1 && nv <= 7;
    if (lpc == 2 || lpc == 4 || lpc == 8) return nv >= 4 && nv <= 7;
    return lpc == 16 && nv == 4;
}
inline bool gather_combo_ok(int nv, int lpc)
{
    if (lpc == 4) return (nv >= 1 && nv <= 8) || nv == 10;
    if (lpc == 8) return nv == 6 || nv == 7 || nv == 8 || nv == 10;
    return lpc == 16 && nv >= 6 && nv <= 8;
}

template <typename T>
hipError_t launch_sweep(const SweepArgs<T> &a, int nv, int lpc, int mode, int64_t n_waves, hipStream_t st);
template <typename T>
hipError_t launch_random_phi(const SweepArgs<T> &a, int nv, int lpc, uint64_t seed, int major_is_cell,
                             int64_t n_waves, hipStream_t st);
template <typename T>
hipError_t launch_tile_sweep(const TileArgs<T> &a, int nv, int lpc, int mode, int packed, int64_t n_tasks,
                             int threads, size_t lds_bytes, hipStream_t st);
// cell-side (a0) and gene-side (a1) MODE_PHI sweeps in one launch; order[slot] = task | ~task.
// queue != nullptr (two zeroed ints): `resident` persistent workgroups draw the slots from it
template <typename T>
hipError_t launch_tile_sweep_dual(const TileArgs<T> &a0, const TileArgs<T> &a1, const int *order, int nv, int lpc,
                                  int packed, int64_t n_slots, int threads, size_t lds_bytes, int *queue, int resident,
                                  hipStream_t st);
template <typename T> hipError_t launch_gamma_update(const UpdateArgs<T> &a, int src, int nblocks, hipStream_t st);
// rows a 256-thread block of the update kernel takes per group (UpdateArgs::rows_per_block must be this)
int update_rows_per_block(int K);
hipError_t launch_colsum_reduce(const double *part, int nblocks, int K, double *out, void *mirror,
                                int mirror_is_f32, hipStream_t st);
template <typename T>
hipError_t launch_combine_strided(const T *partials, const int *pfirst, const int *pcount, int64_t pstride, int n,
                                  int K, int KP, T *out, hipStream_t st);
hipError_t launch_sum_doubles(const double *v, int64_t n, double *out, hipStream_t st);
// minibatch rows from a resident row-sorted copy (upload.hip finish_upload / upload_rows):
//   out_col/val[j] = col/val[order[j]]  (order == nullptr: identity copy)
hipError_t launch_gather_by_order(const int *order, const int *col, const float *val, int64_t nnz, int *out_col,
                                  float *out_val, hipStream_t st);
//   batch row i = source row rows[i]: its (col, val) run src_ptr[rows[i]] .. src_ptr[rows[i] + 1] goes to
//   dst_ptr[i] ..., with local row index i
hipError_t launch_gather_rows(const int *rows, int n_rows, const int64_t *src_ptr, const int *src_col,
                              const float *src_val, const int64_t *dst_ptr, int *out_row, int *out_col,
                              float *out_val, hipStream_t st);
hipError_t launch_gammaln_sum(const float *x, int64_t n, double *block_out, int nblocks, hipStream_t st);
template <typename T>
hipError_t launch_zero_rate_sum(const int *row, const int *col, int64_t n, const T *et, const T *eb, int K, int KP,
                                double *out, hipStream_t st);
// Per-row loss.  The records a MODE_LLH_ROWS sweep left, summed per major row in fixed order -- addressed as
// the update kernel addresses a row's partial rows: records pfirst[row] + j * pstride, j < pcount[row] -- into llh[n],
// gl[n], cnt[n]
hipError_t launch_row_records_reduce(const double *rec, const int *pfirst, const int *pcount, int64_t pstride, int n,
                                     double *llh, double *gl, int64_t *cnt, hipStream_t st);
// ... and the explicitly stored zeros, which the sweeps take for padding: one thread per major row that has any
// (seg_major[s]; its zeros are minor[seg_ptr[s] .. seg_ptr[s + 1]), an order fixed when the list was sorted):
// llh[row] -= sum r, cnt[row] += their number
template <typename T>
hipError_t launch_zero_rate_rows(const int *seg_major, const int *seg_ptr, int n_seg, const int *minor,
                                 const T *e_major, const T *e_minor, int K, int KP, double *llh, int64_t *cnt,
                                 hipStream_t st);
template <typename T>
hipError_t launch_segment_sum(const double *xphi, const int *order, const int64_t *mptr, int n, int K, T *out,
                              hipStream_t st);

template <typename T> hipError_t launch_elog(const T *shape, const T *rate, int64_t n, T *out, hipStream_t st);
template <typename T> hipError_t launch_ratio(const T *shape, const T *rate, int64_t n, T *out, hipStream_t st);
template <typename T>
hipError_t launch_xphi_coo(const T *x, const int *row, const int *col, const T *elt, const T *elb, int64_t nnz,
                           int K, T *out, hipStream_t st);
template <typename T>
hipError_t launch_llh_coo(const T *x, const int *row, const int *col, const T *et, const T *eb, int64_t nnz,
                          int K, T *out, hipStream_t st);
template <typename T>
hipError_t launch_shape_update(const T *xphi, const int *order, const int64_t *ptr, int n, int K, double prior,
                               T *out, hipStream_t st);
template <typename T>
hipError_t launch_ratio_colsum(const T *shape, const T *rate, int m, int K, double *part, int nblocks,
                               hipStream_t st);
template <typename T>
hipError_t launch_rate_update(const T *ps, const T *pr, const double *S, int n, int K, T *out, hipStream_t st);
template <typename T>
hipError_t launch_capacity_rate(const T *shape, const T *rate, int n, int K, double prior, T *out,
                                hipStream_t st);
// ELBO: per major row, the sum of its stored counts in the plan's (major, minor)-sorted order
// (order == nullptr: the caller's COO is in that order already); one thread per row, fixed order
hipError_t launch_count_sums(const float *val, const int *order, const int64_t *mptr, int n, double *out,
                             hipStream_t st);
// the Gamma terms of one side: per block b, part[b * (K + 2) + ...] = {the K column sums of E[x], the prior / entropy
// terms of the loadings and of their capacities, sum_i m_i * counts_i} (m_i = max_k of the row of `log_tab`); reduced
// by launch_colsum_reduce with K + 2 columns
template <typename T>
hipError_t launch_elbo_gamma(const T *shape, const T *rate, const T *cap_shape, const T *cap_rate, const T *log_tab,
                             const double *counts, int n, int K, int KP, double prior, double cap_prior_shape,
                             double cap_prior_rate, double *part, int nblocks, hipStream_t st);
// Posterior predictive row sums (predictive.hip).  launch_predictive_e: E = shape / rate of one side as
// doubles, etab[predictive_pad(n) * K] in the blocked layout the tiles are staged from.  launch_predictive_rows: per
// major row the sums over ALL minor rows of exp(-lambda), lambda, lambda^2 (lambda = E_major . E_minor), out = [zeros |
// rate | rate2] of n_major doubles each; strip = major rows per workgroup, predictive_strip()'s choice
inline int predictive_pad(int n) { return (int)(((int64_t)n + 127) / 128 * 128); }
// 64 x 64 pairs per tile unless the strips of 64 would not give every compute unit four workgroups: then 32 x 128
inline int predictive_strip(int n_major, int cu_count) { return (n_major + 63) / 64 >= 4 * cu_count ? 64 : 32; }
template <typename T>
hipError_t launch_predictive_e(const T *shape, const T *rate, int n, int K, double *etab, hipStream_t st);
hipError_t launch_predictive_rows(const double *e_major, const double *e_minor, int n_major, int n_minor, int K, int strip,
                                  double *out, hipStream_t st);
// k nearest neighbours between two sets of rows (knn.hip).  launch_knn_table: one side's rows as doubles,
// tab[knn_pad(n) * K] in the blocked layout [row / 64][k][row % 64], padding rows 0; *bad_row, a word of the call's record
// of offenders (device_call.h: preset to "none"), takes the smallest row that holds a non-finite value.  launch_knn_select: a
// workgroup per (strip of 64 query rows, segment of seg_tiles tiles of 64 reference rows) leaves the segment's sorted
// best min(k, admissible) keys (d2, r) of every row at [(q * n_seg + s) * k ...) of idx / d2 and their number in
// cnt[q * n_seg + s] (nullptr with n_seg = 1: the final lists).  launch_knn_merge: the n_seg lists of a row -> its k best
inline int knn_pad(int n) { return (int)(((int64_t)n + 127) / 128 * 128); }
inline int64_t knn_table_blocks(int n, int K) { return ((int64_t)knn_pad(n) * K + 255) / 256; }
// Strips of 64 query rows alone fill the chip when there are two per compute unit.  With fewer, the reference axis is cut
// into as many segments as bring the grid there, each at least 16 tiles (1024 rows) long, 64 at the most
inline int knn_segments(int n_query, int n_ref, int cu_count)
{
    const int64_t strips = ((int64_t)n_query + 63) / 64, want = 2 * (int64_t)cu_count;
    if (strips >= want) return 1;
    const int64_t longest = ((int64_t)n_ref + 63) / 64 / 16;
    int64_t s = (want + strips - 1) / strips;
    s = s < longest ? s : longest;
    return (int)(s < 1 ? 1 : s > 64 ? 64 : s);
}
// factors staged per pass of the select kernel and its LDS bytes: 32 factors unless the lists of a large k leave no room
inline size_t knn_lds_bytes(int k, int kc) { return 8 * ((size_t)128 * kc + 64 * 64 + 64 * (size_t)k + 64) + 4 * (64 * (size_t)k + 192); }
inline int knn_stage_factors(int k) { return knn_lds_bytes(k, 32) <= 160 * 1024 ? 32 : 16; }
template <typename T>
hipError_t launch_knn_table(const T *x, int n, int K, double *tab, unsigned long long *bad_row, hipStream_t st);
hipError_t launch_knn_select(const double *qtab, const double *rtab, int n_query, int n_ref, int K, int k,
                             int64_t self_first, int seg_tiles, int n_seg, int32_t *idx, double *d2, int *cnt,
                             hipStream_t st);
hipError_t launch_knn_merge(const int32_t *part_idx, const double *part_d2, const int *part_cnt, int n_query, int n_seg,
                            int k, int32_t *idx, double *d2, hipStream_t st);
// Weighted neighbour graphs from k-NN lists (knn_graph.hip).  launch_graph_rows: one thread per row, 64 rows
// per workgroup: *bad_idx / *bad_dist, two words of the call's record of offenders (device_call.h: preset to "none"), take
// the smallest row whose list (an index out of range, the row itself, an index twice) or whose distances (negative, not
// finite) are refused; dist != nullptr (umap): rho[n], sigma[n] and the directed weights w[n * k]; sorted != nullptr: the rows'
// indices ascending.  launch_graph_keys: the 2 n k records of the directed edges, key = ((row * n + col) << 1) | direction,
// val (may be nullptr) the edge's weight.  launch_graph_heads: head[p] = 1 where the SORTED key p starts a new (row, col).
// launch_graph_fill: pos = the exclusive scan of head; writes indptr[n + 1], indices and data; val (the sorted weights:
// umap) or sorted (the ascending lists: jaccard), exactly one of them
inline int64_t graph_row_blocks(int n) { return ((int64_t)n + 63) / 64; }
inline size_t graph_row_lds_bytes(int k) { return (size_t)64 * (size_t)k * sizeof(double); }
hipError_t launch_graph_rows(const int32_t *idx, const double *dist, int n, int k, double target, double *w, double *rho,
                             double *sigma, int32_t *sorted, unsigned long long *bad_idx, unsigned long long *bad_dist,
                             hipStream_t st);
hipError_t launch_graph_keys(const int32_t *idx, const double *w, int n, int k, uint64_t *key, double *val, hipStream_t st);
hipError_t launch_graph_heads(const uint64_t *key, int64_t n_keys, int64_t *head, hipStream_t st);
hipError_t launch_graph_fill(const uint64_t *key, const double *val, const int64_t *pos, const int32_t *sorted, int64_t n_keys,
                             int n, int k, int64_t *indptr, int32_t *indices, double *data, hipStream_t st);
hipError_t launch_digamma_array(const double *x, int64_t n, double *out, hipStream_t st);
hipError_t launch_gammaln_array(const double *x, int64_t n, double *out, hipStream_t st);

}  // namespace schpf
