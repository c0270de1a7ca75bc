/*
 * schpf_hip.h -- C ABI of libschpf_hip.so, the MI355X (gfx950) engine for the scHPF CAVI
 * hot path.
 *
 * The reference (simslab/scHPF 0.5.0) has no FFI: its seam for this path is the set of
 * numba-compiled Python callables in schpf/hpf_numba.py, imported by schpf/scHPF_.py:21
 * and schpf/loss.py:13 and called only from scHPF._fit (scHPF_.py:642-715) and
 * loss.pois_llh_pointwise (loss.py:136-138).  Every entry point below names the
 * reference interface it replaces.  The binding a maintainer would add on the
 * reference side is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; all array arguments of the stateless functions and of
 *     set/get_state are HOST pointers (the *_device entry points take device pointers and say so) to C-contiguous row-major buffers owned by the
 *     caller for the duration of the call (nothing is retained);
 *   - `dtype` selects the model precision T: SCHPF_F32 or SCHPF_F64 (the reference's
 *     scHPF(dtype=...) / hpf_numba.py:30,80);  indices are int32 (SciPy COO default);
 *   - every function returns 0 on success, non-zero on failure (SCHPF_ERR_NO_MEMORY when the
 *     device or the host ran out of memory, 1 for everything else); schpf_last_error()
 *     returns a message for the calling thread.  The library never aborts the process;
 *   - one context = one GPU = one host thread at a time.  Work is enqueued on the
 *     context's HIP stream; calls that return data to the host synchronise it.
 */
#ifndef SCHPF_HIP_H
#define SCHPF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden and an export list (csrc/libschpf_hip.map): the functions declared
 * between this pragma and its pop are everything the shared object exports */
#pragma GCC visibility push(default)

#define SCHPF_F32 0
#define SCHPF_F64 1

/* which variational distribution (scHPF_.py:264-267) */
#define SCHPF_XI 0
#define SCHPF_THETA 1
#define SCHPF_ETA 2
#define SCHPF_BETA 3

/* status of a call that failed because hipMalloc (or a host allocation of the plan builders) found no memory */
#define SCHPF_ERR_NO_MEMORY 2

/* element type of the COO values handed to schpf_upload_coo */
#define SCHPF_VAL_I32 0
#define SCHPF_VAL_I64 1
#define SCHPF_VAL_F32 2
#define SCHPF_VAL_F64 3

/* step flags (keyword arguments of scHPF._fit, scHPF_.py:526-530) */
#define SCHPF_FREEZE_GENES 1u   /* freeze_genes=True: skip the eta/beta block (project()) */
#define SCHPF_SIMULTANEOUS 2u   /* beta_theta_simultaneous=True (scHPF_.py:666-685)      */
#define SCHPF_CELLS_FIRST 8u    /* minibatch order (scHPF_.py:688-704): xi/theta block first (theta.rate
                                   from the current beta), then the gene block from the NEW theta    */
#define SCHPF_LOCAL_GENE 16u    /* schpf_step_local: only the gene-side sweep (+ packing)           */
#define SCHPF_LOCAL_CELL 32u    /* schpf_step_local: only the cell-side sweep; neither bit = both.
                                   Lets the host start the all-reduce of the gene-side sums and
                                   overlap it with the cell-side sweep.                             */
#define SCHPF_SHARDED 4u        /* cells are sharded over several GPUs: gene-side sums go
                                   through the exchange buffer (all-reduced by the host) */

typedef struct schpf_ctx schpf_ctx;

const char *schpf_last_error(void);
int schpf_device_count(int *count);
const char *schpf_version(void);

/* ---------------------------------------------------------------------------------
 * Stateless operator mirrors: array in, array out, caller's COO order.
 *
 * nfactors: every one of the five operators refuses nfactors < 1 ("nfactors must be at
 * least 1") on the host, before anything is allocated, uploaded or launched.  Only
 * schpf_rate_update has an upper limit, [1, 256]: its column-sum kernel deals the 256
 * threads of a block out as 256 / nfactors rows of nfactors factors.  schpf_xphi,
 * schpf_pois_llh_pointwise, schpf_shape_update and schpf_capacity_rate_update loop over the
 * factors and take any nfactors >= 1.  The library reads exactly the element counts given
 * below behind every pointer; it cannot see an array's real length (schpf_amd/hpf_hip.py
 * checks every array's shape before it takes a pointer).
 * ------------------------------------------------------------------------------- */

/* hpf_numba.psi / hpf_numba.cgammaln (hpf_numba.py:16-22): double -> double. */
int schpf_digamma(int64_t n, const double *x, double *out);
int schpf_gammaln(int64_t n, const double *x, double *out);

/* compute_Xphi_data(X_data, X_row, X_col, theta_vi_shape, theta_vi_rate, beta_vi_shape,
 * beta_vi_rate) -> Xphi (nnz, K)                              hpf_numba.py:54-114.
 * x: (nnz,) of T;  row/col: (nnz,) int32;  theta_*: (ncells, K);  beta_*: (ngenes, K). */
int schpf_xphi(int dtype, int64_t nnz, int ncells, int ngenes, int nfactors, const void *x,
               const int32_t *row, const int32_t *col, const void *theta_shape,
               const void *theta_rate, const void *beta_shape, const void *beta_rate, void *out);

/* compute_pois_llh(...) -> llh (nnz,)                         hpf_numba.py:24-51. */
int schpf_pois_llh_pointwise(int dtype, int64_t nnz, int ncells, int ngenes, int nfactors,
                             const void *x, const int32_t *row, const int32_t *col,
                             const void *theta_shape, const void *theta_rate,
                             const void *beta_shape, const void *beta_rate, void *out);

/* compute_loading_shape_update(Xphi_data, X_keep, nkeep, shape_prior) -> (nkeep, K)
 *                                                             hpf_numba.py:128-156. */
int schpf_shape_update(int dtype, int64_t nnz, int nfactors, const void *xphi,
                       const int32_t *keep, int nkeep, double shape_prior, void *out);

/* compute_loading_rate_update(prior_vi_shape, prior_vi_rate, other_loading_vi_shape,
 * other_loading_vi_rate) -> (n, K)                            hpf_numba.py:159-177.
 * prior_*: (n,);  other_*: (m, K). */
int schpf_rate_update(int dtype, int n, int m, int nfactors, const void *prior_shape,
                      const void *prior_rate, const void *other_shape, const void *other_rate,
                      void *out);

/* compute_capacity_rate_update(loading_vi_shape, loading_vi_rate, prior_rate) -> (n,)
 *                                                             hpf_numba.py:180-188. */
int schpf_capacity_rate_update(int dtype, int n, int nfactors, const void *shape,
                               const void *rate, double prior_rate, void *out);

/* ---------------------------------------------------------------------------------
 * The engine: device-resident state for scHPF._fit's loop (scHPF_.py:642-715).
 * ------------------------------------------------------------------------------- */

/* Create a context on HIP device `device`.  `stream`: a hipStream_t to enqueue on; NULL lets the
 * library create a (non-blocking) stream of its own; SCHPF_STREAM_DEFAULT selects the device's
 * null stream -- torch.cuda.current_stream().cuda_stream is 0 for it, which a caller must map to
 * SCHPF_STREAM_DEFAULT when it wants its collectives ordered with the engine's kernels.
 * ncells is the number of LOCAL cells when cells are sharded. */
#define SCHPF_STREAM_DEFAULT ((void *)1)
int schpf_create(schpf_ctx **out, int device, void *stream, int dtype, int ncells, int ngenes,
                 int nfactors);
int schpf_destroy(schpf_ctx *ctx);

/* The count matrix X (scipy coo_matrix: X.row, X.col, X.data), any order, duplicates kept
 * as separate observations like the reference (hpf_numba.py:98-112).  Validates on the host,
 * copies the triples to the device and builds both sweep plans there (the host
 * builder, SCHPF_DEVICE_PLAN=0, gives the same plans bit for bit).  Values must be finite and
 * >= 0 -- the reference takes any X.data (hpf_numba.py:98-112).  They are stored as float32: UMI
 * counts are exact; other values are rounded (relative 6e-8) and counted in schpf_upload_info.
 * Explicitly stored zeros add nothing to the updates and -r each to the loss, as in the reference
 * (hpf_numba.py:43-50).  Host pointers are not retained. */
int schpf_upload_coo(schpf_ctx *ctx, int64_t nnz, const int32_t *row, const int32_t *col,
                     const void *val, int val_kind);

/* The same matrix when it is in GPU memory already, as a COO or as a CSR (a torch sparse tensor, the output of a
 * GPU-side filtering step): nothing of O(nnz) crosses PCIe.  Everything schpf_upload_coo does with host
 * threads -- validation, conversion to float32 / int32, the stored-zero list, the order of the entries, the samples of
 * the task-range model -- runs as device passes, and the engine then holds what schpf_upload_coo would hold after the
 * same entries in the same order: the same plans and upload_info, every later result bit for bit.  Under
 * SCHPF_PLAN=gather / SCHPF_DEVICE_PLAN=0 the converted triples are staged to the host builders (the cross-check).
 *   row/col/val (indptr/indices/val): DEVICE pointers on the context's device, complete before the call, not
 *   modified, not retained; on return the engine has finished reading them.  Indices are int32 or int64 (idx_kind;
 *   a CSR's indptr[ncells + 1] has a kind of its own), values of any SCHPF_VAL_* kind; int32 / float32 arrays are
 *   read in place.
 * Errors carry schpf_upload_coo's messages, "COO index out of range at entry N" (negative, >= ncells / ngenes, or an
 * int64 beyond int32) and "X.data must be finite and >= 0; offending entry N", with THIS path's rule for N: the smallest
 * offending entry of the whole matrix, an index error before a value error (the host path reports per slab of its
 * threads).  A CSR is refused unless indptr[0] == 0, indptr is non-decreasing and indptr[ncells] == nnz.
 * nnz >= 2^31 and NULL pointers with nnz > 0 are refused.  A failed upload leaves the engine without a matrix. */
#define SCHPF_IDX_I32 0
#define SCHPF_IDX_I64 1
int schpf_upload_coo_device(schpf_ctx *ctx, int64_t nnz, const void *row, const void *col, int idx_kind,
                            const void *val, int val_kind);
int schpf_upload_csr_device(schpf_ctx *ctx, int64_t nnz, const void *indptr, int indptr_kind,
                            const void *indices, int idx_kind, const void *val, int val_kind);

/* Row sums (per local cell) and column sums (per gene) of the matrix the engine holds, as the doubles it already
 * keeps for the ELBO shift terms: sums of the stored float32 values in plan order, exact for counts.  Host arrays of
 * ncells / ngenes (either may be NULL).  Fails on a batch engine (schpf_upload_rows). */
int schpf_marginals(schpf_ctx *ctx, double *row_sums, double *col_sums);

/* a, c (shape priors of theta, beta) and bp, dp (rate hyper-priors; scHPF_.py:847-879).
 * ap/cp only enter through the constant xi/eta shapes (scHPF_.py:616-618), which the
 * caller sets with schpf_set_state. */
int schpf_set_hypers(schpf_ctx *ctx, double a, double c, double bp, double dp);

/* vi_shape / vi_rate of one HPF_Gamma (scHPF_.py:27-81); (n,) for xi/eta, (n, K) else. */
int schpf_set_state(schpf_ctx *ctx, int which, const void *shape, const void *rate);
int schpf_get_state(schpf_ctx *ctx, int which, void *shape, void *rate);
/* The same with DEVICE pointers of the engine's dtype on the context's device (copies on the context's stream; both
 * calls synchronise it before returning, so the caller may release or read its arrays at once). */
int schpf_set_state_device(schpf_ctx *ctx, int which, const void *shape, const void *rate);
int schpf_get_state_device(schpf_ctx *ctx, int which, void *shape, void *rate);

/* t == 0 of a fit with reinit=True (scHPF_.py:652-655): X*phi with phi ~ Dirichlet(1_K).
 * _host: the caller drew it (NumPy, seed-compatible with the reference) and passes
 *        Xphi_data, (nnz, K) float64, in the order of the uploaded COO.
 * _device: counter-based generator on the GPU (not NumPy-compatible; for matrices whose
 *        nnz*K host draw is impractical).
 * The next schpf_step / schpf_step_local consumes it instead of computing responsibilities. */
int schpf_init_phi_host(schpf_ctx *ctx, const double *xphi);
int schpf_init_phi_device(schpf_ctx *ctx, uint64_t seed);

/* One CAVI iteration, the body of the loop at scHPF_.py:657-714 (non-batched order):
 * responsibilities -> [beta.shape, beta.rate, eta.rate] -> [theta.shape, theta.rate,
 * xi.rate].  schpf_step = schpf_step_local + schpf_step_finish on one GPU. */
int schpf_step(schpf_ctx *ctx, unsigned flags);

/* n iterations in one call -- the iterations between two loss checks of scHPF._fit
 * (scHPF_.py:642-718 with check_freq).  Same result as n schpf_step calls; from the second call
 * with the same (flags, n) the iterations are replayed as one hipGraph (SCHPF_GRAPH=0 disables). */
int schpf_steps(schpf_ctx *ctx, unsigned flags, int n);

/* Sharded form: _local runs both sweeps and packs the gene-side sums [G*K] followed by
 * the local sum_i E[theta_ik] [K] into the exchange buffer (device memory, dtype T);
 * the host all-reduces (sum) that buffer over the ranks (RCCL), then calls _finish. */
int schpf_step_local(schpf_ctx *ctx, unsigned flags);
int schpf_exchange_buffer(schpf_ctx *ctx, void **device_ptr, int64_t *count);
int schpf_step_finish(schpf_ctx *ctx, unsigned flags);

/* Loss terms of mean_negative_pois_llh (loss.py:142-168) for the CURRENT state over the
 * local nonzeros:  llh_sum = sum x*log(r) - r,  gammaln_sum = sum lgamma(x+1).
 * mean negative llh = -(llh_sum - gammaln_sum) / nnz  (sum the three over ranks first). */
int schpf_loss_terms(schpf_ctx *ctx, double *llh_sum, double *gammaln_sum, int64_t *nnz);

/* The evidence lower bound of the current state, split into its terms:
 * terms[0] data, [1] logfac, [2] rate, [3] cell, [4] gene;  ELBO = t0 - t1 - t2 + t3 + t4.
 * ap, cp: the shape priors of xi / eta (the engine holds a, c, bp, dp from schpf_set_hypers).
 * Over the local cells (a shard: sum data, logfac, rate, cell over the ranks; gene is replicated).
 * A batch engine (schpf_upload_rows) fails, as schpf_loss_terms does.  Definition: DESIGN.md 11. */
int schpf_elbo_terms(schpf_ctx *ctx, double ap, double cp, double terms[5]);

#define SCHPF_BY_CELL 0
#define SCHPF_BY_GENE 1
/* Per major row m of the chosen axis, over the LOCAL stored entries (duplicates are separate observations, stored
 * zeros count): llh_sum[m] = sum x log r - r, gammaln_sum[m] = sum lgamma(x+1), count[m] = stored entries.
 * Mean negative llh of row m = -(llh_sum[m] - gammaln_sum[m]) / count[m].  Host arrays of ncells (local) / ngenes.
 * Sweeps the plan whose major axis is `by`, reads the state only, no atomics: two calls on one state return the
 * same bits.  Its scratch is allocated by the first call (SCHPF_ERR_NO_MEMORY if that fails) and released by the next
 * upload.  A shard: concatenate the cells' arrays over the ranks, sum the genes'.  A batch engine
 * (schpf_upload_rows) fails, as schpf_loss_terms does.  Definition: DESIGN.md 12. */
int schpf_loss_rows(schpf_ctx *ctx, int by, double *llh_sum, double *gammaln_sum, int64_t *count);

/* Posterior predictive check.  With the plug-in rates lambda_ig = sum_k E[theta_ik] E[beta_gk] (E = shape /
 * rate of the state the engine holds), per major row r of the axis `by` and over ALL rows m of the other axis -- stored
 * or not, the matrix plays no part and none need be uploaded:
 *   zeros[r] = sum_m exp(-lambda_rm)   the expected number of zero entries of the row
 *   rate[r]  = sum_m lambda_rm         the expected sum of the row
 *   rate2[r] = sum_m lambda_rm^2       with n rows m: the predicted variance of an entry of the row is
 *                                      rate/n + rate2/n - (rate/n)^2  (Poisson given lambda, law of total variance)
 * Host arrays of ncells (SCHPF_BY_CELL) / ngenes (SCHPF_BY_GENE) doubles; a NULL output is skipped, all three NULL and
 * any other `by` fail with a message.  Arithmetic in double from the stored shape / rate in both dtypes; reads the state
 * only, no atomics: two calls on one state return the same bits, and the next iteration finds what it would have found.
 * Its device scratch is made by the first call.  A shard: `by` cell covers the local cells; sum the genes' over the ranks. */
int schpf_predictive_rows(schpf_ctx *ctx, int by, double *zeros, double *rate, double *rate2);

int schpf_synchronize(schpf_ctx *ctx);

/* Cells sharded over the GPUs of a node, the collective inside the library (RCCL over xGMI, bound
 * at run time to the copy of librccl.so already in the process -- PyTorch's when torch is loaded
 * -- else $SCHPF_RCCL_PATH, else /opt/rocm/lib).  One context per GPU (per process, or per host
 * thread of one process).  schpf_comm_unique_id: 128 bytes from ONE rank, handed to all others by
 * the host (a file, MPI, torch.distributed, a Python list between threads); schpf_comm_init: every
 * rank, collectively (it blocks until all `world` ranks have called it).  schpf_steps_sharded =
 * n x [schpf_step_local(gene side) -> all-reduce of the exchange buffer on the communicator's own
 * stream, under the cell-side sweep -> schpf_step_finish]; freeze_genes needs no exchange.
 * schpf_loss_terms_all = schpf_loss_terms summed over the ranks. */
/* Before schpf_upload_coo, optional: tell the context that its iterations will be sharded ones (the two
 * sweeps then run as two launches, and the plans of a small row block are cut into tasks that fill the
 * GPU once per launch instead of once per pair of launches). */
int schpf_hint_sharded(schpf_ctx *ctx, int on);
/* Before schpf_upload_coo, optional: this context's matrix is replaced every iteration or so (the host-slicing
 * fall-back of minibatch CAVI, scHPF_.py:643-650): plans are then built the cheapest way -- windows cut by index, no
 * balancing pass (plan.h BALANCED WINDOWS pays for itself over tens of iterations on one matrix, not over one). */
int schpf_hint_transient(schpf_ctx *ctx, int on);

/* Minibatch CAVI without re-uploads (the reference re-slices X each iteration: X[batch_ix], scHPF_.py:643-650,
 * with util.minibatch_ix_generator :218-231).  schpf_keep_rows(ctx, 1) BEFORE schpf_upload_coo makes the engine
 * keep, beside its plans, a (row, col)-sorted copy of the matrix in HBM.  schpf_upload_rows(batch, source, rows, n)
 * then makes `batch`'s matrix the rows rows[0..n) of `source`'s (local cell i = source cell rows[i]; n must be the
 * ncells `batch` was created with, same device, dtype, ngenes, nfactors): gathered and planned on the device,
 * nothing crosses PCIe but the n row numbers.  A batch engine has no loss constants: schpf_loss_terms on it fails,
 * evaluate the loss on the source. */
int schpf_keep_rows(schpf_ctx *ctx, int on);
int schpf_upload_rows(schpf_ctx *ctx, schpf_ctx *source, const int32_t *rows, int n_rows);
int schpf_comm_unique_id(void *out128);
int schpf_comm_init(schpf_ctx *ctx, const void *unique_id128, int rank, int world);
int schpf_comm_destroy(schpf_ctx *ctx);
int schpf_steps_sharded(schpf_ctx *ctx, unsigned flags, int n);
int schpf_loss_terms_all(schpf_ctx *ctx, double *llh_sum, double *gammaln_sum, int64_t *nnz);

/* The hipStream_t the context enqueues on (0 = the null stream), so that a caller can order its
 * own work -- the all-reduce of the exchange buffer -- with the engine's kernels. */
int schpf_stream_handle(schpf_ctx *ctx, void **stream);

/* HIP-event timing of the sweep kernel launches on the context's stream (bench.py).
 * ms[0] = cell sweep, ms[1] = gene sweep, ms[2] = loss sweep, ms[3] = gamma updates;
 * launches[] likewise.  When both sweeps of an iteration run as ONE launch (the default for
 * schpf_step) that launch is counted under ms[0]/launches[0] and ms[1] stays 0.
 * Reading synchronises the stream and resets the counters. */
int schpf_profile_enable(schpf_ctx *ctx, int enable);
int schpf_profile_read(schpf_ctx *ctx, double ms[4], int64_t launches[4]);

/* Shader clock (MHz) the device sustained UNDER the sweep launches on this context since the last call: workgroup 0 of
 * every tile-plan sweep launch stamps the shader-cycle counter and the constant-rate counter on entry and exit
 * (sweep_impl.h clock_probe_*); launches = how many launches the figure averages (0: none ran, shader_mhz = 0).
 * Synchronises the stream and resets the accumulators.  bench.py's roofline.sclk_mhz. */
int schpf_profile_clock(schpf_ctx *ctx, double *shader_mhz, int64_t *launches);

/* Bytes ONE iteration moves through the LDS and streams from HBM, computed from the tile plans (all zero for the
 * gather plan): info = {LDS reads of the nonzeros alone (2 * nnz table rows of KP values), LDS reads of every stored
 * step slot (padding included), LDS writes of the window stagings cell side, gene side, entry-stream bytes of both
 * plans in HBM, partial-row bytes written, the plan the loss pass sweeps (0 cell-major, 1 gene-major: the model of
 * capi.hip loss_tasks / loss_side), the tasks it runs as}.  bench.py's roofline.lds and loss_pass. */
int schpf_sweep_bytes(schpf_ctx *ctx, int64_t info[8]);

/* Plan facts for reports: info[0..] = KP, KL, LPC, chunk_len (tile plan: minus the rows per LDS
 * window / ring slot), windows_cell, windows_gene, n_chunks_cell, n_chunks_gene, n_waves_cell,
 * n_waves_gene, stored entry slots cell, gene, ring slots cell, gene (1 = window schedule),
 * bytes per ring slot, waves per workgroup */
int schpf_plan_info(schpf_ctx *ctx, int64_t info[16]);

/* Facts about the uploaded matrix: info = {nnz, values that were rounded to float32, explicitly
 * stored zeros, bit 0: the packed 8-byte entry format is in use | bit 1: a row-sorted copy is resident
 * (schpf_keep_rows took effect: device-built tile plans)}. */
int schpf_upload_info(schpf_ctx *ctx, int64_t info[4]);

/* Row sums (per cell) and column sums (per gene) of a host COO matrix: the inputs of the empirical
 * hyperparameters bp = ap * mean/var(cell sums), dp = cp * mean/var(gene sums)
 * (scHPF_.py:847-879, where they are X.sum(1) / X.sum(0)).  Host-side, multi-threaded, no GPU
 * needed; sums are accumulated in double (exact for counts).  row_sums[ncells], col_sums[ngenes]. */
int schpf_coo_marginals(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int val_kind,
                        int ncells, int ngenes, double *row_sums, double *col_sums);

/* Count thinning (count splitting): every stored count x is split into x_test ~ Binomial(x, frac) and
 * x_train = x - x_test, so that a model fitted to the train matrix can be scored on the test matrix (for x ~ Poisson(l)
 * the parts are independent Poisson((1 - frac) l) and Poisson(frac l)).  The draw of an entry depends on (seed, frac, row,
 * col, x) alone -- philox.h: Philox4x32-10 keyed by the seed, counter (row, col, block, 0), trial t goes to the test
 * matrix iff word t % 4 of block t / 4 is < floor(frac * 2^32) -- not on the entry's position, the index or value type,
 * or where the matrix lives.  Entries that share a coordinate share a stream: sum duplicates first.
 *   train / test: int32[nnz], the parts in the order of the entries.  stats = {train nonzeros, test nonzeros, sum of
 *   train, sum of test}.  0 < frac < 1 and frac >= 2^-32; every value a non-negative integer <= 2^24 (float values must
 *   be integral), every index in [0, 2^31).  An invalid entry is never drawn: the call fails with "COO index out of range
 *   at entry N" or "thinning needs integer counts in [0, 2^24]; offending entry N", N the smallest offending entry of
 *   the whole matrix, an index error before a value error, and the outputs are then unspecified.  nnz = 0 succeeds with
 *   zero statistics; nnz >= 2^31 and NULL pointers with nnz > 0 are refused.
 * _device: row / col (of idx_kind) / val (of val_kind) and train / test are DEVICE pointers on `device`, read and written
 *   in place -- nothing of O(nnz) crosses PCIe; stream as in schpf_create (NULL = a stream of the call's own), on which the
 *   inputs must be complete or ordered; synchronised before the call returns.
 * schpf_thin_counts: host pointers; the entries are staged through the device in slabs; the same result. */
int schpf_thin_counts_device(int device, void *stream, int64_t nnz, const void *row, const void *col, int idx_kind,
                             const void *val, int val_kind, double frac, uint64_t seed, int32_t *train, int32_t *test,
                             int64_t stats[4]);
int schpf_thin_counts(int device, int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int val_kind,
                      double frac, uint64_t seed, int32_t *train, int32_t *test, int64_t stats[4]);
/* Test hooks (host only, no GPU needed): the serial restatement of the thinning kernels on the same header, which they
 * must match bit for bit, and one block of the generator. */
int schpf_debug_thin_counts(int64_t nnz, const int32_t *row, const int32_t *col, const void *val, int val_kind,
                            double frac, uint64_t seed, int32_t *train, int32_t *test, int64_t stats[4]);
int schpf_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* Nearest neighbours in factor space: for every row of query[n_query, nfactors] its k nearest rows of
 * ref[n_ref, nfactors], exact (every pair is looked at), both row-major and of `dtype`.  Definition, which the result
 * equals bit for bit however the work was scheduled:
 *   every value is converted to double (exact);  d2(q, r) = the result of
 *       d2 = 0;  for f = 0 .. nfactors - 1, in this order:  d = query[q][f] - ref[r][f];  d2 = fma(d, d, d2)
 *   in double with exactly this subtraction and this fused multiply-add (not |a|^2 + |b|^2 - 2ab, which cancels);
 *   the pairs of a query row are ordered by the key (d2, r): the smaller d2 first, equal d2 by the smaller r -- a total
 *   order, so the k smallest are unique;
 *   self_first >= 0 removes the one pair r == self_first + q from row q (a cell as its own neighbour: by index, not by
 *   distance, so duplicate rows at distance 0 stay neighbours); self_first = -1 removes nothing.
 *   idx[q * k + j] (int32) and d2[q * k + j] (double), j < k: the k smallest pairs of row q, ascending in the key.
 * 1 <= k <= 128 and k <= the admissible reference rows of every query row; 1 <= nfactors <= 256; n_query, n_ref <
 * 2^31 - 128.  n_query = 0 succeeds and writes nothing; n_ref = 0, a k out of range and NULL pointers fail with a message.
 * Non-finite values are refused before anything is selected, with "scores must be finite; offending row N of query" (or
 * "of ref"), N the smallest such row, query before ref; nothing is written then.  With finite inputs d2 is never NaN; a d2
 * that overflows is +inf and sorts by r.  query == ref (the same pointer, n_query == n_ref) is the usual self graph, with
 * self_first = 0.  Stateless; device memory that cannot be had returns SCHPF_ERR_NO_MEMORY.
 * _device: query, ref, idx and d2 are DEVICE pointers on `device`; stream as in schpf_create (NULL = a stream of the
 *   call's own), on which the inputs must be complete or ordered; synchronised before the call returns.
 * schpf_knn: host pointers, staged through the device; the same result.
 * schpf_debug_knn: test hook (host only, no GPU needed): the serial restatement of the definition -- a loop over the pairs
 *   with std::fma and a partial sort on the key -- which both must match bit for bit. */
int schpf_knn_device(int device, void *stream, int dtype, int n_query, int n_ref, int nfactors, const void *query,
                     const void *ref, int k, int64_t self_first, int32_t *idx, double *d2);
int schpf_knn(int device, int dtype, int n_query, int n_ref, int nfactors, const void *query, const void *ref, int k,
              int64_t self_first, int32_t *idx, double *d2);
int schpf_debug_knn(int dtype, int n_query, int n_ref, int nfactors, const void *query, const void *ref, int k,
                    int64_t self_first, int32_t *idx, double *d2);

/* Weighted neighbour graphs from k-NN lists: the exact self graph of schpf_knn (self_first = 0) turned into
 * the symmetric n x n CSR matrix a clustering or a layout reads -- UMAP's fuzzy simplicial set (scanpy's
 * obsp["connectivities"]) or the shared-neighbour Jaccard graph (Phenograph, Seurat).  Definition, which the result equals
 * bit for bit however the work was scheduled:
 * Inputs.  idx[n][k] (int32) and dist[n][k] (double), row-major: row i lists k rows j with a distance each.  1 <= k <= 128,
 *   k <= n - 1, n < 2^31 - 128.  Refused, the outputs untouched, N the smallest offending row, lists before distances:
 *     an index outside [0, n), equal to its own row, or twice in a row:
 *       "neighbour lists must hold k distinct rows other than the row itself; offending row N"
 *     (SCHPF_GRAPH_UMAP) a distance that is negative or not finite: "distances must be finite and >= 0; offending row N"
 *   Ascending distances are NOT required; cosine distances are taken as they are.
 * SCHPF_GRAPH_UMAP: UMAP's fuzzy simplicial set with local_connectivity = 1, bandwidth = 1, set_op_mix_ratio = 1.  All
 *   arithmetic in double, every sum serial in column order j = 0 .. k - 1:
 *     rho_i = the smallest strictly positive dist[i][j], 0 if there is none;  target = log2(k + 1) (std::log2 on the host;
 *       UMAP's n_neighbors counts the cell itself: k = 14 here is scanpy's n_neighbors = 15);
 *     W(e, s):  t = e / s (IEEE division);  W = t > 708 ? 0.0 : fast_exp(-t)  (csrc/special.h; the cut keeps denormals out);
 *     sigma_i by bisection:  lo = 0, hi = inf, mid = 1;  at most 64 rounds of
 *         psum = sum_j (dist[i][j] - rho_i > 0 ? W(dist[i][j] - rho_i, mid) : 1.0);
 *         if fabs(psum - target) < 1e-5: stop;
 *         if psum > target:  hi = mid, mid = (lo + hi) / 2;
 *         else:  lo = mid, mid = (hi == inf) ? mid * 2 : (lo + hi) / 2;
 *       sigma_i = mid;  then, if rho_i > 0 and sigma_i < 1e-3 * mean_i (mean_i = the row's sum of distances / k):
 *       sigma_i = 1e-3 * mean_i  (a row with rho_i = 0 has all distances 0 and all weights 1: its sigma is what the loop left);
 *     directed weight  w_ij = (dist[i][j] - rho_i <= 0) ? 1.0 : W(dist[i][j] - rho_i, sigma_i);
 *     union: for every unordered pair {i, j} with an edge either way, a = w_ij (0 if j is not in row i), b = w_ji likewise,
 *       c = fma(-a, b, a + b) -- symmetric in a and b bit for bit.
 * SCHPF_GRAPH_JACCARD: N+(i) = {i} and row i (a cell belongs to its own neighbourhood, Seurat's convention); for the same
 *   pairs m = |N+(i) ^ N+(j)| and c = (double)m / (double)(2 * (k + 1) - m).  dist is not read and may be NULL.
 * Output: the CSR matrix of c.  indptr[n + 1] (int64); indices (int32) and data (double), both of capacity 2 * n * k, the
 *   bound; nnz = indptr[n].  Columns strictly ascending within a row, no diagonal, every pair in both rows with the same
 *   bits; an edge whose c is exactly 0 is still stored (the structure depends on idx alone).  rho[n], sigma[n]: optional
 *   outputs of SCHPF_GRAPH_UMAP, may be NULL (not written by SCHPF_GRAPH_JACCARD).
 * n = 0 succeeds and writes nothing; bad arguments fail with a message.  Stateless; device memory that cannot be had
 * returns SCHPF_ERR_NO_MEMORY (scratch: about 72 n k bytes for umap, 52 n k for jaccard, and the sort's own).
 * _device: idx, dist and the outputs are DEVICE pointers on `device`; stream as in schpf_knn_device; synchronised before
 *   the call returns.
 * schpf_knn_graph: host pointers, staged through the device; the same result.
 * schpf_debug_knn_graph: test hook (host only, no GPU needed): the serial restatement of the definition, which both must
 *   match bit for bit. */
#define SCHPF_GRAPH_UMAP 0
#define SCHPF_GRAPH_JACCARD 1
int schpf_knn_graph_device(int device, void *stream, int method, int n, int k, const int32_t *idx, const double *dist,
                           int64_t *indptr, int32_t *indices, double *data, double *rho, double *sigma);
int schpf_knn_graph(int device, int method, int n, int k, const int32_t *idx, const double *dist, int64_t *indptr,
                    int32_t *indices, double *data, double *rho, double *sigma);
int schpf_debug_knn_graph(int method, int n, int k, const int32_t *idx, const double *dist, int64_t *indptr,
                          int32_t *indices, double *data, double *rho, double *sigma);

/* Louvain clustering of a weighted neighbour graph: the labels a clustering of the cells reads off the
 * matrix schpf_knn_graph made.  The weights are quantised once to int64, so every sum below is an integer sum, exact in any
 * order; doubles appear in one score per candidate, a fixed expression of exact integers; moves are synchronous.  The result
 * is one well-defined labelling, equal bit for bit however the work was scheduled:
 * Input.  A CSR matrix n x n: indptr[n + 1] (int64), indices (int32), data (double), nnz = indptr[n] < 2^32; columns strictly
 *   ascending within a row, entries finite and >= 0, a diagonal allowed; symmetric in structure and in bits -- what
 *   schpf_knn_graph returns.  SYMMETRY IS THE CALLER'S CONTRACT AND IS NOT CHECKED: an asymmetric matrix is clustered as
 *   it stands, every row by its own entries.  gamma: the resolution, finite and > 0.  n < 2^31 - 128.
 *   Refused, the outputs untouched, N the smallest offending row, structure before values, indptr before columns:
 *     "indptr must be 0 at row 0 and must be non-decreasing; offending row N"  (indptr[0] != 0: row 0; indptr[N + 1] <
 *       indptr[N]: row N)
 *     "columns must be in [0, n) and strictly ascending within a row; offending row N"
 *     "values must be finite and >= 0; offending row N"
 * Quantisation.  wmax = the largest entry;  q_e = llrint(ldexp(data_e / wmax, 30)) with IEEE division, round to nearest
 *   even.  wmax == 0, n == 0 or nnz == 0: every vertex is its own community, labels[i] = i, 0 levels, 0 rounds, W2 = 0.
 *   nnz < 2^32 keeps every sum below 2^62.
 * A level has n_l vertices and an int64-weighted CSR; level 0 is the quantised input.  k_i = the sum of row i, diagonal
 *   included;  W2 = the sum of all k_i;  communities start as c[i] = i;  tot[d] = the sum of k_i over the members of d.
 *   Rounds r = 0, 1, .., at most 32 per level; a round reads c and tot as they stood at its start.  For vertex i, a = c[i],
 *   and every community d among c[j] of the row's entries with j != i (an entry with q = 0 counts):
 *       K(d) = the integer sum of those entries' q;  K(a) = 0 if no neighbour is in a;
 *       base(d) = tot[d] - (d == a ? k_i : 0);
 *       p = (double)k_i * (double)base(d);  t = p / (double)W2;  score(d) = fma(-gamma, t, (double)K(d))
 *   -- one multiply, one IEEE division, one fused multiply-add, nothing else contracted.  Vertex i is eligible in round r
 *   when (((uint64)i * 2654435761) >> 16 & 1) == (r & 1) and k_i > 0.  An eligible vertex takes the candidate d != a that
 *   is best by the key (score descending, then d ascending) and moves there iff score(d) > score(a), strictly.  All moves
 *   of a round are applied together.  The level ends after a round without a move, or after round 31.
 * Aggregation.  The communities that still have members are renumbered 0 .. n' - 1 in ascending id; entry (c', d') of the
 *   next level is the integer sum of all entries (i, j) with c[i] -> c' and c[j] -> d' (the diagonal is kept: the row sums
 *   are the old tot); labels is composed through the renumbering.  The algorithm stops when a level made no move, and
 *   after 32 levels.
 * Output.  labels[n] (int32) in [0, C);  stats[4] (int64): C, the levels that moved something, the rounds run in all
 *   (the round without a move that ends a level included), W2 of level 0.
 * n = 0 succeeds, writes stats = 0 and does not read the other pointers; bad arguments fail with a message.  Stateless;
 * device memory that cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: about 60 nnz + 60 n bytes, the sorts' own -- about
 * 16 nnz -- and the aggregated levels, at most 40 nnz).
 * _device: indptr, indices, data and labels are DEVICE pointers on `device`, stats is a HOST pointer; stream as in
 *   schpf_knn_device; synchronised before the call returns.
 * schpf_louvain: host pointers, staged through the device; the same result.
 * schpf_debug_louvain: test hook (host only, no GPU needed): the serial restatement of the definition with std::fma, which
 *   both must match bit for bit. */
int schpf_louvain_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                         double gamma, int32_t *labels, int64_t stats[4]);
int schpf_louvain(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, double gamma,
                  int32_t *labels, int64_t stats[4]);
int schpf_debug_louvain(int n, const int64_t *indptr, const int32_t *indices, const double *data, double gamma,
                        int32_t *labels, int64_t stats[4]);

/* Connected components of a graph: which vertices can reach each other, all integers.
 * Input.  The structure of a CSR matrix n x n: indptr[n + 1] (int64), indices (int32), nnz = indptr[n] < 2^32, 0 <= n < 2^31.
 *   Values are not read.  within: int32[n] or NULL.
 * Edges.  Every stored entry (i, j) with j != i is an UNDIRECTED edge {i, j}: the matrix need not be symmetric (the directed
 *   lists of a k-NN search give the weakly connected components), columns need not ascend and an entry may be stored twice.
 *   With `within`, an entry is an edge only when within[i] == within[j] >= 0; a vertex with within[i] == -1 has no edges.
 *   Refused, the outputs untouched, N the smallest offender, in this order:
 *     "indptr must be 0 at row 0 and must be non-decreasing; offending row N"
 *     "columns must be in [0, n); offending row N"
 *     "components: within must be >= -1; offending vertex N"
 *   and before anything is read: n < 0, nnz >= 2^32, NULL pointers.
 * Output.  comp[n] (int32): the number of components whose smallest vertex is below the smallest vertex of i's component, i.e.
 *   labels 0 .. C - 1 in ascending order of first member.  stats[6] (int64): C; the size of the largest component; the
 *   components of size 1; the entries that were edges; then the hook rounds and the shortcut passes the device ran.  The
 *   last two depend on how the work was scheduled and are OUTSIDE the bit contract (0 from the host restatement);
 *   everything else is one well-defined result, equal bit for bit on every schedule.
 * n = 0 succeeds, writes stats = 0 and does not read the other pointers.  nnz = 0: every vertex is its own component.
 * Stateless; device memory that cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: about 4 nnz + 24 n bytes).
 * _device: indptr, indices, within and comp are DEVICE pointers on `device`, stats is a HOST pointer; stream as in
 *   schpf_knn_device; synchronised before the call returns.
 * schpf_components: host pointers, staged through the device; the same result.
 * schpf_debug_components: test hook (host only, no GPU needed): a serial union-find and the numbering, which both must match
 *   bit for bit on comp and stats[0..3]. */
int schpf_components_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const int32_t *within,
                            int32_t *comp, int64_t stats[6]);
int schpf_components(int device, int n, const int64_t *indptr, const int32_t *indices, const int32_t *within, int32_t *comp,
                     int64_t stats[6]);
int schpf_debug_components(int n, const int64_t *indptr, const int32_t *indices, const int32_t *within, int32_t *comp,
                           int64_t stats[6]);

/* The graph of the clusters: how many entries, and how much of Louvain's integer weight, join every pair of
 * groups of vertices -- the integers behind a PAGA plot.  One aggregation step of schpf_louvain with the caller's labels.
 * Input.  The CSR of schpf_components with data (double; NULL: every entry is 1); labels int32[n] in [-1, G), -1: the vertex
 *   is in no group; G = ngroups >= 1 with G * G < 2^31.  Columns need not ascend.
 *   Refused, the outputs untouched, N the smallest offender, in this order: the indptr and columns messages of
 *   schpf_components, then
 *     "values must be finite and >= 0; offending row N"
 *     "cluster_graph: labels must be in [-1, G); offending vertex N"
 * Output, all int64, row-major, written in full.  group_cells[G]: the vertices of every group.  count[G * G]: count[a * G + b]
 *   = the stored entries (i, j) with j != i, labels[i] = a and labels[j] = b; stored zeros count.  weight[G * G] (may be NULL):
 *   the sum over the same entries of q_e = llrint(ldexp(data_e / wmax, 30)), wmax the largest stored entry; with wmax == 0 or
 *   data == NULL every q_e is 2^30.  *wmax (double, a HOST pointer in all three): the largest stored entry; 1 with data == NULL
 *   and nnz > 0; 0 with nnz == 0.
 * n = 0 succeeds and writes zeros.  Integer sums: equal bit for bit on every schedule.  Scratch: about 52 nnz bytes and the
 *   sort's own.
 * _device: indptr, indices, data, labels, group_cells, count and weight are DEVICE pointers; stream as in schpf_knn_device;
 *   synchronised before the call returns.  schpf_cluster_graph: host pointers.  schpf_debug_cluster_graph: the serial
 *   restatement (host only), which both must match bit for bit. */
int schpf_cluster_graph_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                               const int32_t *labels, int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight,
                               double *wmax);
int schpf_cluster_graph(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, const int32_t *labels,
                        int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight, double *wmax);
int schpf_debug_cluster_graph(int n, const int64_t *indptr, const int32_t *indices, const double *data, const int32_t *labels,
                              int ngroups, int64_t *group_cells, int64_t *count, int64_t *weight, double *wmax);

/* Geodesic distances: the exact shortest-path distance of every vertex from sets of root vertices, walking
 * over the graph -- what a pseudotime, Isomap and Palantir start from.
 * Definition.  For one root set, d is the GREATEST solution of
 *     d[v] = 0 for a root v,    d[v] = min over the edges (u, v) of fl(d[u] + w_uv) otherwise,
 *   fl the IEEE double addition, the minimum of nothing +inf.  Floating-point addition is monotone and no length is negative,
 *   so this is one well-defined set of doubles: Dijkstra ends on it, and so does relaxation of the edges in any order.
 * Input.  The CSR of schpf_cluster_graph: int64 indptr[n + 1], int32 indices, double data; data == NULL: every length is 1
 *   (hop counts).  nnz = indptr[n] < 2^32.  Columns need not ascend, an entry may be stored twice, diagonal entries are
 *   ignored.  A stored entry (i, j, w) is an edge i -> j of length w; with directed == 0 it is also an edge j -> i (SciPy's
 *   directed=False): where both directions are stored with different lengths, the smaller applies by itself.  Lengths must
 *   be finite and >= 0; a stored zero is an edge of length 0.
 *   Root sets.  roots[set_ptr[r] .. set_ptr[r + 1]) (int32, int64 set_ptr[nsets + 1]) is root set r; all its members start
 *   at distance 0: one member per set gives one tree per root, one set of many members the distance to the nearest cell of a
 *   root cluster.  A set may be empty (its row is all +inf); a root may appear in several sets and twice in one.
 *   Refused, the outputs untouched, N the smallest offender, in this order: the indptr and columns messages of
 *   schpf_components, the values message of schpf_cluster_graph, then
 *     "geodesic: set_ptr must be 0 at set 0 and must be non-decreasing; offending set N"
 *     "geodesic: roots must be in [0, n); offending set N"
 *   and before anything is read: n < 0, nsets < 0, nnz >= 2^32, NULL pointers, 8 * nsets * n >= 2^63.
 * Output.  dist[nsets * n] (double), row-major, written in full: dist[r * n + v] is d[v] of root set r, computed with one
 *   IEEE addition per edge and no other arithmetic; +inf: v cannot be reached.  A sum that overflows is +inf, the same as
 *   unreachable.  stats[3] (int64): the finite entries of dist; then the rounds and the lowering writes the device made.  The
 *   last two depend on how the work was scheduled and are OUTSIDE the bit contract (0 from the host restatement);
 *   everything else is one well-defined result, equal bit for bit on every schedule.
 * n == 0 or nsets == 0 succeeds, writes stats = 0 and reads nothing else.
 * Stateless; device memory that cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: 4 nnz + n (8 min(nsets, 8) + 4) bytes,
 *   4 bytes per root and a few words).
 * _device: indptr, indices, data, set_ptr, roots and dist are DEVICE pointers on `device`, stats is a HOST pointer; stream as
 *   in schpf_knn_device; synchronised before the call returns.
 * schpf_geodesic: host pointers, staged through the device; the same result.
 * schpf_debug_geodesic: test hook (host only, no GPU needed): a serial binary-heap Dijkstra per root set, which both must
 *   match bit for bit on dist and stats[0]. */
int schpf_geodesic_device(int device, void *stream, int n, const int64_t *indptr, const int32_t *indices, const double *data,
                          int directed, int nsets, const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3]);
int schpf_geodesic(int device, int n, const int64_t *indptr, const int32_t *indices, const double *data, int directed, int nsets,
                   const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3]);
int schpf_debug_geodesic(int n, const int64_t *indptr, const int32_t *indices, const double *data, int directed, int nsets,
                         const int64_t *set_ptr, const int32_t *roots, double *dist, int64_t stats[3]);

/* Wilcoxon rank sums of every gene for every group of cells: the exact integers behind "which genes mark
 * each cluster".  With average ranks for ties, twice a rank is an integer; every output below is an integer sum, exact in
 * any order, and is equal bit for bit however the work was scheduled.
 * Input.  The count matrix gene-major (CSC of cells x genes), ncells = N cells and ngenes = J genes: indptr[J + 1] (int64),
 *   indices (int32: cell ids, strictly ascending within a gene), data (float32, finite and >= 0; -0.0 counts as 0; stored
 *   zeros are allowed and are zeros like the implicit ones), nnz = indptr[J] < 2^32.  labels[N] (int32) in [-1, G), G =
 *   ngroups: -1 means the cell is ranked with all the others but belongs to no group.  G >= 1, G * J < 2^31 and N < 2^21
 *   (the tie term is a sum of cubes and stays under 2^63); these are refused before anything is read.
 *   Refused, the outputs untouched, M the smallest offending gene (for labels: cell), structure before values, indptr before
 *   the cell ids, the matrix before the labels:
 *     "indptr must be 0 at gene 0 and must be non-decreasing; offending gene M"  (indptr[0] != 0: gene 0; indptr[M + 1] <
 *       indptr[M]: gene M)
 *     "cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene M"
 *     "values must be finite and >= 0; offending gene M"
 *     "labels must be in [-1, ngroups); offending cell M"
 * Definition.  For gene j:  z_j = N minus the number of stored entries with value > 0 -- all the cells that tie at zero.
 *   For a stored entry with value v > 0:  lo = z_j + the number of stored entries of the gene with 0 < value < v;  t = the
 *   number of stored entries of the gene with value == v (float32 equality);  twice the average rank is r2 = 2 lo + t + 1.
 *   Every zero cell has r2 = z_j + 1.
 * Output, all int64.  n[G]: the cells per group.  zeros[J] = z_j.  ties[J] = (z_j^3 - z_j) + the sum over the distinct positive
 *   values of (t^3 - t).  nexpr[G x J], row-major by group: the cells of group g with a positive value in gene j.
 *   rank2[G x J]: the sum of r2 over the cells of group g, zeros included = n_g (z_j + 1) + the sum over the group's positive
 *   entries of (r2 - z_j - 1).  An empty group has zeros in its rows of nexpr and rank2.
 *   (The Mann-Whitney U of group g against the rest is (rank2 - n_g (n_g + 1)) / 2.)
 * N = 0 or J = 0 succeeds and reads no input: every output that is not NULL is written as zeros.  Bad arguments fail with a
 * message.  Stateless; device memory that cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: about 32 nnz bytes and the
 * sort's own, about 12 nnz).
 * _device: indptr, indices, data, labels and the five outputs are DEVICE pointers on `device`; stream as in
 *   schpf_knn_device; synchronised before the call returns.
 * schpf_rank_sums: host pointers, staged through the device; the same result.
 * schpf_debug_rank_sums: test hook (host only, no GPU needed): the serial restatement of the definition, one std::sort per
 *   gene, which both must match bit for bit. */
int schpf_rank_sums_device(int device, void *stream, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices,
                           const float *data, const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties,
                           int64_t *nexpr, int64_t *rank2);
int schpf_rank_sums(int device, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                    const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties, int64_t *nexpr,
                    int64_t *rank2);
int schpf_debug_rank_sums(int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                          const int32_t *labels, int ngroups, int64_t *n, int64_t *zeros, int64_t *ties, int64_t *nexpr,
                          int64_t *rank2);

/* Rank sums between pairs of groups: the exact integers behind "which genes tell cluster a from cluster b" --
 * the Mann-Whitney test of group a against group b alone, for every requested pair and every gene.  Twice a U is an
 * integer; every output below is an integer sum, exact in any order, equal bit for bit however the work was scheduled.
 * Input.  The matrix and the labels as for schpf_rank_sums: indptr[J + 1] (int64), indices (int32 cell ids, strictly
 *   ascending within a gene), data (float32, finite and >= 0; -0.0 and stored zeros are zeros), nnz = indptr[J] < 2^32;
 *   labels[N] (int32) in [-1, G).  pairs[P x 2] (int32, row-major): rows (a, b) with a != b, both in [0, G).  A pair may be
 *   repeated and may appear in both orders; a group may appear in no pair.
 *   N < 2^21, G >= 1, G * J < 2^31, P >= 0 and P * J < 2^31: refused before anything is read.  The refusals of
 *   schpf_rank_sums keep their text and their order; after the labels comes
 *     "pairs must name two different groups in [0, ngroups); offending pair M"  (M the smallest such row)
 *   A refused call leaves the outputs untouched.
 * Definition.  Cells outside the pair do not exist for that pair: cells labelled -1 or in a third group are not ranked
 *   (schpf_rank_sums ranks the -1 cells).  For gene j and group g:  nexpr[g, j] = the cells of g with a positive value,
 *   z_g = n_g - nexpr[g, j].  For a pair (a, b) and a distinct positive value v of gene j:  c_a(v), c_b(v) = the cells of
 *   each group with that value (float32 equality);  below_b(v) = z_b + the cells of b with 0 < value < v.
 * Output, all int64.  n[G]: the cells per group.  nexpr[G x J], row-major by group -- both as schpf_rank_sums gives them.
 *   u2[P x J] = z_a z_b + the sum over v of c_a(v) (2 below_b(v) + c_b(v)): twice the Mann-Whitney U of a over b (twice the
 *   rank sum of a within a ∪ b is u2 + n_a (n_a + 1)).  ties[P x J] = (t_0^3 - t_0) + the sum over v of (t_v^3 - t_v), t_0 =
 *   z_a + z_b, t_v = c_a(v) + c_b(v).  An empty group gives u2 = 0.  u2 of (b, a) is 2 n_a n_b - u2 of (a, b); the ties are
 *   equal.
 * N = 0, J = 0 or P = 0 succeeds; N = 0 or J = 0 reads no input, and every output that is not NULL is written as zeros
 *   where it has a size.  u2 and ties may be NULL when P = 0.  Bad arguments fail with a message.  Stateless; device
 *   memory that cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: 28 nnz + 4 G J + 16 P bytes and the sort's own, about
 *   8 nnz -- O(nnz + G J + P J)).
 * _device: indptr, indices, data, labels, pairs and the four outputs are DEVICE pointers on `device`; stream as in
 *   schpf_knn_device; synchronised before the call returns.
 * schpf_pair_rank_sums: host pointers, staged through the device; the same result.
 * schpf_debug_pair_rank_sums: test hook (host only, no GPU needed): the serial restatement of the definition, one std::sort
 *   per gene and one merge of two lists per pair, which both must match bit for bit. */
int schpf_pair_rank_sums_device(int device, void *stream, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices,
                                const float *data, const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n,
                                int64_t *nexpr, int64_t *u2, int64_t *ties);
int schpf_pair_rank_sums(int device, int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                         const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n, int64_t *nexpr,
                         int64_t *u2, int64_t *ties);
int schpf_debug_pair_rank_sums(int ncells, int ngenes, const int64_t *indptr, const int32_t *indices, const float *data,
                               const int32_t *labels, int ngroups, const int32_t *pairs, int npairs, int64_t *n, int64_t *nexpr,
                               int64_t *u2, int64_t *ties);

/* Pearson residual variance per gene: the two sums behind "which genes vary more than a negative-binomial
 * null explains" (Lause et al. 2021; scanpy's highly_variable_genes(flavor="pearson_residuals")), over ALL N J pairs, zeros
 * included, from the raw counts.
 * Input.  The count matrix gene-major as for schpf_rank_sums, ncells = N cells, ngenes = J genes: indptr[J + 1] (int64),
 *   indices (int32 cell ids, strictly ascending within a gene), data (float32: integer counts in [0, 2^24]; -0.0 is 0; stored
 *   zeros are zeros like the implicit ones), nnz = indptr[J].  inv_theta = 1 / theta >= 0, the inverse of the null's
 *   overdispersion (0: the Poisson null).  clip in (0, inf]: the bound of a residual's size.
 *   Refused before anything is read, in this order:
 *     "hvg: ncells, ngenes and nnz must be in [0, 2^31)"
 *     "hvg: inv_theta must be finite and >= 0"
 *     "hvg: clip must be > 0"  (a NaN is refused)
 *     "hvg: sum and sumsq must not be NULL"  (J > 0)
 *     "hvg: indptr must not be NULL"  (J > 0)
 *     "hvg: indices and data must not be NULL"  (nnz > 0)
 *   then, M the smallest offending gene, structure before values, indptr before the cell ids:
 *     "hvg: indptr must be 0 at gene 0, must be non-decreasing and must end at nnz; offending gene M"  (indptr[0] != 0: gene 0;
 *       indptr[M + 1] < indptr[M]: gene M; indptr[J] != nnz: gene J - 1; J = 0 with nnz != 0: gene 0)
 *     "hvg: cell ids must be in [0, ncells) and strictly ascending within a gene; offending gene M"
 *     "hvg: values must be integer counts in [0, 2^24]; offending gene M"  (a fraction, a negative, a denormal, inf, nan)
 *   A refused call leaves the outputs untouched.  No input aborts.
 * Definition, all arithmetic in double.  n_c = the total of cell c, s_g = the total of gene g, T = the total of all, exact
 *   in int64.  q_g = (double)s_g / (double)T,  mu_cg = (double)n_c * q_g,
 *     r_cg = min(clip, max(-clip, (x_cg - mu_cg) / sqrt(mu_cg (1 + mu_cg inv_theta)))),   r_cg = 0 where mu_cg = 0
 *   (a gene or a cell without counts, T = 0).  S1_g = the sum of r_cg over all N cells, S2_g = the sum of r_cg^2.  The
 *   variance of the residuals of gene g (ddof = 0) is S2_g / N - (S1_g / N)^2.
 * Output.  sum[J] = S1, sumsq[J] = S2 (double).  Optional, skipped when NULL: cell_total[N] = n_c, gene_total[J] = s_g (int64).
 * How it is summed.  A zero entry's residual z(mu) = -min(clip, sqrt(mu / (1 + mu inv_theta))) depends on the cell only through
 *   n_c:  S1_g = the sum over the distinct cell totals u, m_u cells each, of m_u z(u q_g)  +  the sum over the stored
 *   entries with x > 0 of r_cg - z(mu_cg);  S2_g likewise with squares.  There are no floating-point atomics and the order of
 *   every sum is fixed by the input alone: two calls, two streams, host or device pointers give the same bits.  The first
 *   part sees only the multiset of the cell totals and does not change by a bit when the cells are renumbered.  The second
 *   part adds a gene's entries in an order fixed by their position in the gene's segment: it is NOT invariant under a
 *   renumbering of the cells, which moves the sums by rounding only.  Against the definition summed in double, |S1 - exact|
 *   <= 4 N 2^-53 * the sum of |r_cg| and |S2 - exact| <= 4 N 2^-53 S2 (tests/test_residual_var_gpu.py).
 * N = 0 or J = 0 or nnz = 0 succeeds: every output that is not NULL is written as zeros.  Stateless; device memory that
 *   cannot be had returns SCHPF_ERR_NO_MEMORY (scratch: 4 nnz bytes during the checks, then 44 N + 8 J and the sort's own).
 * _device: indptr, indices, data and the outputs are DEVICE pointers on `device`; stream as in schpf_thin_counts_device;
 *   synchronised before the call returns.
 * schpf_residual_var: host pointers, staged through the device; the same bits.
 * schpf_debug_residual_var: test hook (host only, no GPU needed): the definition walked serially over all N cells of every
 *   gene, with the same refusals.  It knows nothing of the split and is not bit-equal to the device: both are held to the
 *   bound above. */
int schpf_residual_var_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr,
                              const int32_t *indices, const float *data, double inv_theta, double clip, double *sum, double *sumsq,
                              int64_t *cell_total, int64_t *gene_total);
int schpf_residual_var(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                       const float *data, double inv_theta, double clip, double *sum, double *sumsq, int64_t *cell_total,
                       int64_t *gene_total);
int schpf_debug_residual_var(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                             const float *data, double inv_theta, double clip, double *sum, double *sumsq, int64_t *cell_total,
                             int64_t *gene_total);

/* Simulated doublets: rows that are the sum of two observed cells, the first step of Scrublet's doublet
 * score.  Integer work whose result is fully determined: every schedule gives the same bits.
 * Parents.  Simulated row s has the parents (a, b):  w = philox4x32_10(counter (s & 0xffffffff, s >> 32, 0, 1), key (low,
 *   high word of seed));  a = (uint64(w[0]) * ncells) >> 32,  b = (uint64(w[1]) * ncells) >> 32.  Thinning's counters end in
 *   0, so one seed gives unrelated streams.  a == b is allowed.  The draw depends on (seed, ncells, s) alone.
 *   parents: int32[n_sim, 2], the rows s = first, first + 1, ..., first + n_sim - 1.  first >= 0, 0 <= n_sim < 2^31,
 *   0 < ncells < 2^31.  schpf_doublet_parents is host only and needs no GPU; _device writes the same bits to DEVICE memory
 *   from a kernel (stream as in schpf_thin_counts_device; synchronised before the call returns).
 * Sum of a pair.  Input: a CSR matrix of ncells x ngenes with nnz stored entries, the columns strictly ascending within a
 *   row (canonical, no duplicates), every value a non-negative integer <= 2^24 (what thinning accepts); parents int32[n_pairs,
 *   2].  Row s of the result holds one entry for every column stored in parent a or in parent b, columns ascending, the value
 *   the sum of the stored values as int32; a column stored in either parent is stored in the result even where the sum is 0,
 *   so the structure depends on the indices alone.  out_indptr int64[n_pairs + 1], out_indices int32, out_values int32.
 *   With out_indices == NULL and out_values == NULL only out_indptr is written: the caller reads out_indptr[n_pairs],
 *   allocates, and calls again with capacity = the entries the two arrays hold; capacity < out_indptr[n_pairs] is refused
 *   ("capacity must be at least ..."; the outputs are then unspecified).
 *   Refused before anything is written, M the smallest offender, in this order:
 *     "doublets: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row M"  (indptr[ncells] !=
 *       nnz: row ncells)
 *     "doublets: column index out of range at entry M"  (outside [0, ngenes), or an int64 beyond int32)
 *     "doublets: columns must be strictly ascending within a row; offending row M"
 *     "doublets: values must be integer counts in [0, 2^24]; offending entry M"
 *     "doublets: parents must be in [0, ncells); offending pair M"
 *   n_pairs == 0 or nnz == 0 succeeds without reading any input: out_indptr, where given, is written as zeros.  Sizes
 *   outside [0, 2^31) and NULL pointers otherwise are refused.
 * _device: indptr (of indptr_kind), indices (of idx_kind: SCHPF_IDX_*), val (of val_kind), parents and the outputs are DEVICE
 *   pointers on `device`, read and written in place; stream as in schpf_thin_counts_device; synchronised before the call
 *   returns.  Scratch: 8 (n_pairs + 1) bytes and the scan's own.
 * schpf_doublet_rows: host pointers (int64 indptr, int32 indices), staged through the device; the same result.
 * schpf_debug_doublet_rows: test hook (host only, no GPU needed): the serial restatement, a two-pointer merge per pair, which
 *   both must match bit for bit. */
int schpf_doublet_parents(int64_t first, int64_t n_sim, int64_t ncells, uint64_t seed, int32_t *parents);
int schpf_doublet_parents_device(int device, void *stream, int64_t first, int64_t n_sim, int64_t ncells, uint64_t seed,
                                 int32_t *parents);
int schpf_doublet_rows_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                              int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int64_t n_pairs,
                              const int32_t *parents, int64_t *out_indptr, int32_t *out_indices, int32_t *out_values,
                              int64_t capacity);
int schpf_doublet_rows(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                       const void *val, int val_kind, int64_t n_pairs, const int32_t *parents, int64_t *out_indptr,
                       int32_t *out_indices, int32_t *out_values, int64_t capacity);
int schpf_debug_doublet_rows(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                             const void *val, int val_kind, int64_t n_pairs, const int32_t *parents, int64_t *out_indptr,
                             int32_t *out_indices, int32_t *out_values, int64_t capacity);

/* Cell and gene filtering: the sums a quality filter asks of a count matrix, and X[rows][:, kept genes].
 * Integer work whose result is fully determined: every schedule gives the same bits.
 * Axis statistics.  Input: a CSR matrix of ncells x ngenes with nnz stored entries, as schpf_doublet_rows takes it: indptr 0 at
 *   row 0, non-decreasing, ending at nnz; the columns in [0, ngenes) and strictly ascending within a row; every value an
 *   integer count in [0, 2^24].  gene_flags uint32[ngenes]: bit s is set where gene j belongs to gene set s, 0 <= n_sets <= 32;
 *   with n_sets == 0, gene_flags and cell_set_total may be NULL.  All outputs int64:
 *     cell_n[i]      the stored entries of row i with a value > 0 (a stored zero is no expression)
 *     cell_total[i]  their sum
 *     cell_set_total[s * ncells + i]  the sum of the entries of row i whose gene has bit s
 *     gene_n[j], gene_total[j]  the same per column;  gene_sumsq[j]  the sum of the squared values of column j
 *   Totals stay below 2^55.  Refused before anything is written, M the smallest offender, in this order:
 *     "qc: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row M"
 *     "qc: column index out of range at entry M"
 *     "qc: columns must be strictly ascending within a row; offending row M"
 *     "qc: values must be integer counts in [0, 2^24]; offending entry M"
 *     "qc: sum of squares may overflow: largest value M over N cells"  (M the largest stored value, M^2 * ncells >= 2^63)
 *   nnz == 0 succeeds without reading the matrix: the outputs are zeros.  Sizes outside [0, 2^31), n_sets outside [0, 32],
 *   unknown kinds and NULL pointers otherwise are refused.
 * Submatrix.  Input: a CSR matrix with indptr as above and the columns in [0, ngenes); no order within a row is asked,
 *   duplicates may occur, and the values are not interpreted.  rows int32[n_rows]: row numbers in [0, ncells), in any order,
 *   repeats allowed; NULL: the rows 0 .. ncells - 1, and n_rows must be ncells.  gene_keep uint8[ngenes]: gene j is kept where
 *   gene_keep[j] != 0; NULL keeps every gene.  The kept genes are renumbered in ascending order; *out_ngenes (a HOST pointer
 *   in all three entry points) is their number.  Row r of the result holds the entries of row rows[r] whose gene is kept, in
 *   their stored order, the columns renumbered, the bytes of the values unchanged (-0.0, NaN payloads and stored zeros
 *   survive).  out_indptr int64[n_rows + 1], out_indices int32, out_values of val_kind.  With out_indices == NULL and
 *   out_values == NULL only *out_ngenes and out_indptr are written: the caller reads out_indptr[n_rows], allocates, and calls
 *   again with capacity = the entries the two arrays hold.  Every call validates afresh.
 *   Refused before anything is written, M the smallest offender, in this order: the indptr and the column range as above,
 *     "qc: rows must be in [0, ncells); offending position M"
 *     "capacity must be at least the T entries of the result, got C"
 *   nnz == 0 or n_rows == 0: the matrix is not read and out_indptr is zeros; gene_keep is still counted and rows checked.
 * _device: indptr (of indptr_kind), indices (of idx_kind: SCHPF_IDX_*), val (of val_kind), gene_flags, rows, gene_keep and the
 *   outputs but out_ngenes are DEVICE pointers on `device`, read and written in place; stream as in
 *   schpf_thin_counts_device; synchronised before the call returns.  Scratch: the submatrix 16 (n_rows + 1) + 8 (ngenes + 1)
 *   bytes and the scans' own, the statistics a few words.
 * schpf_axis_stats, schpf_submatrix: host pointers (int64 indptr, int32 indices), staged through the device; the same result.
 * schpf_debug_axis_stats, schpf_debug_submatrix: test hooks (host only, no GPU needed): the serial restatements, one entry
 *   after the other, which the others must match bit for bit. */
int schpf_axis_stats_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                            int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int n_sets,
                            const uint32_t *gene_flags, int64_t *cell_n, int64_t *cell_total, int64_t *cell_set_total,
                            int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq);
int schpf_axis_stats(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                     const void *val, int val_kind, int n_sets, const uint32_t *gene_flags, int64_t *cell_n, int64_t *cell_total,
                     int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq);
int schpf_debug_axis_stats(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                           const void *val, int val_kind, int n_sets, const uint32_t *gene_flags, int64_t *cell_n,
                           int64_t *cell_total, int64_t *cell_set_total, int64_t *gene_n, int64_t *gene_total, int64_t *gene_sumsq);
int schpf_submatrix_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                           int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int64_t n_rows,
                           const int32_t *rows, const uint8_t *gene_keep, int64_t *out_ngenes, int64_t *out_indptr,
                           int32_t *out_indices, void *out_values, int64_t capacity);
int schpf_submatrix(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                    const void *val, int val_kind, int64_t n_rows, const int32_t *rows, const uint8_t *gene_keep,
                    int64_t *out_ngenes, int64_t *out_indptr, int32_t *out_indices, void *out_values, int64_t capacity);
int schpf_debug_submatrix(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                          const void *val, int val_kind, int64_t n_rows, const int32_t *rows, const uint8_t *gene_keep,
                          int64_t *out_ngenes, int64_t *out_indptr, int32_t *out_indices, void *out_values, int64_t capacity);

/* Pseudobulk: per group of cells and gene, the cells that express the gene, the sum of their counts and the
 * sum of the squares.  Integer work whose result is fully determined: every schedule gives the same bits.
 * Input: the canonical count CSR that schpf_axis_stats takes -- indptr 0 at row 0, non-decreasing, ending at nnz; the columns
 *   in [0, ngenes) and strictly ascending within a row; every value an integer count in [0, 2^24]; a stored zero counts as a
 *   zero.  labels int32[ncells] in [-1, ngroups): the group of every cell, -1 for a cell in no group.  ngroups >= 1.
 *   All outputs int64, row-major, written in full (zeros where nothing falls):
 *     group_cells[g]            the cells with label g
 *     nexpr[g * ngenes + j]     the cells of group g whose entry of gene j is > 0
 *     total[g * ngenes + j]     the sum of those entries
 *     sumsq[g * ngenes + j]     the sum of their squares; sumsq may be NULL: then it is neither computed nor checked for overflow
 *   Refused before anything is written, M the smallest offender, in this order:
 *     "group_stats: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row M"
 *     "group_stats: column index out of range at entry M"
 *     "group_stats: columns must be strictly ascending within a row; offending row M"
 *     "group_stats: values must be integer counts in [0, 2^24]; offending entry M"
 *     "group_stats: labels must be in [-1, ngroups); offending cell M"
 *     "group_stats: sum of squares may overflow: largest value M over N cells"  (where sumsq is given; M the largest stored
 *       value, M^2 * ncells >= 2^63: a group holds at most ncells cells)
 *   nnz == 0 succeeds without reading the matrix: the labels are still checked, group_cells is counted, the rest is zeros.
 *   Sizes outside [0, 2^31), ngroups outside [1, 2^31), ngroups * ngenes >= 2^31, unknown kinds and NULL pointers otherwise
 *   are refused.
 * _device: indptr (of indptr_kind), indices (of idx_kind: SCHPF_IDX_*), val (of val_kind), labels and the outputs are DEVICE
 *   pointers on `device`, read and written in place; stream as in schpf_thin_counts_device; synchronised before the call
 *   returns.  Scratch: 16 ncells + 24 (ngroups + 1) bytes, 12 bytes per slab of 2048 cells of one group (at most
 *   ncells / 2048 + min(ngroups, ncells) slabs), the radix sort's and the scan's own, and a few words.
 * schpf_group_stats: host pointers (int64 indptr, int32 indices), staged through the device; the same result.
 * schpf_debug_group_stats: test hook (host only, no GPU needed): the serial restatement, one entry after the other, which
 *   the others must match bit for bit. */
int schpf_group_stats_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                             int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind,
                             const int32_t *labels, int64_t ngroups, int64_t *group_cells, int64_t *nexpr, int64_t *total,
                             int64_t *sumsq);
int schpf_group_stats(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                      const void *val, int val_kind, const int32_t *labels, int64_t ngroups, int64_t *group_cells,
                      int64_t *nexpr, int64_t *total, int64_t *sumsq);
int schpf_debug_group_stats(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                            const void *val, int val_kind, const int32_t *labels, int64_t ngroups, int64_t *group_cells,
                            int64_t *nexpr, int64_t *total, int64_t *sumsq);

/* Gene-major form of a count matrix: an exact sparse transpose, the CSC arrays that schpf_rank_sums,
 * schpf_pair_rank_sums and schpf_residual_var take, from the CSR that everything upstream produces.  Integer work whose
 * result is fully determined: every schedule gives the same bits.
 * Input: a CSR matrix of ncells x ngenes with nnz stored entries, as schpf_axis_stats takes it: indptr 0 at row 0,
 *   non-decreasing, ending at nnz; the columns in [0, ngenes) and strictly ascending within a row.  The values are not
 *   interpreted.  out_val_kind is val_kind -- the bytes of every value are moved unchanged (-0.0, NaN payloads and stored
 *   zeros survive, as in schpf_submatrix) -- or SCHPF_VAL_F32: the value is (float) of the double that the input value
 *   converts to, exact for counts up to 2^24.
 * Output: out_indptr int64[ngenes + 1], out_cells int32[nnz], out_values [nnz] of out_val_kind: the CSC form of the same
 *   matrix.  Gene j's entries lie at [out_indptr[j], out_indptr[j + 1]), the cells ascending: entry (i, j) stands at
 *   out_indptr[j] + #{stored (i', j) : i' < i}.  out_source int64[nnz], skipped when NULL: the stored position in the input
 *   of every output entry, with which a caller carries a second value array across without a second transpose.
 *   Refused before anything is written, M the smallest offender, in this order:
 *     "transpose: indptr must be 0 at row 0, must be non-decreasing and must end at nnz; offending row M"
 *     "transpose: column index out of range at entry M"
 *     "transpose: columns must be strictly ascending within a row; offending row M"
 *   nnz == 0, ncells == 0 or ngenes == 0 succeeds without reading the matrix: out_indptr is zeros.  Sizes outside [0, 2^31),
 *   unknown kinds, an out_val_kind that is neither val_kind nor SCHPF_VAL_F32 and NULL pointers otherwise (out_indptr
 *   always) are refused before anything is read.
 * _device: indptr (of indptr_kind), indices (of idx_kind: SCHPF_IDX_*), val (of val_kind) and the outputs are DEVICE pointers
 *   on `device`, read and written in place; stream as in schpf_thin_counts_device; synchronised before the call returns.
 *   Scratch: a table of 4 ngenes bytes per slab of 2048 rows (4 ngenes ceil(ncells / 2048) bytes: 49 MB at 1M x 25 000),
 *   8 (ngenes + 1) bytes, the scan's own and a few words.
 * schpf_transpose: host pointers (int64 indptr, int32 indices), staged through the device; the same result.
 * schpf_debug_transpose: test hook (host only, no GPU needed): a serial counting transpose, one entry after the other, which
 *   the others must match bit for bit. */
int schpf_transpose_device(int device, void *stream, int64_t ncells, int64_t ngenes, int64_t nnz, const void *indptr,
                           int indptr_kind, const void *indices, int idx_kind, const void *val, int val_kind, int out_val_kind,
                           int64_t *out_indptr, int32_t *out_cells, void *out_values, int64_t *out_source);
int schpf_transpose(int device, int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                    const void *val, int val_kind, int out_val_kind, int64_t *out_indptr, int32_t *out_cells, void *out_values,
                    int64_t *out_source);
int schpf_debug_transpose(int64_t ncells, int64_t ngenes, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                          const void *val, int val_kind, int out_val_kind, int64_t *out_indptr, int32_t *out_cells,
                          void *out_values, int64_t *out_source);

/* Test hooks of the fused Gamma update (kernels.hip gamma_update_kernel; both need a GPU).
 * schpf_debug_special: one function of csrc/special.h per element, evaluated on the DEVICE by one thread per element
 *   through the inline bodies the update kernel calls: out[i] = fast_rcp(x[i]), fast_log(x[i]), fast_exp(x[i]),
 *   digamma(x[i]) or digamma_less_log(x[i], fast_rcp(y[i])) (= psi(shape x) - log(rate y), as the kernel pairs them).
 *   Host arrays of n doubles; y is read by SCHPF_SPECIAL_PSI_LESS_LOG only and may be NULL otherwise.  n = 0 succeeds.
 * schpf_debug_tables: the three [n, KP] tables of one side (SCHPF_BY_CELL: theta's, SCHPF_BY_GENE: beta's; KP =
 *   schpf_plan_info()[0], columns k >= nfactors are padding) copied to the host in the engine's dtype: tab_e = shape /
 *   rate, tab_log = psi(shape) - log(rate), tab_exp = exp(tab_log - float(row max of tab_log)).  Tables older than
 *   the parameters are rebuilt first, as the next schpf_step or schpf_loss_terms would; nothing else changes.  Any of the
 *   three pointers may be NULL. */
#define SCHPF_SPECIAL_RCP 0
#define SCHPF_SPECIAL_LOG 1
#define SCHPF_SPECIAL_EXP 2
#define SCHPF_SPECIAL_PSI 3
#define SCHPF_SPECIAL_PSI_LESS_LOG 4
int schpf_debug_special(int which, int64_t n, const double *x, const double *y, double *out);
int schpf_debug_tables(schpf_ctx *ctx, int side, void *tab_e, void *tab_log, void *tab_exp);

/* Test hook (host only, no GPU needed): build one sweep plan from (major, minor, val) and expand
 * it back into per-nonzero records in storage order -- the major/minor/val it will be processed
 * with, the partials row (natural chunk id) it accumulates into and the wavefront that streams
 * it -- plus cptr[n_major + 1] and stats = {n_chunks, n_slices, n_waves, stored entry slots}. */
int schpf_debug_plan_expand(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val,
                            int n_major, int n_minor, int lpc, int chunk_len, int n_windows,
                            int32_t *out_major, int32_t *out_minor, float *out_val,
                            int32_t *out_natid, int32_t *out_wave, int32_t *out_cptr,
                            int64_t stats[4]);

/* Same for the tile plan (LDS-staged sweep): per stored nonzero the major/minor/val, the partial
 * row (task * groups_per_block + group) it accumulates into and its task; pfirst/pcount[n_major];
 * stats = {n_tasks, n_blocks, n_windows, pstride, stored entry slots, windows_per_task, LDS passes that read a
 * row, extra LDS cycles of those passes under the bank model of plan.cpp (rows of one class are serialised)};
 * $SCHPF_BANK_ORDER picks the order inside a segment (plan.h TileShape::bank_order).
 * ring <= 1: window schedule with win_rows rows per window; ring <= -2: the half-window schedule with
 * -ring slots of slot_bytes (a multiple of 16; table rows are 160 bytes here) -- the hook then also
 * checks that every entry of an epoch points into a slot readable in that epoch. */
int schpf_debug_tile_expand(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val,
                            int n_major, int n_minor, int lpc, int waves_per_block, int win_rows,
                            int target_tasks, int ring, int slot_bytes, int32_t *out_major,
                            int32_t *out_minor, float *out_val, int32_t *out_prow, int32_t *out_task,
                            int32_t *out_pfirst, int32_t *out_pcount, int64_t stats[8]);

/* Test hook (host only, no GPU needed): the half (0 / 1) of its step slot in which a window-schedule tile plan, built
 * as by schpf_debug_tile_expand (160-byte table rows, $SCHPF_BANK_ORDER), stores every nonzero; out_* have nnz
 * entries, in the kernel's walk order.  The float64 sweep with two lanes per row divides for the first half of a slot
 * in the even lane and for the second in the odd one. */
int schpf_debug_tile_halves(int64_t nnz, const int32_t *major, const int32_t *minor, const float *val, int n_major,
                            int n_minor, int lpc, int waves_per_block, int win_rows, int target_tasks,
                            int32_t *out_major, int32_t *out_minor, int32_t *out_half);

/* Test hook (host only, no GPU needed, no environment read): the sweep shape an engine of `dtype` with `nfactors`
 * factors runs on -- the library's own choice (policy.cpp choose_config) under plan = 0 (the library picks the plan),
 * 1 (the tile plan forced, SCHPF_PLAN=tile) or 2 (the gather plan forced).  out = {1 tile / 0 gather, LPC (lanes per
 * row), NV (16-byte vectors per lane), KL (values per lane), KP (padded row length)}.  Fails with the library's
 * message where nfactors is outside [1, 256] or no instantiated shape fits. */
int schpf_debug_choose_config(int dtype, int nfactors, int plan, int out[5]);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* SCHPF_HIP_H */
