// Planning policy (policy.h): the switches, and the decisions that turn an engine's shape and matrix into plan shapes.
#include "policy.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>

#include "kernels.h"

namespace schpf {

Tuning tuning_from_env()
{
    auto set = [](const char *name) -> const char * {
        const char *s = getenv(name);
        return s && *s ? s : nullptr;
    };
    auto num = [&](const char *name, int dflt) { const char *s = set(name); return s ? atoi(s) : dflt; };
    Tuning t;
    if (const char *pk = set("SCHPF_PLAN")) {
        if (!strcmp(pk, "gather")) t.plan = Tuning::PLAN_GATHER;
        if (!strcmp(pk, "tile")) t.plan = Tuning::PLAN_TILE;
    }
    t.half = num("SCHPF_HALF", -1);
    t.balance = num("SCHPF_BALANCE", -1);
    t.wpb = num("SCHPF_WPB", 0);
    if (const char *s = set("SCHPF_TASKS")) t.tasks = atoi(s);
    if (const char *s = set("SCHPF_TAPER")) t.taper = atoi(s);
    t.bank_order = num("SCHPF_BANK_ORDER", 2);
    t.dual = num("SCHPF_DUAL", 1) != 0;
    t.persistent = num("SCHPF_PERSISTENT", 1) != 0;
    t.device_plan = num("SCHPF_DEVICE_PLAN", 1) != 0;
    t.loss_side = num("SCHPF_LOSS_SIDE", -1);
    t.loss_split = num("SCHPF_LOSS_SPLIT", 1) != 0;
    t.fuse_sums = num("SCHPF_FUSE_SUMS", 1) != 0;
    t.graph = num("SCHPF_GRAPH", 1) != 0;
    if (const char *s = set("SCHPF_GRAPH_SHARDED")) t.graph_sharded = atoi(s) != 0;
    t.verbose = num("SCHPF_VERBOSE", 0) != 0;
    t.debug_row_slots = num("SCHPF_DEBUG_ROW_SLOTS", 10);
    t.debug_single = num("SCHPF_DEBUG_SINGLE", 0) != 0;
    t.debug_balance = num("SCHPF_DEBUG_BALANCE", 0) != 0;
    return t;
}

// Row layout of the tables the sweeps read: KP = NV * LPC * VEC values (VEC = values per 16 B);
// a group of LPC lanes shares one row, lane `sub` holding the 16-byte vectors q*LPC + sub.
//  * tile plan (LDS-staged): VALU work per nonzero has a fixed part (reciprocal, cross-lane
//    sum, addressing) that every lane of the group repeats, so rows are split over as FEW
//    lanes as the register budget allows: the smallest LPC with <= 112 row bytes per lane
//    (measured on C3: f64 K=20 -> LPC 2, f32 K=20 -> LPC 1; profiles/r01/explore*.log);
//  * gather plan (L2): the L1 path is charged per 64-byte sector touched, so the cost model
//    is accesses per nonzero = NV * max(1, LPC/4) and LPC = 4 usually wins.
Config choose_config(int K, int elem, const Tuning &tn)
{
    if (K < 1 || K > 256) throw std::invalid_argument("nfactors must be in [1, 256]");
    const int vec = 16 / elem;
    const int nvec = (K + vec - 1) / vec;
    static const int nv_ok[] = {1, 2, 3, 4, 5, 6, 7, 8, 10};
    bool tile = (size_t)nvec * 16 <= 1024;          // at least ~150 rows per 152 KiB window
    if (tn.plan == Tuning::PLAN_GATHER) tile = false;
    if (tn.plan == Tuning::PLAN_TILE) tile = true;
    int best_lpc = 0, best_nv = 0, best_cost = 1 << 30;
    static const int order_tile[] = {1, 2, 4, 8, 16};
    static const int order_gather[] = {4, 8, 2, 16, 1};
    for (int lpc : (tile ? order_tile : order_gather)) {
        const int need = (nvec + lpc - 1) / lpc;
        int nv = 0;
        for (int v : nv_ok) if (v >= need) { nv = v; break; }
        if (!nv || (tile && nv > 7)) continue;           // the tile sweeps are instantiated for <= 7 vectors
        const int cost = tile ? (nv * 16 <= 112 ? 0 : 1 << 20)   // first that fits
                              : nv * std::max(1, lpc / 4);
        // only instantiated pairs (kernels.h)
        if (!(tile ? tile_combo_ok(nv, lpc) : gather_combo_ok(nv, lpc))) continue;
        if (cost < best_cost) { best_cost = cost; best_lpc = lpc; best_nv = nv; }
    }
    if (!best_lpc) throw std::invalid_argument("no instantiated sweep shape fits nfactors (kernels.h tile_combo_ok / "
                                               "gather_combo_ok)");
    const int KL = best_nv * vec;
    return {tile, best_lpc, best_nv, KL, KL * best_lpc};
}

// Windows of a gather plan: the minor table cut in halves until a window's rows fit 2 MiB.
int pick_windows(size_t table_bytes)
{
    const size_t budget = (size_t)2048 * 1024;
    int w = 1;
    while ((table_bytes + w - 1) / w > budget && w < 4096) w *= 2;
    return w;
}

// workgroups of a tile sweep that fit a compute unit at once.  Sized by the LOSS pass's LDS (window + the 1 KiB
// logarithm table behind it, run_sweep): the PHI and LLH launches of a plan must agree on the residency
int per_cu(size_t window_lds_bytes) { return window_lds_bytes + 1024 > 80 * 1024 ? 1 : 2; }

// Workgroup shape of the tile sweep.  One 1024-thread workgroup per CU with a 152 KiB window
// (fewest stagings, longest row segments => least sliced-ELL padding) unless that leaves fewer
// than 256 (block, window) pairs per orientation; then the workgroup is halved (64 KiB windows,
// two or more workgroups per CU) until there are, down to 256 threads.  Measured with the graph /
// persistent launches of round 2 (profiles/r02/explore_c2_shapes.log): C2 (10k x 5k) 256-thread
// workgroups 24.6 k -> 26.7 k it/s in f64, -4 % per iteration in f32 (128 threads: +5 %, hence the
// floor); a 1/8 shard of C3 keeps the large workgroup in f64 (525 pairs) and halves it in f32 (-3 %).
void pick_workgroup(const Problem &p, const Tuning &tn, int n_major, int n_minor, int &wpb, int &lds_kb)
{
    wpb = tn.wpb;
    const size_t row_bytes = (size_t)p.KP * p.elem;
    if (!wpb) {
        wpb = 16;
        for (;;) {
            const int kb = wpb >= 12 ? 152 : 64;
            const int64_t wr = std::max<int64_t>(1, (int64_t)kb * 1024 / (int64_t)row_bytes);
            const int64_t blocks = ((int64_t)n_major + (64 / p.LPC) * wpb - 1) / ((64 / p.LPC) * wpb);
            const int64_t windows = ((int64_t)n_minor + wr - 1) / wr;
            if (blocks * windows >= 256 || wpb <= 4) break;
            wpb /= 2;
        }
    }
    lds_kb = wpb >= 12 ? 152 : 64;
}

// Task ranges of both orientations of the one-launch iteration from the list-schedule model of
// plan.h choose_task_ranges (big problems with the 1024-thread workgroup on both sides; knobs that fix
// task counts or schedules by hand switch it off).  Constants from C3 on an MI355X: a workgroup works
// through ~1.7e11 / (K sizeof(T)) nonzeros per second (K = 20: 1.06e9 f64, 2.1e9 f32; measured 1.07 /
// 1.9), a partial row is written and read back at ~3.5 TB/s, a task costs 3 us beside its nonzeros
// (swept 2-16: 2-4 pick one range per cell block and 18 per gene block at C3 f64, the
// fastest measured).  Against the former fixed counts (profiles/r02/explore_task_ranges.log), per
// iteration: C3 f64 (6, 13) -> (1, 18) ranges -2.4 %, C3 f32 (3, 13) -> (3, 11) -3.3 %, half of C3's
// cells -7.5 %, a quarter -3 %, the C5 share -1..2 % (f64) / -4 % (f32).
bool choose_ranges(const Problem &p, const Tuning &tn, const SampleHistograms &sample, int ranges[2], int half[2])
{
    if (!p.expect_sharded && !tn.dual) return false;
    if (tn.tasks || tn.half >= 2) return false;
    const size_t row_bytes = (size_t)p.KP * p.elem;
    const int n_maj[2] = {p.N, p.G}, n_min[2] = {p.G, p.N};
    int64_t blocks[2], half_windows[2];
    bool half_ok[2];
    double partial_seconds[2];
    int wpb[2];
    for (int s = 0; s < 2; ++s) {
        int lds_kb;
        pick_workgroup(p, tn, n_maj[s], n_min[s], wpb[s], lds_kb);
        if (wpb[s] < 12) return false;
        const int64_t half_rows = ((int64_t)lds_kb * 512 - 64) / (int64_t)row_bytes;
        if (half_rows < 1) return false;
        blocks[s] = ((int64_t)n_maj[s] + (64 / p.LPC) * wpb[s] - 1) / ((64 / p.LPC) * wpb[s]);
        half_windows[s] = ((int64_t)n_min[s] + half_rows - 1) / half_rows;
        const double per_row = (double)p.nnz / std::max(1, n_maj[s]) * (double)half_rows / std::max(1, n_min[s]);
        half_ok[s] = tn.half != 0 && per_row >= 16.0 && !p.balance_now;
        partial_seconds[s] = 2.0 * (double)n_maj[s] * (double)row_bytes / 3.5e12;
    }
    const int resident = p.cu_count;
    // only where a launch is several rounds of workgroups (1/8 of C3: -4 % in one launch, +-0 in two): smaller
    // problems keep the rules of tile_shape
    if (blocks[0] * half_windows[0] + blocks[1] * half_windows[1] < 6 * (int64_t)resident) return false;
    // where the nonzeros sit: a skewed matrix has heavy blocks (the planted benchmark matrix: one range per
    // cell block -- the uniform model's choice -- doubles the iteration, its heaviest block runs last)
    // the blocks the plans will cut: rows per block follow the workgroup (a forced SCHPF_WPB=12 has 12 waves)
    const int64_t stride = std::max<int64_t>(1, p.nnz / 4000000);   // ~4 M samples per orientation: a few ms
    std::vector<int32_t> hist[2];
    sample(stride, hist);
    const std::vector<double> share[2] = {block_shares(hist[0], (64 / p.LPC) * wpb[0]),
                                          block_shares(hist[1], (64 / p.LPC) * wpb[1])};
    const RangeChoice c = choose_task_ranges(blocks, half_windows, half_ok, share, (double)p.nnz, resident,
                                             1.7e11 / ((double)p.K * p.elem), 1e-6 * 3, partial_seconds,
                                             p.expect_sharded ? 4 : 6, p.balance_now ? 1.0 : 1.12, 32, p.expect_sharded,
                                             tn.taper.value_or(30) / 100.0);
    if (c.ranges[0] <= 0 || c.ranges[1] <= 0) return false;
    for (int s = 0; s < 2; ++s) { ranges[s] = c.ranges[s]; half[s] = c.half[s] ? 1 : 0; }
    if (tn.verbose)
        fprintf(stderr, "[schpf_hip]   task ranges from the list-schedule model: cell %d (%s), gene %d (%s), %.3f ms\n",
                ranges[0], half[0] ? "half windows" : "windows", ranges[1], half[1] ? "half windows" : "windows",
                c.seconds * 1e3);
    return true;
}

TileShape tile_shape(const Problem &p, const Tuning &tn, int n_major, int n_minor, int ranges, int force_half)
{
    int wpb, lds_kb;
    pick_workgroup(p, tn, n_major, n_minor, wpb, lds_kb);
    const size_t row_bytes = (size_t)p.KP * p.elem;
    TileShape sh;
    sh.lpc = p.LPC;
    sh.waves_per_block = wpb;
    sh.row_slots = (int)(row_bytes / 16);
    sh.bank_order = tn.bank_order;   // 0 minor order, 1 per row, 2 jointly per LDS pass (plan.h)
    sh.taper = tn.taper.value_or(30) / 100.0;   // window ranges of unequal length (plan.h tile_range_starts), per cent
    sh.verbose = tn.verbose;
    sh.win_rows = (int)std::max<size_t>(1, (size_t)lds_kb * 1024 / row_bytes);
    // tasks per orientation: a few rounds of the 256 CUs for big problems; about one round when
    // there are few (block, window) pairs (1/8 shard of C3: 1024 -> 256 tasks is 10 % faster:
    // fewer partial rows to write and to sum, no ragged second round)
    const int64_t full_rows = sh.ring > 1 ? (int64_t)sh.win_rows * (sh.ring - 1) : sh.win_rows;
    const int64_t blocks = ((int64_t)n_major + (64 / p.LPC) * wpb - 1) / ((64 / p.LPC) * wpb);
    const int64_t windows = ((int64_t)n_minor + full_rows - 1) / full_rows;
    // ... and half as many for an orientation with few blocks (the gene side of C3: 40 blocks of 512
    // genes): 1024 tasks there are 26 window ranges per block = 26 partial rows per gene to write and
    // to sum; 512 measured -3.5 % sweep, -15 % update time (profiles/r02/explore_tasks_per_side.log)
    int dflt = blocks * windows >= 2048 ? (wpb >= 12 ? 1024 : 2048) : 256;
    if (dflt >= 1024 && blocks < 64) dflt /= 2;
    sh.target_tasks = tn.tasks.value_or(dflt);
    // Half-window schedule (plan.h): the window's LDS cut into two slots, refilled at the epoch boundary
    // by the window kernel itself.  Chosen per orientation where it was measured to pay
    // (profiles/r02/explore_half_window.log, explore_half_midsize.log):
    //  * rows with many nonzeros per half window -- the lock-step loss is what it removes; with ~3 per
    //    half window (C5) the second barrier per window costs more;
    //  * the 1024-thread workgroup (64 KiB windows halved lose 5 %);
    //  * tasks long enough to work ahead in: the horizon ends with the task and a task's first epoch
    //    fills both slots.  >= 6 half windows per task in the one-launch iteration (C3 8 / 16: -2..3 %;
    //    half of C3's cells 4 / 8: the cell side +1..4 % with it; 1/8: +2 %), >= 4 in the two-launch
    //    iteration of a row shard (1/8 of C3: sweeps 2 x 70 -> 2 x 63 us).
    // SCHPF_HALF = 0 / slots overrides.
    // one-nonzero-at-a-time kernels (sweep_impl.h: rows wider than 96 bytes per lane in the 1024-thread workgroup --
    // the rolling loop in float64, the plain loop in float32) count their steps in nonzeros wherever rows do not
    // work ahead
    sh.single = (size_t)p.KL * p.elem > 96 && wpb >= 12;
    {
        int n_slots = tn.half >= 2 ? tn.half : 0;
        // balanced windows are whole windows (plan.h).  Decided for the upload, not per side: the library only
        // balances matrices with < 24 nonzeros per row and whole window, i.e. < 12 per half window, where the rule
        // below (>= 16) would not pick half windows either -- a side that then is NOT balanced (too small a
        // workgroup, no memory for the scratch) gets the same whole index-cut windows it would have got without
        // balancing.  Only a forced SCHPF_BALANCE=1 on a dense matrix can lose the half-window schedule this way.
        if (p.balance_now && tn.half < 2) n_slots = 0;
        else if (force_half >= 0) n_slots = force_half ? 2 : 0;
        else if (tn.half < 0 && sh.ring <= 1 && wpb >= 12) {
            const int64_t half_rows = ((int64_t)lds_kb * 512 - 64) / (int64_t)row_bytes;
            if (half_rows >= 1) {
                const double per_row = (double)p.nnz / std::max(1, n_major) * (double)half_rows / std::max(1, n_minor);
                const int64_t half_windows = ((int64_t)n_minor + half_rows - 1) / half_rows;
                const int64_t per_task = half_windows * blocks / std::max(1, sh.target_tasks);   // plan.cpp: wpt
                if (per_row >= 16.0 && per_task >= (p.expect_sharded ? 4 : 6)) n_slots = 2;
            }
        }
        if (n_slots >= 2 && sh.ring <= 1) {
            const int slot_bytes = (int)((size_t)lds_kb * 1024 / (size_t)n_slots / 16 * 16);
            const int64_t sub_rows = ((int64_t)slot_bytes - 64) / (int64_t)row_bytes;
            if (sub_rows >= 1) {
                sh.ring = n_slots;
                sh.sync_stage = 1;
                sh.slot_bytes = slot_bytes;
                sh.win_rows = (int)sub_rows;
                sh.single = false;   // rows work ahead: pairs
            }
        }
    }
    // workgroups in flight: one 1024-thread (152 KiB) workgroup per CU, two of the smaller ones; both
    // orientations share a launch unless the iteration is sharded (two launches, schpf_hint_sharded)
    const int per_launch = p.cu_count * (wpb >= 12 ? 1 : 2);
    sh.slots = p.expect_sharded ? per_launch : per_launch / 2;
    sh.ranges = ranges;
    return sh;
}

// Balanced windows where the rows are sparse in a window (on average under 24 nonzeros per row and 152 KiB window,
// both orientations: the C5 share has 7): there the lock-step padding is 45 % of the executed step slots and the
// balancing takes a quarter of the sweep's compute away; at C3 (49 per row and window) the half-window schedule
// already fills 0.87-0.93 of the slots and the row-list indirection of the staging costs what the rest would
// return (profiles/r04/ab_balanced_windows.txt).  SCHPF_BALANCE=1 / 0 forces it on / off.  Off for an engine that
// keeps a (row, col)-sorted copy (the plans' own order is then the virtual one) and for transient matrices.
bool balance_windows(const Problem &p, const Tuning &tn)
{
    const double win = 152.0 * 1024.0 / ((double)p.KP * p.elem);
    const double per_row_cell = (double)p.nnz / std::max(1, p.N) * std::min(1.0, win / std::max(1, p.G));
    const double per_row_gene = (double)p.nnz / std::max(1, p.G) * std::min(1.0, win / std::max(1, p.N));
    const bool sparse = per_row_cell < 24.0 && per_row_gene < 24.0 && (double)p.G > 2.0 * win && (double)p.N > 2.0 * win;
    return (tn.balance < 0 ? sparse : tn.balance != 0) && !p.want_rows && !p.transient;
}

// Chunk length of the gather plan: a power of two in 16..256 that leaves ~16 k waves.
int gather_chunk_len(const Problem &p)
{
    const int64_t target_waves = 16384;
    const int64_t c = p.nnz / (target_waves * (64 / p.LPC));
    int chunk = 16;
    while (chunk * 2 <= c && chunk < 256) chunk *= 2;
    return chunk;
}

void loss_cut_points(const TilePlanHost &h, int64_t t, int parts, std::vector<int> &cuts)
{
    const int min_windows = h.ring > 1 ? 4 : 2;   // sub-windows of the half-window schedule are half as long
    const int a0 = h.task_w0[(size_t)t], a1 = h.task_w1[(size_t)t];
    const int n = std::max(1, std::min(parts, (a1 - a0) / min_windows));
    cuts.clear();
    for (int q = 0; q <= n; ++q) cuts.push_back(a0 + (int)((int64_t)(a1 - a0) * q / n));
}

// Tasks of the loss pass.  The iteration's task ranges are chosen for the merged launch of both orientations and for
// few partial rows (C3 f64: ONE range per cell block = 196 tasks on 256 compute units -- a loss pass over them ran
// 0.42 ms where half a dual launch is 0.32); the loss pass keeps no partial rows, so every task's window range may be
// cut into `parts` sub-ranges (never below two windows / four sub-windows per sub-task: a first window costs a staging
// and the major rows).  `parts` is the count in 1..8 with the shortest modelled pass: the sub-tasks, longest first,
// on the resident workgroups (list schedule), a sub-task = its barrier-limited steps + two per window + a fixed cost.
// What decides is the last round: 784 equal tasks on 256 workgroups take four rounds, not 3.06 (measured: 0.46 ms
// against 0.41 for the gene-side plan's 640).  The modelled time also picks the plan (loss_side).  Needs the host
// copies of steps / task_wave_off.  A matrix that is replaced every iteration (minibatch engines: schpf_hint_transient,
// schpf_upload_rows) is planned the cheapest way, and batch engines never evaluate the loss themselves.
LossCut loss_cut(const Problem &p, const Tuning &tn, const TilePlanHost &h)
{
    LossCut c;
    if (h.n_tasks <= 0 || h.steps.empty() || h.task_wave_off.empty()) return c;
    if (p.transient || p.planning_batch_rows) return c;
    const int wpb = h.wpb, W = h.n_windows;
    const size_t lds = h.ring > 1 ? (size_t)h.ring * h.slot16 * 16 : (size_t)h.win_rows * p.KP * p.elem;
    const int resident = p.cu_count * per_cu(lds);
    const double task_cost = 8.0;
    // barrier-limited steps (+ 2) of every (block, window)
    std::vector<int32_t> &wwork = c.window_work;
    wwork.resize((size_t)h.n_blocks * W);
    for (int64_t b = 0; b < h.n_blocks; ++b)
        for (int w = 0; w < W; ++w) {
            int mx = 0;
            for (int v = 0; v < wpb; ++v) mx = std::max<int>(mx, h.steps[((size_t)b * wpb + v) * W + w]);
            wwork[(size_t)b * W + w] = (int32_t)tile_stored_steps(h, mx) + 2;
        }
    std::vector<int> cuts;
    std::vector<double> dur, load;
    auto model = [&](int parts) {
        dur.clear();
        for (int64_t t = 0; t < h.n_tasks; ++t) {
            loss_cut_points(h, t, parts, cuts);
            const int32_t *ww = wwork.data() + (size_t)h.task_block[(size_t)t] * W;
            for (size_t q = 0; q + 1 < cuts.size(); ++q) {
                double d = task_cost;
                for (int w = cuts[q]; w < cuts[q + 1]; ++w) d += ww[w];
                dur.push_back(d);
            }
        }
        std::sort(dur.begin(), dur.end(), std::greater<double>());
        load.assign((size_t)resident, 0.0);
        std::make_heap(load.begin(), load.end(), std::greater<double>());
        for (double d : dur) {
            std::pop_heap(load.begin(), load.end(), std::greater<double>());
            load.back() += d;
            std::push_heap(load.begin(), load.end(), std::greater<double>());
        }
        return *std::max_element(load.begin(), load.end());
    };
    const double uncut = model(1);
    c.model = uncut;
    if (tn.loss_split)
        for (int parts = 2; parts <= 8; ++parts) {
            const double m = model(parts);
            if (m < 0.97 * c.model) { c.model = m; c.parts = parts; }   // a cut has to pay for itself
        }
    if (tn.verbose)
        fprintf(stderr, "[schpf_hip]   loss pass on the %d x %d plan: %d sub-range(s) per task, modelled %.0f step units (uncut %.0f)\n",
                h.n_major, h.n_minor, c.parts, c.model, uncut);
    return c;
}

// The loss pass sweeps ONE plan, either will do (both hold every nonzero; r = sum_k E[theta] E[beta] is symmetric).
// The cell-side plan unless it has too few tasks to fill the device and the gene-side plan has more: the task ranges
// are chosen for the iteration's merged launch, where C3 f64 gets one range per cell block = 196 tasks for 256
// compute units (loss pass 421 us on the cell plan; the gene plan's 640 tapered tasks: see DESIGN 9).
int loss_side(const Problem &p, const Tuning &tn, bool gene_fits, const double model[2], const int64_t tasks[2],
              size_t cell_lds_bytes)
{
    if (tn.loss_side == 0 || tn.loss_side == 1) return tn.loss_side;
    if (!gene_fits) return 0;
    // the plan with the shorter modelled pass (loss_cut); the gene side's steps are worth a little more: its windows
    // are shorter (more stagings per nonzero than the model's two step units per window say)
    if (model[0] > 0.0 && model[1] > 0.0) return model[1] * 1.05 < model[0] ? 1 : 0;
    const int64_t resident = (int64_t)p.cu_count * per_cu(cell_lds_bytes);
    return (tasks[0] < 2 * resident && tasks[1] > tasks[0]) ? 1 : 0;
}

}  // namespace schpf
