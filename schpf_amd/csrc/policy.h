// Planning policy of an engine: which plan kind, row layout, workgroup shape, task ranges and loss-pass cut a matrix
// gets, and every environment switch the planner and the launches consult.  Host-only decisions: the
// engine (capi.hip) holds the device state and carries them out.  A Problem is made per question: during an upload
// from the engine and that upload's record (Engine::problem(UploadJob)), afterwards from the engine alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <optional>
#include <vector>

#include "plan.h"

namespace schpf {

// The switches of DESIGN 10, read once: by schpf_create for an engine, on every call by the debug entry points.
// An empty optional is "not set"; where that default depends on the caller it is applied there.
struct Tuning {
    enum Plan { PLAN_AUTO, PLAN_TILE, PLAN_GATHER };
    Plan plan = PLAN_AUTO;          // SCHPF_PLAN=tile / gather
    int half = -1;                  // SCHPF_HALF: -1 auto, 0 off, n >= 2 forces n slots
    int balance = -1;               // SCHPF_BALANCE: -1 auto, 0 / 1 force balanced windows off / on
    int wpb = 0;                    // SCHPF_WPB: waves per workgroup (0: auto)
    std::optional<int> tasks;       // SCHPF_TASKS: tasks per orientation; set, it also switches the range model off
    std::optional<int> taper;       // SCHPF_TAPER, per cent: 30 for an engine, 0 for schpf_debug_tile_expand
    int bank_order = 2;             // SCHPF_BANK_ORDER (plan.h TileShape)
    bool dual = true;               // SCHPF_DUAL: both sweeps in one launch
    bool persistent = true;         // SCHPF_PERSISTENT: persistent workgroups that draw tasks from a counter
    bool device_plan = true;        // SCHPF_DEVICE_PLAN: tile plans built on the device (0: host builder)
    int loss_side = -1;             // SCHPF_LOSS_SIDE: -1 model, 0 / 1 force the cell / gene plan
    bool loss_split = true;         // SCHPF_LOSS_SPLIT: the loss pass on sub-ranges of the tasks
    bool fuse_sums = true;          // SCHPF_FUSE_SUMS: small problems fold the column sums into the updates
    bool graph = true;              // SCHPF_GRAPH: schpf_steps as one hipGraph
    std::optional<bool> graph_sharded;  // SCHPF_GRAPH_SHARDED: default on for a one-rank communicator
    bool verbose = false;           // SCHPF_VERBOSE: plan-build timings on stderr
    int debug_row_slots = 10;       // SCHPF_DEBUG_ROW_SLOTS, _SINGLE, _BALANCE: schpf_debug_tile_expand only
    bool debug_single = false, debug_balance = false;
};
Tuning tuning_from_env();

// What the policy knows of an engine and its matrix.  elem = sizeof(T); LPC / NV / KL / KP from choose_config.
struct Problem {
    int N = 0, G = 0, K = 0, elem = 8;
    int64_t nnz = 0;
    int cu_count = 256;
    int LPC = 1, NV = 1, KL = 0, KP = 0;
    bool expect_sharded = false;        // schpf_hint_sharded
    bool transient = false;             // schpf_hint_transient
    bool want_rows = false;             // schpf_keep_rows
    bool planning_batch_rows = false;   // this upload is schpf_upload_rows' (UploadJob::batch_rows); unset after it
    bool balance_now = false;           // balanced windows for this upload (balance_windows); unset after it
};

struct Config { bool tile; int LPC, NV, KL, KP; };
Config choose_config(int K, int elem, const Tuning &tn);

int per_cu(size_t window_lds_bytes);
void pick_workgroup(const Problem &p, const Tuning &tn, int n_major, int n_minor, int &wpb, int &lds_kb);
int pick_windows(size_t table_bytes);
// The sampled histograms are made where the COO lies: sample(stride, hist) fills hist[0][N] / hist[1][G] with the counts
// of the row / col indices at the positions i * stride (plan.h sample_histogram).  Called only when the model runs
using SampleHistograms = std::function<void(int64_t stride, std::vector<int32_t> hist[2])>;
bool choose_ranges(const Problem &p, const Tuning &tn, const SampleHistograms &sample, int ranges[2], int half[2]);
TileShape tile_shape(const Problem &p, const Tuning &tn, int n_major, int n_minor, int ranges = 0, int force_half = -1);
bool balance_windows(const Problem &p, const Tuning &tn);
int gather_chunk_len(const Problem &p);

// The loss pass's cut of a tile plan's tasks into sub-ranges (LossCut::parts; 1: the iteration's own tasks).
struct LossCut {
    int parts = 1;
    double model = 0.0;                 // modelled length of the pass in step units (0: not modelled)
    std::vector<int32_t> window_work;   // barrier-limited steps + 2 of every (block, window)
};
LossCut loss_cut(const Problem &p, const Tuning &tn, const TilePlanHost &h);
void loss_cut_points(const TilePlanHost &h, int64_t t, int parts, std::vector<int> &cuts);
// model / tasks: per side (0 cell, 1 gene), the modelled loss pass (LossCut::model) and the iteration's task count
int loss_side(const Problem &p, const Tuning &tn, bool gene_fits, const double model[2], const int64_t tasks[2],
              size_t cell_lds_bytes);

}  // namespace schpf
