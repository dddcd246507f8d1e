// C ABI of the MI355X scheduler kernel library (loaded via ctypes —
// deliberately no torch/pybind dependency: pure HIP, zero ABI hazards).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

extern "C" {

void vamd_score_cap(
    const float* alloc, const float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score_out, int* cap_out,
    int N, int R, int W, hipStream_t stream);

void vamd_select_commit(
    float* score, const int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed, int fuse_min,
    unsigned* sort_scratch,  // [4N] bulk-fill radix scratch (nullable)
    int N, int R, int K, hipStream_t stream);

void vamd_fused_score_select(
    const float* alloc, float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score, int* cap,
    int ntasks, float* queue_alloc, const float* queue_limit,
    int* log_nodes, int* log_counts, int* log_len, int* placed,
    int* job_placed, int fuse_min, int N, int R, int W, int K,
    hipStream_t stream);

void vamd_finalize_job(
    const int* job_placed, int occupied, int min_available,
    const int* class_placed, const int* class_min, uint8_t* flag, int nc,
    hipStream_t stream);

void vamd_cond_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, int N, int R, hipStream_t stream);

// Topology-spread select (after vamd_score_cap; ONE workgroup): maxSkew is
// checked before every single placement against the group's live
// per-domain counts.  `score` and `cap` are consumed.  `scratch` holds
// 8*D + 4*N bytes, 8-byte aligned.  D in [1, N]; dom_of[n] in [-1, D).
void vamd_spread_select(
    float* score, int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    const int* dom_of,       // [N] node -> domain id, -1 = no label
    int* dom_count,          // [D] group members per domain, in place
    int D, int max_skew, int fuse_min,
    void* scratch, int N, int R, int K, hipStream_t stream);

// vamd_cond_revert for a spread class: also takes the logged placements
// back out of dom_count.
void vamd_spread_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, const int* dom_of, int* dom_count, int D, int N, int R,
    hipStream_t stream);

// Inter-pod (anti-)affinity over a topology key, per placement (after
// vamd_score_cap, before vamd_select_commit; ONE workgroup).  Masks
// score/cap in place (masked: score = -inf, cap = 0) so that the ordinary
// select yields the sequential per-instance result.
//   mode 1, affinity: keep nodes of domains with count > 0; if there is
//     none, keep the domain of the best placeable node (the anchor).
//   mode 2, anti-affinity: keep the best node of each domain with
//     count == 0, with cap 1.
// Nodes with dom_of < 0 are masked in both modes.  `scratch` holds 8*D
// bytes, 8-byte aligned (used in mode 2).  D in [1, N].
void vamd_domain_mask(
    float* score, int* cap, const int* dom_of, const int* dom_count, int D,
    int mode, void* scratch, int N, hipStream_t stream);

// dom_count[dom_of[log_nodes[e]]] += log_counts[e] for e < *log_len
// (<= K), after the select of a domain-mask class.
void vamd_domain_count_add(
    const int* log_nodes, const int* log_counts, const int* log_len,
    const int* dom_of, int* dom_count, int D, int N, int K,
    hipStream_t stream);

// --- whole-cycle runner ----------------------------------------------------

// One task class (a batch of identical pending tasks of one job).
struct VamdClassDesc {
    int32_t job_idx;      // index into the job desc array
    int32_t queue_idx;    // row of queue_alloc / queue_limit
    int32_t ntasks;       // instances to place
    int32_t min_needed;   // per-class (role) minimum
    int32_t log_off;      // offset into the log arrays
    int32_t log_cap;      // slot capacity (>= min(ntasks, N))
    int32_t flags;        // bit0: use extra (future-idle) credit
    int32_t bias_row;     // row of bias_rows for this class, or -1 → plan bias
    float w_least, w_most, w_bal;  // score weights for this class's queue tier
    float _padf;
};

// One job (PodGroup shard-local view).
struct VamdJobDesc {
    int32_t class_begin;  // [begin, end) into the class array
    int32_t class_end;
    int32_t occupied;     // tasks already holding resources at cycle start
    int32_t min_available;
};

// Shared by the runner (host) and the megacycle / chain kernels (device).
#if defined(__HIPCC__)
#define VAMD_HD __host__ __device__
#else
#define VAMD_HD
#endif

// Gang minimum of a single-class job, fused into its select: how many more
// tasks the job needs to become ready (min_available - occupied), never
// less than the class's own role minimum, never negative.
VAMD_HD inline int gang_fuse_min(const VamdJobDesc& job,
                                 const VamdClassDesc& cd) {
    int need = job.min_available - job.occupied;
    if (cd.min_needed > need) need = cd.min_needed;
    return need > 0 ? need : 0;
}

// Future-idle credit plane (flags bit0) and bias plane of a class: its own
// row of bias_rows (task-topology bucket packing) overrides the plan bias.
struct VamdClassPlanes { const float* ext; const float* bias; };

VAMD_HD inline VamdClassPlanes class_planes(
    const VamdClassDesc& cd, const float* extra, const float* bias,
    const float* bias_rows, int N) {
    return {(cd.flags & 1) ? extra : nullptr,
            (cd.bias_row >= 0 && bias_rows)
                ? bias_rows + (size_t)cd.bias_row * N : bias};
}

// Everything one allocate cycle reads and writes.  Device pointers unless
// marked HOST; C = n_classes, J = n_jobs.
struct VamdCycle {
    uint64_t struct_size;          // sizeof(VamdCycle), checked on entry
    int32_t N, R, W;
    int32_t n_classes, n_jobs;
    int32_t _pad;
    const VamdClassDesc* classes;  // HOST [C]
    const VamdJobDesc* jobs;       // HOST [J]
    // node state [R, N] (+ masks)
    const float* alloc;
    float* used;
    const float* extra;
    const uint8_t* ready;          // [N]
    const int64_t* taints;         // [N]
    const int64_t* planes;         // [W, N]
    const float* bias;             // [N] plan-wide (nullable)
    const float* bias_rows;        // [B, N] per-class rows (nullable)
    // per-class constraint rows
    const float* class_req;        // [C, R]
    const int64_t* class_tol;      // HOST [C]
    const int64_t* class_require;  // [C, W]
    const int64_t* class_forbid;   // [C, W]
    const int32_t* class_min;      // [C] (device copy of min_needed, for finalize)
    const float* dim_w;            // [R]
    // queue state
    float* queue_alloc;            // [Q, R]
    const float* queue_limit;      // [Q, R]
    // outputs / scratch
    float* score_scratch;          // [N]
    int* cap_scratch;              // [N]
    int* log_nodes;                // [L]
    int* log_counts;               // [L]
    int* log_len;                  // [C]
    int* class_placed;             // [C]
    int* job_placed;               // [J]
    uint8_t* job_flag;             // [J]
    unsigned* sort_scratch;        // [4N] bulk-select radix scratch (nullable)
    // domain-rule block (topology spread, inter-pod (anti-)affinity): live
    // only when class_group, dom_of, count and domain_scratch are all set
    const int32_t* class_group;    // HOST [C]: group index or -1
    const int32_t* class_skew;     // HOST [C]: maxSkew (>= 1, mode 0)
    const int32_t* class_mode;     // HOST [C]: 0 / 1 / 2; null = all 0
    const int32_t* dom_of;         // [G, N]
    int32_t* count;                // groups back to back
    const int32_t* count_off;      // HOST [G]: offset into count
    const int32_t* domains;        // HOST [G]: D of each group
    void* domain_scratch;          // 12*N bytes, 8-aligned
};

// Device copies of the descriptor arrays (chain and megacycle paths).
struct VamdDevDescs {
    const VamdClassDesc* classes;  // [C]
    const VamdJobDesc* jobs;       // [J]
    const int64_t* class_tol;      // [C]
};

// Chain path (heterogeneous mixes): batch-score a chunk of consecutive
// single-class jobs against chunk-start usage, then replay their selects
// in one launch with lazy exact re-scoring of touched nodes.  Decisions
// are bit-identical to the per-class path (see scheduler_kernels.hip).
// These three are called by the runner only.
void vamd_batch_score(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                      int count, float* score_buf, hipStream_t stream);

void vamd_topk(float* score_buf, int count, float* topk_vals, int* topk_ids,
               int N, hipStream_t stream);

void vamd_select_chain(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                       int c1, float* score_buf, const float* topk_vals,
                       const int* topk_ids, uint8_t* touched,
                       int* touched_list, hipStream_t stream);

// One launch for a whole small-class plan (heterogeneous shapes).
void vamd_megacycle(const VamdCycle& cy, const VamdDevDescs& dd,
                    hipStream_t stream);

// Executes a whole allocate cycle: for each job (in the host-given order),
// for each of its classes: score_cap + select_commit; then the gang
// finalize/revert.  Single-class jobs fuse the gang check into
// select_commit (2 launches per job).  Everything stays on `stream`;
// NO host synchronisation happens here.
//   * A spread class (class_group[c] >= 0, mode 0) always runs
//     vamd_score_cap + vamd_spread_select — never the fused, bulk, chain
//     or megacycle path — and reverts through vamd_spread_revert.  Counts
//     carry across the classes of a group in plan order, on the device.
//   * An affinity (mode 1) / keyed anti-affinity (mode 2) class always
//     runs vamd_score_cap -> vamd_domain_mask -> vamd_select_commit (bulk
//     by size, given sort_scratch) -> vamd_domain_count_add: a launch
//     count constant in ntasks; it reverts through vamd_spread_revert.
//   * With the domain block dead (or every group -1) nothing above
//     changes a single launch.
// Returns 0; nonzero, before any HIP call, when cy->struct_size is not
// sizeof(VamdCycle).
int vamd_run_cycle(const VamdCycle* cy, hipStream_t stream);

}  // extern "C"
