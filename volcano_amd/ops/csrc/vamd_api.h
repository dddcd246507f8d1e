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
//   mode 3, network topology: confine the class to ONE hypernode, chosen
//     from the live cap.  dom_of = leaf_of[N] (the node's leaf id in
//     [0, D), -1 = in no hypernode; leaves are numbered depth-first, so a
//     hypernode of any tier is one leaf range [lo, hi)), D = number of
//     leaves, and dom_count is a read-only int32 table instead of counts:
//       tab[0] T       tiers to try, lowest first (>= 1)
//       tab[1] need    instances that must fit in the domain (>= 1)
//       tab[2] pin_lo  a domain is eligible iff lo <= pin_lo and
//       tab[3] pin_hi    pin_hi <= hi; no pin: pin_lo = D, pin_hi = 0
//       tab[4] soft    0 = hard, 1 = soft
//       tab[5..5+T]    off[t]: start of tier t's (lo, hi) pairs, off[T] =
//                      end; offsets into tab
//       ...            the pairs, tier by tier
//     With C = sum of cap over the leaves of [lo, hi) (int64), the first
//     tier with an eligible domain of C >= need wins, within it the
//     smallest C, ties to the lower table index.  Nodes outside the
//     winner are masked; without a winner hard masks every node, soft
//     none.  `scratch` holds 8*(D+1) bytes (used above
//     vamd_hypernode_lds_leaves() leaves).
void vamd_domain_mask(
    float* score, int* cap, const int* dom_of, const int* dom_count, int D,
    int mode, void* scratch, int N, hipStream_t stream);

// Largest D whose leaf sums mode 3 keeps in LDS.
int vamd_hypernode_lds_leaves(void);

// dom_count[dom_of[log_nodes[e]]] += log_counts[e] for e < *log_len
// (<= K), after the select of a domain-mask class.
void vamd_domain_count_add(
    const int* log_nodes, const int* log_counts, const int* log_len,
    const int* dom_of, int* dom_count, int D, int N, int K,
    hipStream_t stream);

// --- several topology-spread rules per class ---------------------------------
//
// Up to VAMD_SPREAD_MAX_RULES rules, passed by value: a node may take an
// instance only while EVERY rule's count[dom_of[n]] + 1 - min(count) <= skew
// holds, so it is eligible in the intersection of the rules' open domains.
#define VAMD_SPREAD_MAX_RULES 4

struct VamdSpreadRule {
    const int32_t* dom_of;   // [N] node -> domain id of this rule, -1 = no label
    int32_t* count;          // [D] group members per domain, in place
    int32_t D;               // in [1, N]
    int32_t skew;            // >= 1
};

struct VamdSpreadRules {
    VamdSpreadRule r[VAMD_SPREAD_MAX_RULES];
    int32_t n;               // rules in use, 1..VAMD_SPREAD_MAX_RULES
    int32_t _pad;
};

// The two launchers are weak, like the pack launchers: a program that links
// the runner alone leaves class_spread_rules unset and never calls them.

// vamd_spread_select under rules.n rules at once (after vamd_score_cap; ONE
// workgroup).  Every placement joins the counts of every rule; a fused gang
// that misses fuse_min gives them all back.  The domains' eligibility bits
// live in LDS: sum of D over the rules <= vamd_spread_multi_lds_domains().
// `slot` holds 4*N bytes.  With one rule the result is that of
// vamd_spread_select.  A rule set outside these limits places nothing:
// *log_len = 0 and *placed = 0.
__attribute__((weak)) void vamd_spread_multi_select(
    float* score, int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    VamdSpreadRules rules, int fuse_min, void* slot, int N, int R, int K,
    hipStream_t stream);

// When *flag == 0: the log (e < *log_len <= K) leaves the counts of rules
// 1..n-1.  Runs BEFORE vamd_spread_revert, which gives rule 0 its counts back
// and zeroes the log.
__attribute__((weak)) void vamd_spread_multi_count_sub(
    const uint8_t* flag, const int* log_nodes, const int* log_counts,
    const int* log_len, VamdSpreadRules rules, int N, int K,
    hipStream_t stream);

// Largest sum of D over the rules of one vamd_spread_multi_select.
__attribute__((weak)) int vamd_spread_multi_lds_domains(void);

// --- re-scoring select (nodeorder exact) -------------------------------------
//
// vamd_select_commit with the chosen node scored again after EVERY placement
// (after vamd_score_cap and any cap or mask launcher; ONE workgroup).  It
// takes the score inputs of vamd_fused_score_select: the score of a node with
// k instances staged is the vamd_score_cap formula on
// used_k = fma(k, req, used), bit for bit, or -inf when the node is full or
// the formula's fit test fails there; no other node's score moves.  `score`
// is consumed, `cap` only read; `slot` holds 4*N bytes.  The log carries one
// (node, count) entry per node in order of first placement, so everything
// that reads the log of vamd_select_commit reads this one.  Log entries past
// *log_len are left as they were, as by the other selects.  Weak, like the
// launchers above: the runner calls it only for a class flagged in
// class_rescore.
__attribute__((weak)) void vamd_rescore_select(
    const float* alloc, float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score, const int* cap,
    int ntasks, float* queue_alloc, const float* queue_limit,
    int* log_nodes, int* log_counts, int* log_len, int* placed,
    int* job_placed, int fuse_min, void* slot, int N, int R, int W, int K,
    hipStream_t stream);

// --- re-scoring select under topology spread ---------------------------------
//
// vamd_spread_multi_select (1..VAMD_SPREAD_MAX_RULES rules, the same limits,
// the same count updates and gang give-back) with the chosen node scored
// again after EVERY placement, as vamd_rescore_select scores it: the formula
// of vamd_score_cap on used_k = fma(k, req, used) for its k staged instances,
// -inf once k reaches cap[node] or the fit test fails.  After vamd_score_cap
// and any cap launcher; ONE workgroup.  `score` is consumed, `cap` only read;
// `slot` holds 4*N bytes.  With scores that never fall within the class the
// result is that of vamd_spread_multi_select; with rules that never bind,
// that of vamd_rescore_select.  Weak, like the launchers above: the runner
// calls it only for a class flagged in class_spread_rescore.
__attribute__((weak)) void vamd_spread_rescore_select(
    const float* alloc, float* used, const float* extra, const float* req,
    float w_least, float w_most, float w_bal, const float* dim_w,
    const float* bias, float* score, const int* cap, int ntasks,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    VamdSpreadRules rules, int fuse_min, void* slot, int N, int R, int K,
    hipStream_t stream);

// --- soft topology spread (whenUnsatisfiable: ScheduleAnyway) ----------------
//
// One f32 weight per rule of a VamdSpreadRules, passed by value beside it:
// tw[r] == 0 marks rule r hard, anything else soft.
struct VamdSpreadWeights {
    float tw[VAMD_SPREAD_MAX_RULES];
};

// vamd_spread_rescore_select with soft rules among its 1..4.  A hard rule
// filters on its skew as there.  A soft rule never filters on counts (a node
// without its label is still out); before EVERY placement a node's key is
// score - pen, pen = fma(tw_R, float(count_R[dom_R]), ... fma(tw_1,
// float(count_1[dom_1]), 0)) over the soft rules in rule order, the best key
// among the nodes open under every hard rule wins (ties to the lower index),
// and every rule's count rises.  With `rescore` nonzero the chosen node is
// scored again as in vamd_spread_rescore_select; otherwise its score stays
// until its capacity is used up.  A fused gang that misses fuse_min gives
// every rule its counts back.  Limits: sum of D over the hard rules <=
// vamd_spread_multi_lds_domains(), over the soft rules <=
// vamd_spread_soft_lds_domains(); a set outside them places nothing.
// After vamd_score_cap and any cap launcher; ONE workgroup; `score` is
// consumed, `cap` only read; `slot` holds 4*N bytes.  Weak: the runner calls
// it only for a class with a nonzero row in class_spread_soft.
__attribute__((weak)) void vamd_spread_soft_select(
    const float* alloc, float* used, const float* extra, const float* req,
    float w_least, float w_most, float w_bal, const float* dim_w,
    const float* bias, float* score, const int* cap, int ntasks,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    VamdSpreadRules rules, VamdSpreadWeights weights, int rescore,
    int fuse_min, void* slot, int N, int R, int K, hipStream_t stream);

// Largest sum of D over the soft rules of one vamd_spread_soft_select.
__attribute__((weak)) int vamd_spread_soft_lds_domains(void);

// --- per-unit packing: GPU slices on cards, CPU requests on NUMA zones ------
//
// A pod takes its request from the units of a node; the rule is the host's
// own, once per pod, computed in closed form: a unit has a fixed number of
// slots for a request, a node packs sum(slots) / need pods, and pods in a
// row fill the units in a strict order among units with slots, each to its
// slot count.  Unit planes are int32 [U, N] (unit-major).  A commit records
// what it took in assign[L, U], parallel to the log: the used units of
// entry e in fill order, unit << 28 | take; the tail is 0.
//
// The six launchers are weak: a program that links the runner alone leaves
// both blocks of VamdCycle unset and never calls them.
//
// Device share.  Card planes [K, N], K <= vamd_device_max_cards():
// card_mem_used, card_cores_used (percent) and card_state = slice count,
// with VAMD_CARD_GONE set for an exclusive or absent card;
// card_mem_total[N] < 2^28.  A request is (count slices, memory per slice,
// cores per slice); memory == 0 && cores == 0 asks for whole cards.  The
// rule is GPUDevicePool.allocate (best fit: fullest feasible card first,
// ties to the lower index).
#define VAMD_CARD_GONE (1 << 30)

// After vamd_score_cap, before any domain rule: cap = min(cap, S / count)
// with S the node's slots for the shape; score = -inf where that is 0.
__attribute__((weak)) void vamd_device_cap(
    float* score, int* cap, const int* card_mem_used,
    const int* card_cores_used, const int* card_state,
    const int* card_mem_total, int count, int memory, int cores, int K,
    int N, hipStream_t stream);

// After the select: entry e < *log_len (<= L) of the log takes
// log_counts[e] * count slices on node log_nodes[e], cards in the order
// (mem_used desc, index asc) among cards with slots, recorded in
// assign[L, K].
__attribute__((weak)) void vamd_device_commit(
    const int* log_nodes, const int* log_counts, const int* log_len,
    int* card_mem_used, int* card_cores_used, int* card_state,
    const int* card_mem_total, int* assign, int count, int memory, int cores,
    int K, int N, int L, hipStream_t stream);

// When *flag == 0: gives back what the assignment rows recorded and zeroes
// them (beside vamd_cond_revert / vamd_spread_revert).
__attribute__((weak)) void vamd_device_revert(
    const uint8_t* flag, const int* log_nodes, const int* log_len,
    int* card_mem_used, int* card_cores_used, int* card_state, int* assign,
    int memory, int cores, int K, int N, int L, hipStream_t stream);

// Largest K of the card planes.
__attribute__((weak)) int vamd_device_max_cards(void);

// Numaaware.  zone_free is one plane [Z, N], Z <= vamd_numa_max_zones():
// free millicores of zone z of node n, 0 <= free < 2^28, 0 for the missing
// zones of a smaller node.  A request is `cpu` >= 1 millicores that must
// come from ONE zone: zone z has free / cpu slots.  The rule is
// NumaState.best_zone / take (the smallest zone that still fits, ties to
// the lower index): zones fill in the order (free asc, index asc).

// Hard policies only, after vamd_score_cap (and vamd_device_cap), before any
// domain rule: cap = min(cap, S) with S the node's slots; score = -inf
// where that is 0.
__attribute__((weak)) void vamd_numa_cap(
    float* score, int* cap, const int* zone_free, int cpu, int Z, int N,
    hipStream_t stream);

// After the select: the first min(log_counts[e], S) pods of entry
// e < *log_len (<= L) take a zone each on node log_nodes[e]; the rest stay
// unpinned; recorded in assign[L, Z].
__attribute__((weak)) void vamd_numa_commit(
    const int* log_nodes, const int* log_counts, const int* log_len,
    int* zone_free, int* assign, int cpu, int Z, int N, int L,
    hipStream_t stream);

// When *flag == 0: gives back what the assignment rows recorded and zeroes
// them (beside vamd_cond_revert / vamd_spread_revert / vamd_device_revert).
__attribute__((weak)) void vamd_numa_revert(
    const uint8_t* flag, const int* log_nodes, const int* log_len,
    int* zone_free, int* assign, int cpu, int Z, int N, int L,
    hipStream_t stream);

// Largest Z of the zone plane.
__attribute__((weak)) int vamd_numa_max_zones(void);

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
    // domain-rule block (topology spread, inter-pod (anti-)affinity,
    // network topology): live only when class_group, dom_of, count and
    // domain_scratch are all set
    const int32_t* class_group;    // HOST [C]: group index or -1
    const int32_t* class_skew;     // HOST [C]: maxSkew (>= 1, mode 0)
    const int32_t* class_mode;     // HOST [C]: 0 / 1 / 2 / 3; null = all 0
    const int32_t* dom_of;         // [rows, N]; rows = G without group_row
    int32_t* count;                // groups back to back (mode 3: tables)
    const int32_t* count_off;      // HOST [G]: offset into count
    const int32_t* domains;        // HOST [G]: D of each group
    void* domain_scratch;          // 12*N bytes, 8-aligned
    const int32_t* group_row;      // HOST [G]: row of dom_of for group g; null = g
    // device-share block: live only when all of it is set (card_K >= 1)
    int32_t* card_mem_used;        // [card_K, N]
    int32_t* card_cores_used;      // [card_K, N]
    int32_t* card_state;           // [card_K, N]
    const int32_t* card_mem_total; // [N]
    const int32_t* class_dev_req;  // HOST [C, 4]: count, memory, cores, 0;
                                   //   count == 0 = no device request
    int32_t* dev_assign;           // [L, card_K], parallel to the log
    int32_t card_K;
    int32_t _pad2;
    // NUMA block: live only when all of it is set (zone_Z >= 1)
    int32_t* zone_free;            // [zone_Z, N]
    const int32_t* class_numa_req; // HOST [C, 2]: cpu millicores, policy
                                   //   (0 = none, 1 = hard, 2 = best-effort)
    int32_t* numa_assign;          // [L, zone_Z], parallel to the log
    int32_t zone_Z;
    int32_t _pad3;
    // several spread rules per class: live when set (and the domain-rule
    // block is).  Row c is n, then VAMD_SPREAD_MAX_RULES (group, maxSkew)
    // pairs; the class is multi-rule when n >= 2 and then also carries rule 0
    // in class_group / class_skew with mode 0
    const int32_t* class_spread_rules;  // HOST [C, 9]
    // re-scoring block: live when both are set.  A class with a nonzero
    // flag has its chosen node scored again after every placement
    const int32_t* class_rescore;  // HOST [C]
    int32_t* rescore_slot;         // [N] scratch of vamd_rescore_select
    // live when set (and the domain-rule block is): a spread class (mode 0)
    // with a nonzero flag runs vamd_spread_rescore_select, for one rule or
    // several
    const int32_t* class_spread_rescore;  // HOST [C]
    // live when set (and the domain-rule block is): row c holds one weight
    // per rule of spread class c, in the order of class_spread_rules (or rule
    // 0 alone); a row with a nonzero weight runs vamd_spread_soft_select
    const float* class_spread_soft;  // HOST [C, VAMD_SPREAD_MAX_RULES]
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
//   * A spread class with n >= 2 rules (class_spread_rules[c]) runs
//     vamd_spread_multi_select in place of vamd_spread_select, and its
//     multi-class revert runs vamd_spread_multi_count_sub before
//     vamd_spread_revert.  With the column null nothing changes a single
//     launch.
//   * An affinity (mode 1) / keyed anti-affinity (mode 2) class always
//     runs vamd_score_cap -> vamd_domain_mask -> vamd_select_commit (bulk
//     by size, given sort_scratch) -> vamd_domain_count_add: a launch
//     count constant in ntasks; it reverts through vamd_spread_revert.
//   * A network-topology class (mode 3) always runs vamd_score_cap ->
//     vamd_domain_mask(3) -> vamd_select_commit (bulk by size): its count
//     slice is a read-only table, so there is no count update and it
//     reverts through vamd_cond_revert.  All such groups of a cycle can
//     share one leaf_of row through group_row.
//   * With the domain block dead (or every group -1) nothing above
//     changes a single launch.
//   * A class with a device request (device-share block live,
//     class_dev_req[c].count > 0) always takes the split path:
//     vamd_score_cap -> vamd_device_cap -> [its domain rule] -> select
//     (bulk by size) -> [count update] -> vamd_device_commit — never the
//     fused, chain or megacycle path — and its multi-class revert runs
//     vamd_device_revert beside the existing one.  With the block dead
//     nothing changes a single launch.
//   * A class with a NUMA request (NUMA block live, class_numa_req[c]
//     .policy != 0) takes the same split path: vamd_score_cap ->
//     [vamd_device_cap] -> [vamd_numa_cap, hard policy only] -> [its domain
//     rule] -> select (bulk by size) -> [count update] ->
//     [vamd_device_commit] -> vamd_numa_commit, and its multi-class revert
//     runs vamd_numa_revert as well.  With the block dead nothing changes a
//     single launch.
//   * A re-scoring class (re-scoring block live, class_rescore[c] != 0)
//     always takes the split path: vamd_score_cap -> [vamd_device_cap] ->
//     [vamd_numa_cap] -> [vamd_domain_mask, modes 1/2/3] ->
//     vamd_rescore_select -> [count update] -> [commits] — never the fused,
//     bulk, chain or megacycle path (a chain run breaks at it, a megacycle
//     plan that holds one runs per class).  Its reverts are those of its
//     domain rule.  A spread class (mode 0) never reads this flag: it has
//     its own, below.  With the block dead nothing changes a single launch.
//   * A spread class flagged in class_spread_rescore runs
//     vamd_spread_rescore_select in place of vamd_spread_select /
//     vamd_spread_multi_select, for one rule or several (one rule travels as
//     a rule set of one; the slot is the first 4*N bytes of the domain
//     scratch).  The caps before, the commits after and the multi-class
//     reverts are those of the select it replaces.  With the column null
//     nothing changes a single launch.
//   * A spread class whose class_spread_soft row has a nonzero weight runs
//     vamd_spread_soft_select where any of the three selects above would
//     stand, with class_spread_rescore[c] as its re-score flag.  A class with
//     only soft rules carries rule 0 in class_group / class_skew with a skew
//     that never binds.  Everything around the select is unchanged.  With
//     the column null nothing changes a single launch.
// Returns 0; nonzero, before any HIP call, when cy->struct_size is not
// sizeof(VamdCycle).
int vamd_run_cycle(const VamdCycle* cy, hipStream_t stream);

}  // extern "C"
