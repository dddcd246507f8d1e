// MI355X (gfx950 / CDNA4) scheduler kernels — the decision-plane hot loop.
//
// Semantics oracle: volcano_amd/ops/reference.py (PyTorch).  Reference
// behavior being rebuilt: volcano-sh/volcano pkg/scheduler/actions/allocate
// (allocate.go:719-953), util/predicate_helper.go:45, scheduler_helper.go:78,
// framework/statement.go (gang transaction) — re-designed as dense tensor
// passes instead of per-(task,node) Go callbacks.
//
// Layout: node state is SoA / transposed [R, N] so a wave's 64 lanes read
// 64 consecutive floats of one resource dim — fully coalesced on HBM3E.
// All kernels are enqueued on one HIP stream with ZERO host syncs per
// scheduling cycle; the gang commit/revert decision is taken on-device.
//
// Sizing: N (nodes) up to ~1M, R (resource dims) <= 16, W (label planes
// words) <= 4.  The per-class tensors are tiny (N*4B score) and L2/LLC
// resident; kernels are memory-latency/launch bound, not HBM bound.

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

#include "vamd_api.h"   // VamdClassDesc/VamdJobDesc for the megacycle

#define DEVINL __device__ __forceinline__

namespace vamd {

constexpr int WAVE = 64;              // CDNA wavefront width (NOT 32)
#define NEG_INF (-__builtin_inff())   // matches the torch reference's -inf
constexpr float EPS = 1e-4f;
constexpr long long BIG_CAP = 1 << 30;

// ---------------------------------------------------------------------------
// K1+K2 fused: per-node feasibility + capacity + score for one task class.
//   grid-stride over N; one thread = one node; all loads coalesced ([R,N]).
// ---------------------------------------------------------------------------
// core of K1+K2: score/cap for nodes {start, start+step, ...} — shared
// by the grid-stride kernel and the fused megacycle (block stride)
// per-node score/cap/feasibility — the ONE implementation shared by the
// grid-stride kernel, the batched chain scorer, and the chain select's
// live re-scoring of touched nodes.  Float op order is fixed: every
// caller gets bit-identical values for identical inputs (the decision-
// exactness contract with the torch oracle).
struct NodeScore { float s; int cap; };

DEVINL NodeScore node_score_one(
    int i,
    const float* __restrict__ alloc,
    const float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready,
    const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ req,
    int64_t tolerated,
    const int64_t* __restrict__ require,
    const int64_t* __restrict__ forbid,
    float w_least, float w_most, float w_bal,
    const float* __restrict__ dim_w, float wsum,
    const float* __restrict__ bias,
    int N, int R, int W)
{
    bool feasible = ready[i] != 0;
    feasible = feasible && ((taints[i] & ~tolerated) == 0);
    for (int w = 0; w < W; ++w) {
        int64_t p = planes[(size_t)w * N + i];
        feasible = feasible && ((p & require[w]) == require[w]);
        feasible = feasible && ((p & forbid[w]) == 0);
    }

    long long cap = BIG_CAP;
    float least = 0.f, most = 0.f, mean = 0.f;
    for (int r = 0; r < R; ++r) {
        size_t off = (size_t)r * N + i;
        float a = alloc[off];
        float u = used[off];
        float e = extra ? extra[off] : 0.f;
        float avail = a - u + e;
        float rq = req[r];
        // the fit test covers EVERY dim, as in the oracle: a node over-
        // committed (used > alloc) in a dim the class does not request
        // is still not a place to put more work
        feasible = feasible && (avail + EPS >= rq);
        if (rq > EPS) {
            float cc = (avail + EPS) / rq;     // clamp before the int
            if (cc > (float)BIG_CAP) cc = (float)BIG_CAP;  // cast: UB on inf
            long long c = (long long)floorf(cc);
            cap = min(cap, max(c, 0ll));
        }
        float f = fminf((u + rq) / fmaxf(a, EPS), 1.0f);
        float dw = dim_w[r];
        least += (1.0f - f) * dw;
        most += f * dw;
        mean += f;
    }
    mean /= (float)R;
    // balanced-allocation variance: second pass RECOMPUTES f instead
    // of staging a per-thread frac[] array (a fixed-size array caps R
    // and spills VGPRs; inputs are L2-resident so the re-read is
    // cheap, and the float op sequence is identical — bit-equal to
    // the torch oracle).  Skipped entirely when the weight is 0.
    float bal = 0.f;
    if (w_bal != 0.f) {
        float var = 0.f;
        for (int r = 0; r < R; ++r) {
            size_t off = (size_t)r * N + i;
            float f = fminf((used[off] + req[r]) /
                            fmaxf(alloc[off], EPS), 1.0f);
            float d = f - mean;
            var += d * d;
        }
        bal = 1.0f - sqrtf(var / (float)R);
    }
    float s = w_least * least / wsum + w_most * most / wsum + w_bal * bal;
    if (bias) s += bias[i];

    bool ok = feasible && cap > 0;
    NodeScore out;
    out.s = ok ? s : NEG_INF;
    out.cap = ok ? (int)min(cap, BIG_CAP) : 0;
    return out;
}

__device__ void score_pass(
    int start, int step,
    const float* __restrict__ alloc,
    const float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready,
    const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ req,
    int64_t tolerated,
    const int64_t* __restrict__ require,
    const int64_t* __restrict__ forbid,
    float w_least, float w_most, float w_bal,
    const float* __restrict__ dim_w,
    const float* __restrict__ bias,
    float* __restrict__ score_out,
    int* __restrict__ cap_out,
    int N, int R, int W)
{
    // req/dim_w are tiny and wave-uniform: scalar-cached by L1 automatically.
    float wsum = 0.f;
    for (int r = 0; r < R; ++r) wsum += dim_w[r];
    wsum = fmaxf(wsum, EPS);

    for (int i = start; i < N; i += step) {
        NodeScore ns = node_score_one(
            i, alloc, used, extra, ready, taints, planes, req, tolerated,
            require, forbid, w_least, w_most, w_bal, dim_w, wsum, bias,
            N, R, W);
        score_out[i] = ns.s;
        if (cap_out) cap_out[i] = ns.cap;
    }
}

__global__ void score_cap_kernel(
    const float* alloc, const float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score_out, int* cap_out,
    int N, int R, int W)
{
    score_pass(blockIdx.x * blockDim.x + threadIdx.x,
               gridDim.x * blockDim.x,
               alloc, used, extra, ready, taints, planes, req, tolerated,
               require, forbid, w_least, w_most, w_bal, dim_w, bias,
               score_out, cap_out, N, R, W);
}

// ---------------------------------------------------------------------------
// (value, index) argmax with ties -> lowest index, across a wave then a block.
// ---------------------------------------------------------------------------
struct ValIdx { float v; int i; };

DEVINL ValIdx better(ValIdx a, ValIdx b) {
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}

DEVINL ValIdx wave_reduce(ValIdx x) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        ValIdx o;
        o.v = __shfl_down(x.v, off);
        o.i = __shfl_down(x.i, off);
        x = better(x, o);
    }
    return x;
}

// queue quota -> instance budget of one class (proportion/capacity
// Allocatable check, session_plugins.go:405 — enforced exactly, on device).
// Serial over R: one thread calls it and publishes the result.
DEVINL long long dev_queue_budget(
    const float* __restrict__ req, const float* __restrict__ queue_limit,
    const float* __restrict__ queue_alloc, int ntasks, int R)
{
    long long quota = BIG_CAP;
    for (int r = 0; r < R; ++r) {
        float rq = req[r];
        if (rq > EPS) {
            float head = queue_limit[r] - queue_alloc[r];
            float qq = (head + EPS) / rq;
            if (qq > (float)BIG_CAP) qq = (float)BIG_CAP;
            long long q = (long long)floorf(qq);
            quota = min(quota, max(q, 0ll));
        }
    }
    return min((long long)ntasks, quota);
}

// count * req joins (sign > 0) or leaves (sign < 0) an accumulator in ONE
// rounding.  Spelled out so that every commit and every revert site of
// every kernel compiles the same operation, whatever the compiler would
// contract in that inlining context: the selects must leave bit-equal
// usage, and a revert must subtract exactly what its commit added.
DEVINL float acc_add(float acc, int count, float req) {
    return fmaf((float)count, req, acc);
}
DEVINL float acc_sub(float acc, int count, float req) {
    return fmaf(-(float)count, req, acc);
}

// Commit epilogue of every select (serial, bulk, spread), whole 1024-
// thread block: ONE count * req per log entry goes into `used` (a wave per
// entry), the class total into queue_alloc, then the counters are
// published.  All selects are log-first: nothing touches `used` or
// queue_alloc before this point, so a single-class gang that misses its
// minimum (fuse_min) is discarded by simply not calling it — no
// add-then-subtract, whose f32 result is not the starting value once
// usage comes in bytes.
DEVINL void dev_commit_log(
    const int* __restrict__ log_nodes, const int* __restrict__ log_counts,
    int len, int total, const float* __restrict__ req,
    float* __restrict__ used, float* __restrict__ queue_alloc,
    int* __restrict__ log_len, int* __restrict__ placed,
    int* __restrict__ job_placed, int N, int R)
{
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    for (int e = tid / WAVE; e < len; e += 1024 / WAVE) {
        int node = log_nodes[e];
        int cnt = log_counts[e];
        if (lane < R) {
            float* u = used + (size_t)lane * N + node;
            *u = acc_add(*u, cnt, req[lane]);
        }
    }
    if (tid < R) queue_alloc[tid] = acc_add(queue_alloc[tid], total, req[tid]);
    if (tid == 0) {
        *log_len = len;
        *placed = total;
        *job_placed += total;
    }
}

// ---------------------------------------------------------------------------
// K2 select + K4 gang-transactional placement for one task class.
//   ONE workgroup (1024 threads = 16 waves).  Iterative argmax over the
//   score vector with per-thread cached local maxima: after node b is
//   consumed only its owner thread rescans its stride (N/1024 elements,
//   L2-resident).  The loop only writes the undo log (it never reads
//   `used`); usage, queue_alloc and the job accounting are committed from
//   the log afterwards (dev_commit_log) — or not at all when the single-
//   class gang misses its minimum (fuse_min >= 0).
// ---------------------------------------------------------------------------
#define SC_THREADS 1024
#define SC_WAVES (SC_THREADS / WAVE)

__device__ void dev_select_commit(
    float* __restrict__ score,        // [N] (consumed: selected entries -> -inf)
    const int* __restrict__ cap,      // [N]
    const float* __restrict__ req,    // [R]
    int ntasks,
    float* __restrict__ used,         // [R, N] in place
    float* __restrict__ queue_alloc,  // [R] in place
    const float* __restrict__ queue_limit, // [R]
    int* __restrict__ log_nodes,      // [K]
    int* __restrict__ log_counts,     // [K]
    int* __restrict__ log_len,        // [1]
    int* __restrict__ placed,         // [1]
    int* __restrict__ job_placed,     // [1]
    int fuse_min,                     // >=0: single-class gang min (in-kernel revert)
    int N, int R, int K)
{
    __shared__ ValIdx s_wave[SC_WAVES];
    __shared__ ValIdx s_best;
    __shared__ int s_remaining;
    __shared__ int s_cursor;
    __shared__ int s_go;
    __shared__ long long s_budget;

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    if (tid == 0) {
        s_budget = dev_queue_budget(req, queue_limit, queue_alloc, ntasks, R);
        s_remaining = (int)min(s_budget, (long long)INT32_MAX);
        s_cursor = 0;
    }
    __syncthreads();

    // per-thread local argmax over the strided slice {tid, tid+1024, ...}
    ValIdx loc; loc.v = NEG_INF; loc.i = INT32_MAX;
    for (int i = tid; i < N; i += SC_THREADS) {
        ValIdx c; c.v = score[i]; c.i = i;
        loc = better(loc, c);
    }

    while (true) {
        // block argmax: wave shuffle reduce, then wave 0 reduces the 16
        ValIdx w = wave_reduce(loc);
        if (lane == 0) s_wave[wid] = w;
        __syncthreads();
        if (wid == 0) {
            ValIdx b; b.v = NEG_INF; b.i = INT32_MAX;
            if (lane < SC_WAVES) b = s_wave[lane];
            b = wave_reduce(b);
            // lane 0 of wave 0 IS thread 0, the only writer of
            // s_remaining/s_cursor: it decides "continue" here and
            // publishes it with the winner.  Other threads must not read
            // the two counters themselves — thread 0 updates them below
            // with no barrier in between, so a late wave could see the
            // post-update values and leave one iteration early.
            if (lane == 0) {
                s_best = b;
                s_go = (b.v != NEG_INF && s_remaining > 0 && s_cursor < K)
                    ? 1 : 0;
            }
        }
        __syncthreads();

        ValIdx best = s_best;
        if (!s_go) break;

        if (tid == 0) {
            const int take = min(cap[best.i], s_remaining);
            log_nodes[s_cursor] = best.i;
            log_counts[s_cursor] = take;
            s_cursor += 1;
            s_remaining -= take;
        }
        // knock out the chosen node; its owner rescans its slice
        if (tid == (best.i & (SC_THREADS - 1))) {
            score[best.i] = NEG_INF;
            loc.v = NEG_INF; loc.i = INT32_MAX;
            for (int i = tid; i < N; i += SC_THREADS) {
                ValIdx c; c.v = score[i]; c.i = i;
                loc = better(loc, c);
            }
        }
        __syncthreads();
    }

    __syncthreads();
    int total = (int)s_budget - s_remaining;
    bool revert = (fuse_min >= 0) && (total < fuse_min);

    const int cursor = s_cursor;

    if (revert) {
        // single-class gang failed (statement.go:375 Discard): nothing was
        // applied, the log keeps its nodes with zeroed counts
        for (int e = tid; e < cursor; e += SC_THREADS) log_counts[e] = 0;
        if (tid == 0) { *log_len = cursor; *placed = 0; }
    } else {
        dev_commit_log(log_nodes, log_counts, cursor, total, req, used,
                       queue_alloc, log_len, placed, job_placed, N, R);
    }
}

__global__ void __launch_bounds__(SC_THREADS)
select_commit_kernel(
    float* score, const int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    int fuse_min, int N, int R, int K)
{
    dev_select_commit(score, cap, req, ntasks, used, queue_alloc,
                      queue_limit, log_nodes, log_counts, log_len, placed,
                      job_placed, fuse_min, N, R, K);
}

// ---------------------------------------------------------------------------
// Fused score+select for small classes: ONE launch does the score pass
// (block-stride, 16 waves hide the L2 latency at small N) and the
// serial select.  Halves the per-class launch count on heterogeneous
// plans where the grid-stride score kernel was dispatch-latency bound
// (~12.5 us/class -> ~7 us measured on the mix bench).  Bit-identical
// math: same score_pass + dev_select_commit bodies.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SC_THREADS)
fused_score_select_kernel(
    const float* __restrict__ alloc, float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready, const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ req, int64_t tolerated,
    const int64_t* __restrict__ require, const int64_t* __restrict__ forbid,
    float w_least, float w_most, float w_bal,
    const float* __restrict__ dim_w, const float* __restrict__ bias,
    float* __restrict__ score, int* __restrict__ cap,
    int ntasks,
    float* __restrict__ queue_alloc, const float* __restrict__ queue_limit,
    int* __restrict__ log_nodes, int* __restrict__ log_counts,
    int* __restrict__ log_len, int* __restrict__ placed,
    int* __restrict__ job_placed, int fuse_min,
    int N, int R, int W, int K)
{
    score_pass(threadIdx.x, SC_THREADS, alloc, used, extra, ready, taints,
               planes, req, tolerated, require, forbid,
               w_least, w_most, w_bal, dim_w, bias, score, cap, N, R, W);
    __syncthreads();
    dev_select_commit(score, cap, req, ntasks, used, queue_alloc,
                      queue_limit, log_nodes, log_counts, log_len, placed,
                      job_placed, fuse_min, N, R, K);
}

// ---------------------------------------------------------------------------
// K4 gang readiness for multi-class jobs (JobReady AND-aggregation,
// session_plugins.go:483).  One tiny block.
// ---------------------------------------------------------------------------
DEVINL void dev_finalize_job(
    const int* job_placed, int occupied, int min_available,
    const int* class_placed, const int* class_min, uint8_t* flag, int nc)
{
    if (threadIdx.x == 0) {
        bool ok = (*job_placed + occupied) >= min_available;
        for (int c = 0; c < nc && ok; ++c)
            ok = class_placed[c] >= class_min[c];
        *flag = ok ? 1 : 0;
    }
}

__global__ void finalize_job_kernel(
    const int* __restrict__ job_placed,   // [1]
    int occupied, int min_available,
    const int* __restrict__ class_placed, // [nc] (slice)
    const int* __restrict__ class_min,    // [nc]
    uint8_t* __restrict__ flag,           // [1]
    int nc)
{
    dev_finalize_job(job_placed, occupied, min_available, class_placed,
                     class_min, flag, nc);
}

// ---------------------------------------------------------------------------
// K4 conditional rollback of one class, gated on the job's device flag.
// Block-scope (callers launch ONE block / run inside the megacycle).
// ---------------------------------------------------------------------------
__device__ void dev_cond_revert(
    const uint8_t* __restrict__ flag,  // [1] 1 = keep
    int* __restrict__ log_nodes,       // [K]
    int* __restrict__ log_counts,      // [K]
    const int* __restrict__ log_len,   // [1]
    const float* __restrict__ req,     // [R]
    float* __restrict__ used,          // [R, N]
    float* __restrict__ queue_alloc,   // [R]
    int* __restrict__ placed,          // [1]
    int* __restrict__ job_placed,      // [1]
    int N, int R)
{
    if (*flag) return;
    int len = *log_len;
    int tid = threadIdx.x;
    int lane_r = tid % WAVE;         // one wave per entry: R <= 64 dims
    int entry = tid / WAVE;
    int stride = blockDim.x / WAVE;
    for (int e = entry; e < len; e += stride) {
        int cnt = log_counts[e];
        if (cnt == 0) continue;
        int node = log_nodes[e];
        if (lane_r < R) {
            float* u = used + (size_t)lane_r * N + node;
            *u = acc_sub(*u, cnt, req[lane_r]);
        }
    }
    if (tid == 0) {
        int p = *placed;
        for (int r = 0; r < R; ++r)
            queue_alloc[r] = acc_sub(queue_alloc[r], p, req[r]);
        *job_placed -= p;
        *placed = 0;
    }
    // zero the counts after the subtraction pass completes
    __syncthreads();
    for (int e = threadIdx.x; e < len; e += blockDim.x) log_counts[e] = 0;
}

__global__ void cond_revert_kernel(
    const uint8_t* flag, int* log_nodes, int* log_counts,
    const int* log_len, const float* req, float* used, float* queue_alloc,
    int* placed, int* job_placed, int N, int R)
{
    dev_cond_revert(flag, log_nodes, log_counts, log_len, req, used,
                    queue_alloc, placed, job_placed, N, R);
}

// ---------------------------------------------------------------------------
// K2/K4 bulk select for mega-classes (gang bundles): the serial argmax
// loop above costs one block-reduce + owner rescan PER CONSUMED NODE
// (~10k sequential steps for a 100k-task bundle).  Scores are static
// within a class, so the fill equals "stable-sort nodes by score desc,
// take caps until the budget" — exactly the torch oracle
// (reference.py select_commit: argsort + cumsum + clamp).  This kernel
// computes that directly: a workgroup LSD radix sort (8 passes of 4-bit
// digits, rank-stable) followed by a chunked block scan that emits the
// undo log in sorted order.  One workgroup; ~16N global accesses total
// instead of ~N per consumed node.
// ---------------------------------------------------------------------------
#define BS_THREADS 1024
#define BS_WAVES (BS_THREADS / WAVE)   // 16
#define BS_DIGITS 16                   // 4-bit LSD
#define BS_PASSES 8

// monotonic float->uint map, then invert so ASCENDING key == score DESC
DEVINL unsigned score_key(float s) {
    unsigned u = __float_as_uint(s);
    // -0.0 == +0.0 for the oracle's stable sort and the serial argmax:
    // both zeros share one key so the index alone orders them
    if (u == 0x80000000u) u = 0u;
    unsigned m = (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ~(u ^ m);
}

__global__ void __launch_bounds__(BS_THREADS)
bulk_select_kernel(
    const float* __restrict__ score,       // [N]
    const int* __restrict__ cap,           // [N]
    const float* __restrict__ req,         // [R]
    int ntasks,
    float* __restrict__ used,              // [R, N] in place
    float* __restrict__ queue_alloc,       // [R] in place
    const float* __restrict__ queue_limit, // [R]
    int* __restrict__ log_nodes,           // [K]
    int* __restrict__ log_counts,          // [K]
    int* __restrict__ log_len,             // [1]
    int* __restrict__ placed,              // [1]
    int* __restrict__ job_placed,          // [1]
    int fuse_min,
    unsigned* __restrict__ scratch,        // [4N]: keys/ids ping-pong
    int N, int R, int K)
{
    __shared__ unsigned s_hist[BS_DIGITS * BS_THREADS];     // 64 KB
    __shared__ unsigned s_digit_base[BS_DIGITS];
    __shared__ long long s_budget;
    __shared__ long long s_carry_cap;      // running csum across chunks
    __shared__ int s_carry_log;            // running log-entry count
    __shared__ long long s_wave_ll[BS_WAVES];
    __shared__ int s_wave_i[BS_WAVES];

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    unsigned* keys_a = scratch;
    unsigned* ids_a = scratch + (size_t)N;
    unsigned* keys_b = scratch + 2 * (size_t)N;
    unsigned* ids_b = scratch + 3 * (size_t)N;

    if (tid == 0) {
        s_budget = dev_queue_budget(req, queue_limit, queue_alloc, ntasks, R);
        s_carry_cap = 0;
        s_carry_log = 0;
    }

    // -- build (key, id) pairs; array position i = node i (stable base) --
    for (int i = tid; i < N; i += BS_THREADS) {
        keys_a[i] = score_key(score[i]);
        ids_a[i] = (unsigned)i;
    }
    __syncthreads();

    // -- 8-pass LSD radix (each thread owns a CONTIGUOUS chunk: rank
    //    order inside a digit bin is (thread, position) = input order,
    //    which is what makes the sort stable) -------------------------------
    const int chunk = (N + BS_THREADS - 1) / BS_THREADS;
    const int lo = min(tid * chunk, N);
    const int hi = min(lo + chunk, N);

    for (int pass = 0; pass < BS_PASSES; ++pass) {
        unsigned* in_k = (pass & 1) ? keys_b : keys_a;
        unsigned* in_i = (pass & 1) ? ids_b : ids_a;
        unsigned* out_k = (pass & 1) ? keys_a : keys_b;
        unsigned* out_i = (pass & 1) ? ids_a : ids_b;
        const int shift = pass * 4;

        unsigned cnt[BS_DIGITS];
        for (int d = 0; d < BS_DIGITS; ++d) cnt[d] = 0;
        for (int i = lo; i < hi; ++i)
            cnt[(in_k[i] >> shift) & 15u]++;
        for (int d = 0; d < BS_DIGITS; ++d)
            s_hist[d * BS_THREADS + tid] = cnt[d];
        __syncthreads();

        // wave `wid` scans digit row `wid` (inclusive, 16 chunks of 64)
        {
            unsigned carry = 0;
            unsigned* row = s_hist + wid * BS_THREADS;
            for (int c = 0; c < BS_THREADS / WAVE; ++c) {
                unsigned v = row[c * WAVE + lane];
                for (int off = 1; off < WAVE; off <<= 1) {
                    unsigned o = __shfl_up(v, off);
                    if (lane >= off) v += o;
                }
                v += carry;
                row[c * WAVE + lane] = v;
                carry = __shfl(v, WAVE - 1);
            }
            if (lane == 0) s_digit_base[wid] = carry;   // digit total
        }
        __syncthreads();
        if (tid == 0) {
            unsigned run = 0;
            for (int d = 0; d < BS_DIGITS; ++d) {
                unsigned t = s_digit_base[d];
                s_digit_base[d] = run;
                run += t;
            }
        }
        __syncthreads();

        unsigned off[BS_DIGITS];
        for (int d = 0; d < BS_DIGITS; ++d)
            off[d] = s_digit_base[d] + s_hist[d * BS_THREADS + tid] - cnt[d];
        for (int i = lo; i < hi; ++i) {
            unsigned k = in_k[i];
            unsigned d = (k >> shift) & 15u;
            unsigned p = off[d]++;
            out_k[p] = k;
            out_i[p] = in_i[i];
        }
        __syncthreads();
    }
    // even pass count -> sorted result is back in keys_a / ids_a

    // -- chunked block scan over the sorted order: cumulative caps ->
    //    per-position take, log compaction, usage commit ---------------------
    const long long budget = s_budget;
    const int nchunks = (N + BS_THREADS - 1) / BS_THREADS;
    long long total_ll = 0;

    for (int c = 0; c < nchunks; ++c) {
        int j = c * BS_THREADS + tid;
        long long cj = 0;
        int node = -1;
        if (j < N) {
            node = (int)ids_a[j];
            float s = score[node];
            if (s != NEG_INF) cj = (long long)cap[node];
        }
        // block inclusive scan of cj (wave scan + cross-wave offsets)
        long long v = cj;
        for (int off = 1; off < WAVE; off <<= 1) {
            long long o = __shfl_up(v, off);
            if (lane >= off) v += o;
        }
        if (lane == WAVE - 1) s_wave_ll[wid] = v;
        __syncthreads();
        if (wid == 0) {
            long long w = (lane < BS_WAVES) ? s_wave_ll[lane] : 0;
            for (int off = 1; off < BS_WAVES; off <<= 1) {
                long long o = __shfl_up(w, off);
                if (lane >= off) w += o;
            }
            if (lane < BS_WAVES) s_wave_ll[lane] = w;
        }
        __syncthreads();
        long long csum = v + (wid > 0 ? s_wave_ll[wid - 1] : 0) + s_carry_cap;

        long long over = csum - budget; if (over < 0) over = 0;
        long long take_ll = cj - over; if (take_ll < 0) take_ll = 0;
        int take = (int)take_ll;
        int flag = take > 0 ? 1 : 0;

        // block inclusive scan of flags -> log slot
        int f = flag;
        for (int off = 1; off < WAVE; off <<= 1) {
            int o = __shfl_up(f, off);
            if (lane >= off) f += o;
        }
        if (lane == WAVE - 1) s_wave_i[wid] = f;
        __syncthreads();
        if (wid == 0) {
            int w = (lane < BS_WAVES) ? s_wave_i[lane] : 0;
            for (int off = 1; off < BS_WAVES; off <<= 1) {
                int o = __shfl_up(w, off);
                if (lane >= off) w += o;
            }
            if (lane < BS_WAVES) s_wave_i[lane] = w;
        }
        __syncthreads();
        int fsum = f + (wid > 0 ? s_wave_i[wid - 1] : 0) + s_carry_log;

        if (flag && fsum - 1 < K) {
            log_nodes[fsum - 1] = node;
            log_counts[fsum - 1] = take;
        }
        __syncthreads();
        if (tid == BS_THREADS - 1) {
            s_carry_cap = csum;
            s_carry_log = fsum;
        }
        __syncthreads();
    }
    total_ll = min(s_carry_cap, budget);
    int total = (int)total_ll;
    int m = min(s_carry_log, K);
    bool revert = (fuse_min >= 0) && (total < fuse_min);

    if (revert) {
        // gang can't reach its minimum: nothing is applied; the log keeps
        // zeroed counts (same end state as the serial kernel's discard)
        for (int e = tid; e < m; e += BS_THREADS) log_counts[e] = 0;
        if (tid == 0) { *log_len = m; *placed = 0; }
        return;
    }
    // commit: apply the logged takes to the staged usage
    dev_commit_log(log_nodes, log_counts, m, total, req, used, queue_alloc,
                   log_len, placed, job_placed, N, R);
}

// ---------------------------------------------------------------------------
// K2 select under a topology-spread constraint (maxSkew, DoNotSchedule),
// enforced before EVERY placement — oracle: reference.py
// spread_select_commit.  Scores are static within the class, but a node
// is eligible only while count[its domain] + 1 - min(count) <= max_skew,
// and every placement moves a count, so the fill is a true per-instance
// loop (bounded by the budget):
//
//   * head[d] caches the best remaining node of domain d as one 64-bit
//     key (ordered score << 32 | ~index): the larger key is the better
//     score, ties the lower index.  0 = domain has no node left.
//   * one iteration = one pass over the D domains (count + head per
//     domain, O(D/1024) per thread) feeding ONE block reduce that yields
//     the best eligible head and n0 = #domains sitting at the minimum m.
//     Thread 0 places one instance and advances m when the placement
//     took the last domain off the minimum (n0 == 1) — no second reduce.
//   * a head is rescanned (O(N/1024) per thread) only when its node's
//     remaining capacity reaches 0.
//
// Barrier conventions of dev_select_commit: thread 0 owns every counter
// and publishes go/rescan together; loop exits are read block-uniformly
// after a barrier; no barrier under divergent control flow.
// `score` and `cap` are consumed (cap counts down, used-up nodes -> -inf);
// `used` takes ONE (float)count * req per log entry after the loop, which
// is what keeps it bit-equal to the oracle.
// ---------------------------------------------------------------------------
#define SP_THREADS 1024
#define SP_WAVES (SP_THREADS / WAVE)

DEVINL unsigned long long spread_key(float s, int i) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;              // -0.0 ties with +0.0
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;  // ascending in the score
    return ((unsigned long long)u << 32) | (0xFFFFFFFFu - (unsigned)i);
}

DEVINL int spread_key_node(unsigned long long k) {
    return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
}

DEVINL unsigned long long head_load(unsigned long long* h) {
    return __hip_atomic_load(h, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
}

// keys only grow between two resets, so a stale read can only let a
// redundant atomic through, never drop a better key
DEVINL void head_offer(unsigned long long* h, unsigned long long k) {
    if (k > head_load(h))
        __hip_atomic_fetch_max(h, k, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
}

DEVINL unsigned long long wave_max_u64(unsigned long long x) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        unsigned long long o = __shfl_down(x, off);
        x = o > x ? o : x;
    }
    return x;
}

__global__ void __launch_bounds__(SP_THREADS)
spread_select_kernel(
    float* __restrict__ score,        // [N] consumed
    int* __restrict__ cap,            // [N] consumed (remaining capacity)
    const float* __restrict__ req,    // [R]
    int ntasks,
    float* __restrict__ used,         // [R, N] in place
    float* __restrict__ queue_alloc,  // [R] in place
    const float* __restrict__ queue_limit, // [R]
    int* __restrict__ log_nodes,      // [K]
    int* __restrict__ log_counts,     // [K]
    int* __restrict__ log_len,        // [1]
    int* __restrict__ placed,         // [1]
    int* __restrict__ job_placed,     // [1]
    const int* __restrict__ dom_of,   // [N] domain id, -1 = unlabeled
    int* __restrict__ dom_count,      // [D] in place
    int D, int max_skew, int fuse_min,
    unsigned long long* __restrict__ head,  // [D] scratch
    int* __restrict__ slot,           // [N] scratch: node -> log entry
    int N, int R, int K)
{
    __shared__ unsigned long long s_wkey[SP_WAVES];
    __shared__ int s_wint[SP_WAVES];
    __shared__ int s_budget;
    __shared__ int s_m;         // min(dom_count) for the coming iteration
    __shared__ int s_cursor;
    __shared__ int s_total;
    __shared__ int s_go;
    __shared__ int s_rescan;    // domain whose head must be rebuilt, or -1

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    if (tid == 0) {
        long long b = dev_queue_budget(req, queue_limit, queue_alloc, ntasks,
                                       R);
        s_budget = (D > 0 && b > 0) ? (int)b : 0;
        s_cursor = 0;
        s_total = 0;
    }
    for (int d = tid; d < D; d += SP_THREADS) head[d] = 0ull;
    __syncthreads();

    // nodes that can never take an instance leave the score vector; the
    // others offer themselves as their domain's head
    for (int i = tid; i < N; i += SP_THREADS) {
        slot[i] = -1;
        float s = score[i];
        int d = dom_of[i];
        if (s > NEG_INF && d >= 0 && d < D && cap[i] > 0)
            head_offer(head + d, spread_key(s, i));
        else
            score[i] = NEG_INF;
    }
    {
        int lmin = INT32_MAX;
        for (int d = tid; d < D; d += SP_THREADS)
            lmin = min(lmin, dom_count[d]);
        for (int off = WAVE / 2; off > 0; off >>= 1)
            lmin = min(lmin, __shfl_down(lmin, off));
        if (lane == 0) s_wint[wid] = lmin;
    }
    __syncthreads();
    if (tid == 0) {
        int m = INT32_MAX;
        for (int w = 0; w < SP_WAVES; ++w) m = min(m, s_wint[w]);
        s_m = m;
    }
    __syncthreads();

    const int budget = s_budget;
    for (int it = 0; it < budget; ++it) {
        const int m = s_m;
        unsigned long long loc = 0ull;
        int n0 = 0;
        for (int d = tid; d < D; d += SP_THREADS) {
            int c = dom_count[d];
            unsigned long long k = head_load(head + d);
            n0 += (c == m) ? 1 : 0;
            if (c + 1 - m <= max_skew && k > loc) loc = k;
        }
        loc = wave_max_u64(loc);
        for (int off = WAVE / 2; off > 0; off >>= 1)
            n0 += __shfl_down(n0, off);
        if (lane == 0) { s_wkey[wid] = loc; s_wint[wid] = n0; }
        __syncthreads();
        if (wid == 0) {
            // 16 per-wave partials on lanes 0..15: four steps reach lane 0
            unsigned long long k = lane < SP_WAVES ? s_wkey[lane] : 0ull;
            int nm = lane < SP_WAVES ? s_wint[lane] : 0;
            for (int off = SP_WAVES / 2; off > 0; off >>= 1) {
                unsigned long long o = __shfl_down(k, off);
                k = o > k ? o : k;
                nm += __shfl_down(nm, off);
            }
            // lane 0 of wave 0 is thread 0, the only writer of the
            // counters, the log, dom_count, cap and the head resets
            if (lane == 0) {
                int go = 0, rescan = -1;
                if (k != 0ull) {
                    const int node = spread_key_node(k);
                    int sl = slot[node];
                    if (sl >= 0 || s_cursor < K) {
                        go = 1;
                        const int d = dom_of[node];
                        const int c = dom_count[d];
                        dom_count[d] = c + 1;
                        // the last domain at the minimum moved up
                        if (c == m && nm == 1) s_m = m + 1;
                        if (sl < 0) {
                            sl = s_cursor;
                            s_cursor = sl + 1;
                            slot[node] = sl;
                            log_nodes[sl] = node;
                            log_counts[sl] = 1;
                        } else {
                            log_counts[sl] += 1;
                        }
                        const int left = cap[node] - 1;
                        cap[node] = left;
                        if (left <= 0) {
                            score[node] = NEG_INF;
                            __hip_atomic_store(head + d, 0ull,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                            rescan = d;
                        }
                        s_total += 1;
                    }
                }
                s_go = go;
                s_rescan = rescan;
            }
        }
        __syncthreads();
        if (!s_go) break;            // block-uniform
        const int rd = s_rescan;     // block-uniform
        if (rd >= 0) {
            unsigned long long best = 0ull;
            for (int i = tid; i < N; i += SP_THREADS) {
                if (dom_of[i] == rd) {
                    float s = score[i];
                    if (s > NEG_INF) {
                        unsigned long long k = spread_key(s, i);
                        if (k > best) best = k;
                    }
                }
            }
            best = wave_max_u64(best);
            if (lane == 0 && best != 0ull) head_offer(head + rd, best);
            __syncthreads();
        }
    }

    __syncthreads();
    const int total = s_total;
    const int cursor = s_cursor;
    const bool revert = (fuse_min >= 0) && (total < fuse_min);

    if (revert) {
        // single-class gang failed: nothing was applied to `used` yet;
        // give the placements back to the group's domain counts
        for (int e = tid; e < cursor; e += SP_THREADS) {
            atomicSub(dom_count + dom_of[log_nodes[e]], log_counts[e]);
            log_counts[e] = 0;
        }
        if (tid == 0) { *log_len = cursor; *placed = 0; }
    } else {
        dev_commit_log(log_nodes, log_counts, cursor, total, req, used,
                       queue_alloc, log_len, placed, job_placed, N, R);
    }
}

// cond_revert for a spread class: the same rollback, plus the logged
// placements leave the group's per-domain counts (integer atomics)
__global__ void spread_revert_kernel(
    const uint8_t* flag, int* log_nodes, int* log_counts,
    const int* log_len, const float* req, float* used, float* queue_alloc,
    int* placed, int* job_placed, const int* __restrict__ dom_of,
    int* __restrict__ dom_count, int D, int N, int R)
{
    if (!*flag) {
        const int len = *log_len;
        for (int e = threadIdx.x; e < len; e += blockDim.x) {
            int cnt = log_counts[e];
            if (cnt == 0) continue;
            int d = dom_of[log_nodes[e]];
            if (d >= 0 && d < D) atomicSub(dom_count + d, cnt);
        }
    }
    __syncthreads();
    dev_cond_revert(flag, log_nodes, log_counts, log_len, req, used,
                    queue_alloc, placed, job_placed, N, R);
}

// ---------------------------------------------------------------------------
// Inter-pod (anti-)affinity over a topology key, enforced before EVERY
// placement — oracle: reference.py affinity_select_commit.  Unlike spread
// this needs no per-instance loop: for both modes the per-placement rule
// collapses into a static mask over score/cap, computed once per class
// from the live per-domain counts, after which the ordinary select_commit
// (serial or bulk) yields the sequential result, log order included.
//
//   * affinity: placing into an eligible domain never changes the eligible
//     set; only the anchor (first member of an empty group) does.  So:
//     hosting = #domains with count > 0 (counts are >= 0 — every revert
//     takes back exactly what its own log added — so this is zero iff the
//     sum of the counts is); if 0, the anchor is the domain of
//     the block argmax over placeable nodes (ties -> lower index); every
//     node of a domain that is neither hosting nor the anchor is masked.
//   * anti: "best eligible node, then its domain closes" repeated equals
//     "the best node of each open domain, capacity 1, in score order".
//     Heads are 64-bit keys as in spread_select_kernel (atomicMax behind a
//     filtering read, only for domains with count == 0); a node stays iff
//     its key is its domain's head.
//
// A masked node gets score = -inf AND cap = 0; a kept node always has
// score > -inf, cap > 0 and 0 <= dom < D.  ONE workgroup: the argmax and
// the heads need a block-wide result before the mask pass, and a class's
// score vector is L2-resident (4 B/node).  Barriers sit only under
// block-uniform conditions (mode is a launch argument, s_hosting is read
// after a barrier); thread 0 publishes the anchor.
// `head` is D 64-bit words of scratch (anti mode only).
// ---------------------------------------------------------------------------
#define DM_AFFINITY 1
#define DM_ANTI 2

__global__ void __launch_bounds__(SP_THREADS)
domain_mask_kernel(
    float* __restrict__ score,            // [N] in place
    int* __restrict__ cap,                // [N] in place
    const int* __restrict__ dom_of,       // [N] domain id, -1 = unlabeled
    const int* __restrict__ dom_count,    // [D]
    int D, int mode,
    unsigned long long* __restrict__ head,  // [D] scratch (anti)
    int N)
{
    __shared__ ValIdx s_wave[SP_WAVES];
    __shared__ int s_wint[SP_WAVES];
    __shared__ int s_hosting;
    __shared__ int s_anchor;

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    if (mode == DM_AFFINITY) {
        int h = 0;
        for (int d = tid; d < D; d += SP_THREADS)
            h += dom_count[d] > 0 ? 1 : 0;
        for (int off = WAVE / 2; off > 0; off >>= 1)
            h += __shfl_down(h, off);
        if (lane == 0) s_wint[wid] = h;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < SP_WAVES; ++w) t += s_wint[w];
            s_hosting = t;
            s_anchor = -1;
        }
        __syncthreads();
        const bool need_anchor = s_hosting == 0;    // block-uniform
        if (need_anchor) {
            ValIdx loc; loc.v = NEG_INF; loc.i = INT32_MAX;
            for (int i = tid; i < N; i += SP_THREADS) {
                const int d = dom_of[i];
                if (d >= 0 && d < D && cap[i] > 0) {
                    ValIdx c; c.v = score[i]; c.i = i;
                    loc = better(loc, c);
                }
            }
            ValIdx w = wave_reduce(loc);
            if (lane == 0) s_wave[wid] = w;
            __syncthreads();
            if (wid == 0) {
                ValIdx b; b.v = NEG_INF; b.i = INT32_MAX;
                if (lane < SP_WAVES) b = s_wave[lane];
                b = wave_reduce(b);
                if (lane == 0)
                    s_anchor = (b.v != NEG_INF && b.i >= 0 && b.i < N)
                        ? dom_of[b.i] : -1;
            }
            __syncthreads();
        }
        const int anchor = s_anchor;
        for (int i = tid; i < N; i += SP_THREADS) {
            const int d = dom_of[i];
            bool keep = d >= 0 && d < D && cap[i] > 0 && score[i] > NEG_INF;
            if (keep) keep = dom_count[d] > 0 || d == anchor;
            if (!keep) { score[i] = NEG_INF; cap[i] = 0; }
        }
        return;
    }

    // anti-affinity: one head per open domain
    for (int d = tid; d < D; d += SP_THREADS) head[d] = 0ull;
    __syncthreads();
    for (int i = tid; i < N; i += SP_THREADS) {
        const int d = dom_of[i];
        const float s = score[i];
        if (d >= 0 && d < D && cap[i] > 0 && s > NEG_INF
                && dom_count[d] == 0)
            head_offer(head + d, spread_key(s, i));
    }
    __syncthreads();
    for (int i = tid; i < N; i += SP_THREADS) {
        const int d = dom_of[i];
        const float s = score[i];
        bool keep = d >= 0 && d < D && cap[i] > 0 && s > NEG_INF
            && dom_count[d] == 0;
        if (keep) keep = head_load(head + d) == spread_key(s, i);
        if (keep) cap[i] = 1;
        else { score[i] = NEG_INF; cap[i] = 0; }
    }
}

// After the select of an affinity / anti-affinity class: the logged
// placements join the group's per-domain counts.  Integer atomics — log
// entries can share a domain.  A fused gang revert leaves zeroed counts in
// the log, so it adds nothing.
__global__ void domain_count_add_kernel(
    const int* __restrict__ log_nodes, const int* __restrict__ log_counts,
    const int* __restrict__ log_len, const int* __restrict__ dom_of,
    int* __restrict__ dom_count, int D, int N, int K)
{
    int len = *log_len;
    if (len > K) len = K;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < len;
         e += gridDim.x * blockDim.x) {
        const int cnt = log_counts[e];
        const int node = log_nodes[e];
        if (cnt <= 0 || node < 0 || node >= N) continue;
        const int d = dom_of[node];
        if (d >= 0 && d < D) atomicAdd(dom_count + d, cnt);
    }
}

// ---------------------------------------------------------------------------
// Megacycle: a WHOLE small-class plan in ONE launch.  Heterogeneous
// inventories produce thousands of per-job classes; at ~2 enqueues per
// class the cycle becomes launch-bound.  This kernel sequences the
// per-job kernel bodies device-side (score -> select -> gang
// finalize/revert), preserving the exact sequential semantics: one
// workgroup, every class sees the previous classes' staged usage.
// Dispatched only when no class takes the bulk path (cycle_runner).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SC_THREADS)
megacycle_kernel(
    const VamdClassDesc* __restrict__ classes,   // [C] (device copy)
    const VamdJobDesc* __restrict__ jobs,        // [J] (device copy)
    int n_jobs,
    const float* __restrict__ alloc, float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready, const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ bias, const float* __restrict__ bias_rows,
    const float* __restrict__ class_req,        // [C, R]
    const int64_t* __restrict__ class_tol,      // [C] (device copy)
    const int64_t* __restrict__ class_require,  // [C, W]
    const int64_t* __restrict__ class_forbid,   // [C, W]
    const int32_t* __restrict__ class_min,      // [C]
    const float* __restrict__ dim_w,
    float* __restrict__ queue_alloc, const float* __restrict__ queue_limit,
    float* __restrict__ score, int* __restrict__ cap,
    int* __restrict__ log_nodes, int* __restrict__ log_counts,
    int* __restrict__ log_len, int* __restrict__ class_placed,
    int* __restrict__ job_placed, uint8_t* __restrict__ job_flag,
    int N, int R, int W)
{
    const int tid = threadIdx.x;
    for (int j = 0; j < n_jobs; ++j) {
        const VamdJobDesc jd = jobs[j];
        const int nc = jd.class_end - jd.class_begin;
        const bool single = (nc == 1);

        for (int c = jd.class_begin; c < jd.class_end; ++c) {
            const VamdClassDesc cd = classes[c];
            const VamdClassPlanes pl =
                class_planes(cd, extra, bias, bias_rows, N);

            score_pass(tid, SC_THREADS, alloc, used, pl.ext, ready, taints,
                       planes, class_req + (size_t)c * R, class_tol[c],
                       class_require + (size_t)c * W,
                       class_forbid + (size_t)c * W,
                       cd.w_least, cd.w_most, cd.w_bal, dim_w, pl.bias,
                       score, cap, N, R, W);
            __syncthreads();

            const int fuse_min = single ? gang_fuse_min(jd, cd) : -1;
            dev_select_commit(score, cap, class_req + (size_t)c * R,
                              cd.ntasks, used,
                              queue_alloc + (size_t)cd.queue_idx * R,
                              queue_limit + (size_t)cd.queue_idx * R,
                              log_nodes + cd.log_off,
                              log_counts + cd.log_off,
                              log_len + c, class_placed + c, job_placed + j,
                              fuse_min, N, R, cd.log_cap);
            __syncthreads();
        }

        if (!single) {
            dev_finalize_job(job_placed + j, jd.occupied, jd.min_available,
                             class_placed + jd.class_begin,
                             class_min + jd.class_begin, job_flag + j, nc);
            __syncthreads();
            for (int c = jd.class_begin; c < jd.class_end; ++c) {
                const VamdClassDesc cd = classes[c];
                dev_cond_revert(job_flag + j, log_nodes + cd.log_off,
                                log_counts + cd.log_off, log_len + c,
                                class_req + (size_t)c * R, used,
                                queue_alloc + (size_t)cd.queue_idx * R,
                                class_placed + c, job_placed + j, N, R);
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Chain path for many-small-class plans (heterogeneous mixes).  The
// per-class pipeline pays 2 launches + a serial under-occupied score
// pass per class (~10k classes in a mixed inventory).  Here a CHUNK of
// consecutive single-class jobs runs as TWO launches:
//
//   1. batch_score_kernel — scores ALL classes of the chunk against the
//      usage at chunk start, one class per blockIdx.y, filling the chip
//      (the [C,R]x[R,N] pass; L2-resident node planes make it bandwidth-
//      trivial).
//   2. select_chain_kernel — one workgroup replays the selects in job
//      order with LAZY EXACT re-scoring: a node whose usage changed
//      since the chunk snapshot ("touched") is re-scored live via the
//      same node_score_one; untouched nodes' snapshot scores ARE their
//      live scores.  The merged argmax is therefore bit-identical to
//      re-scoring every class against live usage — the chain is a pure
//      optimization, decisions match the per-class path and the torch
//      oracle exactly.
//
// Reference semantics covered: allocate.go:719-866 per-job sequential
// order; statement.go gang revert fused per single-class job.
// ---------------------------------------------------------------------------
__global__ void batch_score_kernel(
    const VamdClassDesc* __restrict__ classes,   // [C] device
    int c0,
    const float* __restrict__ alloc, const float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready, const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ bias, const float* __restrict__ bias_rows,
    const float* __restrict__ class_req, const int64_t* __restrict__ class_tol,
    const int64_t* __restrict__ class_require,
    const int64_t* __restrict__ class_forbid,
    const float* __restrict__ dim_w,
    float* __restrict__ score_buf,               // [chunk, N]
    int N, int R, int W)
{
    const int c = c0 + blockIdx.y;
    const VamdClassDesc cd = classes[c];
    const VamdClassPlanes pl = class_planes(cd, extra, bias, bias_rows, N);
    score_pass(blockIdx.x * blockDim.x + threadIdx.x,
               gridDim.x * blockDim.x,
               alloc, used, pl.ext, ready, taints, planes,
               class_req + (size_t)c * R, class_tol[c],
               class_require + (size_t)c * W,
               class_forbid + (size_t)c * W,
               cd.w_least, cd.w_most, cd.w_bal, dim_w, pl.bias,
               score_buf + (size_t)blockIdx.y * N, nullptr, N, R, W);
}

#define CH_THREADS 256
#define CH_WAVES (CH_THREADS / WAVE)
#define CH_TOPK 16

// Per-class top-K candidates by snapshot score (desc, ties → lower
// index), computed in PARALLEL across the chunk (one block per class)
// so the serial select chain never scans the full node row in the
// common case: the best untouched node is the first untouched entry of
// the candidate list.  Chosen entries are knocked out of the row
// (-inf) — the chain handles them via the candidate list / touched set,
// and the rare fallback scan only needs the remaining nodes.
__global__ void __launch_bounds__(SC_THREADS)
topk_kernel(
    float* __restrict__ score_buf,        // [chunk, N] (chosen -> -inf)
    float* __restrict__ topk_vals,        // [chunk, CH_TOPK]
    int* __restrict__ topk_ids,           // [chunk, CH_TOPK]
    int N)
{
    __shared__ ValIdx s_wave[SC_WAVES];
    __shared__ ValIdx s_best;
    float* row = score_buf + (size_t)blockIdx.x * N;
    float* tv = topk_vals + (size_t)blockIdx.x * CH_TOPK;
    int* ti = topk_ids + (size_t)blockIdx.x * CH_TOPK;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    ValIdx loc; loc.v = NEG_INF; loc.i = INT32_MAX;
    for (int i = tid; i < N; i += SC_THREADS) {
        ValIdx c; c.v = row[i]; c.i = i;
        loc = better(loc, c);
    }
    for (int k = 0; k < CH_TOPK; ++k) {
        ValIdx w = wave_reduce(loc);
        if (lane == 0) s_wave[wid] = w;
        __syncthreads();
        if (wid == 0) {
            ValIdx b; b.v = NEG_INF; b.i = INT32_MAX;
            if (lane < SC_WAVES) b = s_wave[lane];
            b = wave_reduce(b);
            if (lane == 0) s_best = b;
        }
        __syncthreads();
        ValIdx best = s_best;
        if (tid == 0) { tv[k] = best.v; ti[k] = best.i; }
        if (best.v == NEG_INF) {
            // fill the tail so the chain's walk can stop at -inf
            if (tid == 0)
                for (int t = k; t < CH_TOPK; ++t) { tv[t] = NEG_INF; ti[t] = INT32_MAX; }
            return;
        }
        if (tid == (best.i & (SC_THREADS - 1))) {
            row[best.i] = NEG_INF;
            loc.v = NEG_INF; loc.i = INT32_MAX;
            for (int i = tid; i < N; i += SC_THREADS) {
                ValIdx c; c.v = row[i]; c.i = i;
                loc = better(loc, c);
            }
        }
        __syncthreads();
    }
}

// 256 threads / 4 waves: enough waves to hide the L2 latency of the
// touched-list re-scoring (one wave measured 5x slower — latency
// bound), small enough that the three per-pop barriers stay cheap.
// Scalar decisions (budget/cap/take) are computed REDUNDANTLY by every
// thread from the same memory — uniform by construction, no broadcast
// barrier needed; the cross-wave argmax merge is one LDS write + one
// barrier + a 4-entry sequential merge on every thread.
__global__ void __launch_bounds__(CH_THREADS)
select_chain_kernel(
    const VamdClassDesc* __restrict__ classes,   // [C] device
    const VamdJobDesc* __restrict__ jobs,        // [J] device
    int c0, int c1,
    const float* __restrict__ alloc, float* __restrict__ used,
    const float* __restrict__ extra,
    const uint8_t* __restrict__ ready, const int64_t* __restrict__ taints,
    const int64_t* __restrict__ planes,
    const float* __restrict__ bias, const float* __restrict__ bias_rows,
    const float* __restrict__ class_req, const int64_t* __restrict__ class_tol,
    const int64_t* __restrict__ class_require,
    const int64_t* __restrict__ class_forbid,
    const float* __restrict__ dim_w,
    float* __restrict__ queue_alloc, const float* __restrict__ queue_limit,
    float* __restrict__ score_buf,               // [c1-c0, N] snapshot scores
    const float* __restrict__ topk_vals,         // [c1-c0, CH_TOPK]
    const int* __restrict__ topk_ids,            // [c1-c0, CH_TOPK]
    int* __restrict__ log_nodes, int* __restrict__ log_counts,
    int* __restrict__ log_len, int* __restrict__ class_placed,
    int* __restrict__ job_placed,
    uint8_t* __restrict__ touched,               // [N] scratch (reset here)
    int* __restrict__ touched_list,              // [N] scratch
    int N, int R, int W)
{
    __shared__ ValIdx s_wave[CH_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;

    // touched set is relative to THIS chunk's score snapshot
    for (int i = tid; i < N; i += CH_THREADS) touched[i] = 0;
    int tcount = 0;                 // block-uniform (all threads mirror it)
    __syncthreads();

    float wsum = 0.f;
    for (int r = 0; r < R; ++r) wsum += dim_w[r];
    wsum = fmaxf(wsum, EPS);

    for (int c = c0; c < c1; ++c) {
        const VamdClassDesc cd = classes[c];
        const VamdJobDesc jd = jobs[cd.job_idx];
        const float* req = class_req + (size_t)c * R;
        const VamdClassPlanes pl = class_planes(cd, extra, bias, bias_rows, N);
        const float* ext = pl.ext;
        const float* b = pl.bias;
        const float* row = score_buf + (size_t)(c - c0) * N;
        float* qa = queue_alloc + (size_t)cd.queue_idx * R;
        const float* ql = queue_limit + (size_t)cd.queue_idx * R;
        int* ln = log_nodes + cd.log_off;
        int* lc = log_counts + cd.log_off;
        const int K = cd.log_cap;
        const int fuse = gang_fuse_min(jd, cd);

        // queue quota (dev_queue_budget, lane-parallel) — per-dim
        // candidates on lanes < R, wave min-reduce
        // (sequential dependent L2 loads cost ~300 ns each; the wave does
        // them in one round).  Every wave computes the same values from
        // the same memory → block-uniform without a barrier.
        long long qcand = BIG_CAP;
        if (lane < R) {
            float rq = req[lane];
            if (rq > EPS) {
                float head = ql[lane] - qa[lane];
                float qq = (head + EPS) / rq;
                if (qq > (float)BIG_CAP) qq = (float)BIG_CAP;
                long long q = (long long)floorf(qq);
                qcand = max(q, 0ll);
            }
        }
        for (int off = WAVE / 2; off > 0; off >>= 1)
            qcand = min(qcand, (long long)__shfl_down((long long)qcand, off));
        const long long quota = __shfl((long long)qcand, 0);
        const long long budget = min((long long)cd.ntasks, quota);
        int remaining = (int)min(budget, (long long)INT32_MAX);
        int cursor = 0;
        const float* tv = topk_vals + (size_t)(c - c0) * CH_TOPK;
        const int* ti = topk_ids + (size_t)(c - c0) * CH_TOPK;

        while (remaining > 0 && cursor < K) {
            // stale side: first UNTOUCHED candidate of the top-K list is
            // exactly the best untouched node (every node outside the
            // list scores <= the last candidate).  Lanes load the list in
            // parallel; a ballot finds the first untouched entry — the
            // serial walk paid ~16 dependent L2 loads here.
            float kv = NEG_INF;
            int ki = INT32_MAX;
            bool feas = false, ok = false;
            if (lane < CH_TOPK) {
                kv = tv[lane];
                ki = ti[lane];
                feas = (kv != NEG_INF);
                ok = feas && !touched[ki];
            }
            uint64_t m_ok = __ballot(ok);
            uint64_t m_feas = __ballot(feas);
            ValIdx stale; stale.v = NEG_INF; stale.i = INT32_MAX;
            bool fallback = false;
            if (m_ok != 0) {
                int pos = __ffsll((unsigned long long)m_ok) - 1;
                stale.v = __shfl(kv, pos);
                stale.i = __shfl(ki, pos);
            } else if ((m_feas & ((1ull << CH_TOPK) - 1))
                       == ((1ull << CH_TOPK) - 1)) {
                // all CH_TOPK candidates feasible AND touched: the best
                // untouched (if any) is below the list — full row scan
                fallback = true;
            }
            ValIdx loc; loc.v = NEG_INF; loc.i = INT32_MAX;
            if (fallback) {
                for (int i = tid; i < N; i += CH_THREADS) {
                    if (!touched[i]) {
                        ValIdx cnd; cnd.v = row[i]; cnd.i = i;
                        loc = better(loc, cnd);
                    }
                }
            }
            loc = better(loc, stale);   // uniform: merges identically
            // touched side: live re-score (usage changed since snapshot)
            for (int k = tid; k < tcount; k += CH_THREADS) {
                int i = touched_list[k];
                bool consumed = false;       // already taken by THIS class
                for (int e = 0; e < cursor; ++e)
                    if (ln[e] == i) { consumed = true; break; }
                if (consumed) continue;
                NodeScore ns = node_score_one(
                    i, alloc, used, ext, ready, taints, planes, req,
                    class_tol[c], class_require + (size_t)c * W,
                    class_forbid + (size_t)c * W,
                    cd.w_least, cd.w_most, cd.w_bal, dim_w, wsum, b,
                    N, R, W);
                ValIdx cnd; cnd.v = ns.s; cnd.i = i;
                loc = better(loc, cnd);
            }
            ValIdx w = wave_reduce(loc);
            if (lane == 0) s_wave[wid] = w;
            __syncthreads();                      // barrier 1
            ValIdx best = s_wave[0];              // 4-entry merge, uniform
            for (int q = 1; q < CH_WAVES; ++q) best = better(best, s_wave[q]);
            if (best.v == NEG_INF) break;

            // live capacity of the chosen node: per-dim candidates on
            // lanes < R, wave min-reduce (uniform across waves; untouched
            // nodes keep their snapshot capacity by definition)
            // touched[] is read here, with the capacity loads: wave 0
            // stores to both below
            const bool was_touched = touched[best.i] != 0;
            long long ccand = BIG_CAP;
            if (lane < R) {
                float rq = req[lane];
                if (rq > EPS) {
                    size_t off = (size_t)lane * N + best.i;
                    float avail = alloc[off] - used[off]
                        + (ext ? ext[off] : 0.f);
                    float cc = (avail + EPS) / rq;
                    if (cc > (float)BIG_CAP) cc = (float)BIG_CAP;
                    long long cl = (long long)floorf(cc);
                    ccand = max(cl, 0ll);
                }
            }
            for (int off = WAVE / 2; off > 0; off >>= 1)
                ccand = min(ccand, (long long)__shfl_down((long long)ccand,
                                                          off));
            const long long cap = __shfl((long long)ccand, 0);
            int take = (int)min(cap, (long long)remaining);
            // every wave has read used[]/touched[] of the winner before
            // any of them is stored to — otherwise a late wave computes
            // a different take / tcount and the mirrors diverge
            __syncthreads();
            if (take > 0) {
                if (tid == 0) {
                    ln[cursor] = best.i;
                    lc[cursor] = take;
                }
                cursor += 1;
                remaining -= take;
                // `used` waits for the end of the class: the winner is
                // never a node this class already took (consumed nodes
                // are skipped above), so nothing in this loop would read
                // the new value, and a discarded gang then leaves no trace
            }
            if (!was_touched) {
                // mark even on take==0 (defensive: a zero-cap winner must
                // never win again; cannot occur when snapshot caps hold)
                if (tid == 0) {
                    touched[best.i] = 1;
                    touched_list[tcount] = best.i;
                }
                tcount += 1;
            }
            __syncthreads();    // barrier 2: order stores vs next loads
        }

        // barrier 2 of the last pop ordered thread 0's log stores
        int total = (int)budget - remaining;
        if (total < fuse) {
            // single-class gang discard (statement.go:375): nothing was
            // applied; the log keeps its nodes with zeroed counts
            for (int e = tid; e < cursor; e += CH_THREADS) lc[e] = 0;
            if (tid == 0) { log_len[c] = cursor; class_placed[c] = 0; }
        } else {
            // commit from the log, a wave per entry (dev_commit_log)
            for (int e = wid; e < cursor; e += CH_WAVES) {
                if (lane < R) {
                    float* u = used + (size_t)lane * N + ln[e];
                    *u = acc_add(*u, lc[e], req[lane]);
                }
            }
            if (tid < R) qa[tid] = acc_add(qa[tid], total, req[tid]);
            if (tid == 0) {
                log_len[c] = cursor;
                class_placed[c] = total;
                job_placed[cd.job_idx] += total;
            }
        }
        __syncthreads();
    }
}

}  // namespace vamd

// ---------------------------------------------------------------------------
// C ABI launchers (bound in bindings.cpp; stream passed from torch)
// ---------------------------------------------------------------------------
extern "C" {

void vamd_score_cap(
    const float* alloc, const float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score_out, int* cap_out,
    int N, int R, int W, hipStream_t stream)
{
    int threads = 256;
    int blocks = min((N + threads - 1) / threads, 4096);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(vamd::score_cap_kernel, dim3(blocks), dim3(threads), 0,
                       stream, alloc, used, extra, ready, taints, planes, req,
                       tolerated, require, forbid, w_least, w_most, w_bal,
                       dim_w, bias, score_out, cap_out, N, R, W);
}

void vamd_select_commit(
    float* score, const int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed, int fuse_min,
    unsigned* sort_scratch, int N, int R, int K, hipStream_t stream)
{
    // mega-classes (gang bundles): sort-based bulk fill — identical
    // decisions, ~16N total accesses instead of ~N per consumed node.
    // Small classes: the iterative argmax loop wins (few consumptions).
    if (sort_scratch != nullptr && ntasks >= 512 && N >= 512) {
        hipLaunchKernelGGL(vamd::bulk_select_kernel, dim3(1),
                           dim3(BS_THREADS), 0, stream, score, cap, req,
                           ntasks, used, queue_alloc, queue_limit, log_nodes,
                           log_counts, log_len, placed, job_placed, fuse_min,
                           sort_scratch, N, R, K);
        return;
    }
    hipLaunchKernelGGL(vamd::select_commit_kernel, dim3(1), dim3(SC_THREADS),
                       0, stream, score, cap, req, ntasks, used, queue_alloc,
                       queue_limit, log_nodes, log_counts, log_len, placed,
                       job_placed, fuse_min, N, R, K);
}

void vamd_fused_score_select(
    const float* alloc, float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score, int* cap,
    int ntasks, float* queue_alloc, const float* queue_limit,
    int* log_nodes, int* log_counts, int* log_len, int* placed,
    int* job_placed, int fuse_min, int N, int R, int W, int K,
    hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::fused_score_select_kernel, dim3(1),
                       dim3(SC_THREADS), 0, stream, alloc, used, extra,
                       ready, taints, planes, req, tolerated, require,
                       forbid, w_least, w_most, w_bal, dim_w, bias, score,
                       cap, ntasks, queue_alloc, queue_limit, log_nodes,
                       log_counts, log_len, placed, job_placed, fuse_min,
                       N, R, W, K);
}

void vamd_finalize_job(
    const int* job_placed, int occupied, int min_available,
    const int* class_placed, const int* class_min, uint8_t* flag, int nc,
    hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::finalize_job_kernel, dim3(1), dim3(64), 0,
                       stream, job_placed, occupied, min_available,
                       class_placed, class_min, flag, nc);
}

void vamd_cond_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, int N, int R, hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::cond_revert_kernel, dim3(1), dim3(1024), 0,
                       stream, flag, log_nodes, log_counts, log_len, req,
                       used, queue_alloc, placed, job_placed, N, R);
}

void vamd_spread_select(
    float* score, int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    const int* dom_of, int* dom_count, int D, int max_skew, int fuse_min,
    void* scratch, int N, int R, int K, hipStream_t stream)
{
    // scratch: D 64-bit head keys, then N log-slot ints
    unsigned long long* head = (unsigned long long*)scratch;
    int* slot = (int*)(head + (D > 0 ? D : 0));
    hipLaunchKernelGGL(vamd::spread_select_kernel, dim3(1), dim3(SP_THREADS),
                       0, stream, score, cap, req, ntasks, used, queue_alloc,
                       queue_limit, log_nodes, log_counts, log_len, placed,
                       job_placed, dom_of, dom_count, D, max_skew, fuse_min,
                       head, slot, N, R, K);
}

void vamd_spread_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, const int* dom_of, int* dom_count, int D, int N, int R,
    hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::spread_revert_kernel, dim3(1), dim3(1024), 0,
                       stream, flag, log_nodes, log_counts, log_len, req,
                       used, queue_alloc, placed, job_placed, dom_of,
                       dom_count, D, N, R);
}

void vamd_domain_mask(
    float* score, int* cap, const int* dom_of, const int* dom_count, int D,
    int mode, void* scratch, int N, hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::domain_mask_kernel, dim3(1), dim3(SP_THREADS),
                       0, stream, score, cap, dom_of, dom_count, D, mode,
                       (unsigned long long*)scratch, N);
}

void vamd_domain_count_add(
    const int* log_nodes, const int* log_counts, const int* log_len,
    const int* dom_of, int* dom_count, int D, int N, int K,
    hipStream_t stream)
{
    int threads = 256;
    int blocks = min((K + threads - 1) / threads, 64);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(vamd::domain_count_add_kernel, dim3(blocks),
                       dim3(threads), 0, stream, log_nodes, log_counts,
                       log_len, dom_of, dom_count, D, N, K);
}

void vamd_batch_score(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                      int count, float* score_buf, hipStream_t stream)
{
    int threads = 256;
    int nx = (cy.N + threads - 1) / threads;
    if (nx > 1024) nx = 1024;
    if (nx < 1) nx = 1;
    hipLaunchKernelGGL(vamd::batch_score_kernel, dim3(nx, count),
                       dim3(threads), 0, stream, dd.classes, c0, cy.alloc,
                       cy.used, cy.extra, cy.ready, cy.taints, cy.planes,
                       cy.bias, cy.bias_rows, cy.class_req, dd.class_tol,
                       cy.class_require, cy.class_forbid, cy.dim_w,
                       score_buf, cy.N, cy.R, cy.W);
}

void vamd_topk(float* score_buf, int count, float* topk_vals, int* topk_ids,
               int N, hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::topk_kernel, dim3(count), dim3(SC_THREADS), 0,
                       stream, score_buf, topk_vals, topk_ids, N);
}

void vamd_select_chain(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                       int c1, float* score_buf, const float* topk_vals,
                       const int* topk_ids, uint8_t* touched,
                       int* touched_list, hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::select_chain_kernel, dim3(1), dim3(CH_THREADS),
                       0, stream, dd.classes, dd.jobs, c0, c1, cy.alloc,
                       cy.used, cy.extra, cy.ready, cy.taints, cy.planes,
                       cy.bias, cy.bias_rows, cy.class_req, dd.class_tol,
                       cy.class_require, cy.class_forbid, cy.dim_w,
                       cy.queue_alloc, cy.queue_limit, score_buf, topk_vals,
                       topk_ids, cy.log_nodes, cy.log_counts, cy.log_len,
                       cy.class_placed, cy.job_placed, touched, touched_list,
                       cy.N, cy.R, cy.W);
}

void vamd_megacycle(const VamdCycle& cy, const VamdDevDescs& dd,
                    hipStream_t stream)
{
    hipLaunchKernelGGL(vamd::megacycle_kernel, dim3(1), dim3(SC_THREADS), 0,
                       stream, dd.classes, dd.jobs, cy.n_jobs, cy.alloc,
                       cy.used, cy.extra, cy.ready, cy.taints, cy.planes,
                       cy.bias, cy.bias_rows, cy.class_req, dd.class_tol,
                       cy.class_require, cy.class_forbid, cy.class_min,
                       cy.dim_w, cy.queue_alloc, cy.queue_limit,
                       cy.score_scratch, cy.cap_scratch, cy.log_nodes,
                       cy.log_counts, cy.log_len, cy.class_placed,
                       cy.job_placed, cy.job_flag, cy.N, cy.R, cy.W);
}

}  // extern "C"
