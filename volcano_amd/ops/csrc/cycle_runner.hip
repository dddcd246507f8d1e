// Whole-cycle launcher: replays an allocate cycle's kernel sequence from a
// host-built plan with one library call (the Python side would otherwise
// pay per-launch ctypes overhead per job; here the per-job cost is two
// hipLaunchKernelGGL enqueues).  Host code only — kernels live in
// scheduler_kernels.hip.
//
// Gang semantics (reference actions/allocate/allocate.go:719-866 +
// framework/statement.go): jobs run in the host-given priority order;
// classes of a job see each other's staged usage; a failed gang reverts
// before the next job's first kernel, so the sequential-cycle semantics
// are preserved exactly while the whole cycle stays on-device.

#include "vamd_api.h"

#include <cstdlib>
#include <cstring>

namespace {

const int CHAIN_MIN = 32;     // shortest run of jobs worth a chain
const int BULK_TASKS = 512;   // classes this large take the bulk select

// The opt-in paths, read once per cycle so tests can flip them.
//
// Megacycle (VAMD_MEGACYCLE=1): one launch for the whole plan when every
// class is small.  Measured OFF by default: at 10k nodes the async
// per-class enqueue pipeline overlaps launches with host plan iteration,
// while the single-workgroup megacycle serializes the per-class score
// passes (mix bench 559 ms vs 778 ms/step — profiles/raw/g28_mix*.log).
// Kept for launch-latency-bound deployments (small N, many classes); a
// cooperative multi-block variant is the roadmap item.
//
// Chain (VAMD_CHAIN_CHUNK=<n>; VAMD_NO_CHAIN=1 kills it): measured OFF by
// default as well: the batched score + topk phases are cheap, but the
// serial select chain degrades under placement CONCENTRATION — when every
// class prefers the same nodes, the top-K candidate lists exhaust and
// each pop pays a full-row fallback scan (mix bench: 199-291 ms vs 157 ms
// per-class at 10k nodes; 1.9 s vs 0.7 s at 50k — profiles/BENCH_NOTES.md).
// The async per-class pipeline keeps the GPU busy at ~12.5 us/class.  The
// variable being set at all opts in (the equivalence test exercises it;
// decisions are exact); a value that is not a positive number keeps the
// chunk of 512.
struct Env {
    bool megacycle, chain;
    int chunk;
};

Env read_env() {
    auto truthy = [](const char* e) { return e != nullptr && atoi(e) != 0; };
    const char* chunk = getenv("VAMD_CHAIN_CHUNK");
    Env env;
    env.megacycle = truthy(getenv("VAMD_MEGACYCLE"));
    env.chain = chunk != nullptr && !truthy(getenv("VAMD_NO_CHAIN"));
    env.chunk = (chunk != nullptr && atoi(chunk) > 0) ? atoi(chunk) : 512;
    return env;
}

// Stages descriptors + taint masks at the head of a fresh device blob of
// sizeof(descriptors) + extra_bytes (stream-ordered).  Returns the first
// byte after them, or nullptr when the allocation failed.
char* stage_descs(const VamdCycle& cy, size_t extra_bytes, hipStream_t stream,
                  void** blob, VamdDevDescs* dd)
{
    size_t sz_c = (size_t)cy.n_classes * sizeof(VamdClassDesc);
    size_t sz_j = (size_t)cy.n_jobs * sizeof(VamdJobDesc);
    size_t sz_t = (size_t)cy.n_classes * sizeof(int64_t);
    *blob = nullptr;
    if (hipMallocAsync(blob, sz_c + sz_j + sz_t + extra_bytes, stream)
            != hipSuccess || *blob == nullptr)
        return nullptr;
    char* p = (char*)*blob;
    (void)hipMemcpyAsync(p, cy.classes, sz_c, hipMemcpyHostToDevice, stream);
    (void)hipMemcpyAsync(p + sz_c, cy.jobs, sz_j, hipMemcpyHostToDevice,
                         stream);
    (void)hipMemcpyAsync(p + sz_c + sz_j, cy.class_tol, sz_t,
                         hipMemcpyHostToDevice, stream);
    dd->classes = (const VamdClassDesc*)p;
    dd->jobs = (const VamdJobDesc*)(p + sz_c);
    dd->class_tol = (const int64_t*)(p + sz_c + sz_j);
    return p + sz_c + sz_j + sz_t;
}

// One class of the plan with its rows resolved (stack only: the mix
// workload builds ~10k of these per cycle).
struct ClassView {
    const VamdClassDesc& cd;
    const float* req;            // [R]
    const int64_t* require;      // [W]
    const int64_t* forbid;       // [W]
    int64_t tol;
    VamdClassPlanes pl;          // ext / bias row
    float* queue_alloc;          // [R]
    const float* queue_limit;    // [R]
    int* log_nodes;              // [log_cap]
    int* log_counts;             // [log_cap]
    int* log_len;
    int* placed;
    int* job_placed;
    uint8_t* job_flag;
    int fuse_min;                // -1: the job's gang check is not fused
    // domain rule: group < 0 = none
    int group, mode, skew, D;
    const int32_t* dom_of;       // [N]
    int32_t* dom_count;          // [D]
};

struct Runner {
    const VamdCycle& cy;
    hipStream_t stream;
    const bool domains_live;

    Runner(const VamdCycle& c, hipStream_t s)
        : cy(c), stream(s),
          domains_live(c.class_group != nullptr && c.dom_of != nullptr &&
                       c.count != nullptr && c.domain_scratch != nullptr) {}

    int group_of(int c) const { return domains_live ? cy.class_group[c] : -1; }

    ClassView view(int j, int c) const {
        const VamdClassDesc& cd = cy.classes[c];
        const VamdJobDesc& job = cy.jobs[j];
        const int g = group_of(c);
        const bool single = job.class_end - job.class_begin == 1;
        ClassView v = {
            cd, cy.class_req + (size_t)c * cy.R,
            cy.class_require + (size_t)c * cy.W,
            cy.class_forbid + (size_t)c * cy.W, cy.class_tol[c],
            class_planes(cd, cy.extra, cy.bias, cy.bias_rows, cy.N),
            cy.queue_alloc + (size_t)cd.queue_idx * cy.R,
            cy.queue_limit + (size_t)cd.queue_idx * cy.R,
            cy.log_nodes + cd.log_off, cy.log_counts + cd.log_off,
            cy.log_len + c, cy.class_placed + c, cy.job_placed + j,
            cy.job_flag + j, single ? gang_fuse_min(job, cd) : -1,
            g, 0, 0, 0, nullptr, nullptr};
        if (g >= 0) {
            v.mode = cy.class_mode != nullptr ? cy.class_mode[c] : 0;
            if (v.mode == 0) v.skew = cy.class_skew[c];
            v.D = cy.domains[g];
            v.dom_of = cy.dom_of + (size_t)g * cy.N;
            v.dom_count = cy.count + cy.count_off[g];
        }
        return v;
    }

    void score(const ClassView& v) const {
        vamd_score_cap(cy.alloc, cy.used, v.pl.ext, cy.ready, cy.taints,
                       cy.planes, v.req, v.tol, v.require, v.forbid,
                       v.cd.w_least, v.cd.w_most, v.cd.w_bal, cy.dim_w,
                       v.pl.bias, cy.score_scratch, cy.cap_scratch,
                       cy.N, cy.R, cy.W, stream);
    }

    void select(const ClassView& v) const {
        vamd_select_commit(cy.score_scratch, cy.cap_scratch, v.req,
                           v.cd.ntasks, cy.used, v.queue_alloc, v.queue_limit,
                           v.log_nodes, v.log_counts, v.log_len, v.placed,
                           v.job_placed, v.fuse_min, cy.sort_scratch,
                           cy.N, cy.R, v.cd.log_cap, stream);
    }

    void fused(const ClassView& v) const {
        vamd_fused_score_select(
            cy.alloc, cy.used, v.pl.ext, cy.ready, cy.taints, cy.planes,
            v.req, v.tol, v.require, v.forbid, v.cd.w_least, v.cd.w_most,
            v.cd.w_bal, cy.dim_w, v.pl.bias, cy.score_scratch,
            cy.cap_scratch, v.cd.ntasks, v.queue_alloc, v.queue_limit,
            v.log_nodes, v.log_counts, v.log_len, v.placed, v.job_placed,
            v.fuse_min, cy.N, cy.R, cy.W, v.cd.log_cap, stream);
    }

    void spread_select(const ClassView& v) const {
        vamd_spread_select(cy.score_scratch, cy.cap_scratch, v.req,
                           v.cd.ntasks, cy.used, v.queue_alloc, v.queue_limit,
                           v.log_nodes, v.log_counts, v.log_len, v.placed,
                           v.job_placed, v.dom_of, v.dom_count, v.D, v.skew,
                           v.fuse_min, cy.domain_scratch, cy.N, cy.R,
                           v.cd.log_cap, stream);
    }

    void domain_mask(const ClassView& v) const {
        vamd_domain_mask(cy.score_scratch, cy.cap_scratch, v.dom_of,
                         v.dom_count, v.D, v.mode, cy.domain_scratch, cy.N,
                         stream);
    }

    void domain_count_add(const ClassView& v) const {
        vamd_domain_count_add(v.log_nodes, v.log_counts, v.log_len, v.dom_of,
                              v.dom_count, v.D, cy.N, v.cd.log_cap, stream);
    }

    void revert(const ClassView& v) const {
        if (v.group >= 0) {
            vamd_spread_revert(v.job_flag, v.log_nodes, v.log_counts,
                               v.log_len, v.req, cy.used, v.queue_alloc,
                               v.placed, v.job_placed, v.dom_of, v.dom_count,
                               v.D, cy.N, cy.R, stream);
            return;
        }
        vamd_cond_revert(v.job_flag, v.log_nodes, v.log_counts, v.log_len,
                         v.req, cy.used, v.queue_alloc, v.placed,
                         v.job_placed, cy.N, cy.R, stream);
    }

    void run_class(const ClassView& v) const {
        if (v.group >= 0 && v.mode != 0) {
            // inter-pod affinity / keyed anti-affinity: the rule collapses
            // into a mask over score/cap computed from the group's live
            // counts, then the ordinary select (bulk by size) and one
            // count update — four launches whatever ntasks is
            score(v);
            domain_mask(v);
            select(v);
            domain_count_add(v);
        } else if (v.group >= 0) {
            // topology spread: eligibility moves with every single
            // placement — always score + spread select, whatever the
            // class size
            score(v);
            spread_select(v);
        } else if (v.cd.ntasks < BULK_TASKS && cy.N <= 4096) {
            // small class on a small inventory: ONE fused launch (score
            // in-block + select).  At larger N the one-block score loses
            // the multi-CU latency hiding of the grid-stride kernel (mix
            // bench at N=10k measured 552 ms/step fused vs 334 ms split).
            fused(v);
        } else {
            score(v);
            select(v);
        }
    }

    // single-class jobs fuse the gang check into the commit (fuse_min)
    void run_job(int j) const {
        const VamdJobDesc& job = cy.jobs[j];
        for (int c = job.class_begin; c < job.class_end; ++c)
            run_class(view(j, c));
        const int nc = job.class_end - job.class_begin;
        if (nc == 1) return;
        vamd_finalize_job(cy.job_placed + j, job.occupied, job.min_available,
                          cy.class_placed + job.class_begin,
                          cy.class_min + job.class_begin, cy.job_flag + j, nc,
                          stream);
        for (int c = job.class_begin; c < job.class_end; ++c)
            revert(view(j, c));
    }

    // a single-class small job without a domain rule; anything else
    // breaks a chain run
    bool chainable(int j) const {
        const VamdJobDesc& jb = cy.jobs[j];
        return jb.class_end - jb.class_begin == 1 &&
            group_of(jb.class_begin) < 0 &&
            cy.classes[jb.class_begin].ntasks < BULK_TASKS;
    }

    // end of the maximal contiguous chain run that starts at job j (j
    // itself when that job is not chainable)
    int chain_run_end(int j) const {
        if (!chainable(j)) return j;
        int e = j + 1;
        while (e < cy.n_jobs && chainable(e) &&
               cy.jobs[e].class_begin == cy.jobs[e - 1].class_end)
            ++e;
        return e;
    }

    // The megacycle kernel has no bulk and no domain-rule select: such a
    // plan runs per class.  False as well when the staging allocation
    // fails: fall through to per-class launches.
    bool try_megacycle() const {
        if (cy.n_classes < 32) return false;
        for (int c = 0; c < cy.n_classes; ++c)
            if (cy.classes[c].ntasks >= BULK_TASKS || group_of(c) >= 0)
                return false;
        void* blob;
        VamdDevDescs dd;
        if (stage_descs(cy, 0, stream, &blob, &dd) == nullptr) return false;
        vamd_megacycle(cy, dd, stream);
        (void)hipFreeAsync(blob, stream);
        return true;
    }

    // ---- chain path: runs of >= CHAIN_MIN consecutive single-class small
    // jobs become 3 launches per chunk (batch score + topk + select chain)
    // instead of 2 per class.  Decisions match the per-class path exactly
    // (lazy re-score of touched nodes — scheduler_kernels.hip).
    void run(const Env& env) const {
        if (env.megacycle && try_megacycle()) return;

        bool chain_on = false;
        for (int j = 0; env.chain && !chain_on && j < cy.n_jobs; ) {
            const int e = chain_run_end(j);
            chain_on = e - j >= CHAIN_MIN;
            j = e > j ? e : j + 1;
        }

        const size_t N = (size_t)cy.N;
        int chunk = env.chunk;
        void* blob = nullptr;
        VamdDevDescs dd;
        float* score_buf = nullptr;
        int* tlist = nullptr;
        float* topk_vals = nullptr;
        int* topk_ids = nullptr;
        uint8_t* touched = nullptr;
        if (chain_on) {
            size_t per_class = N * sizeof(float);
            size_t mem_cap = (size_t)256 << 20;
            if ((size_t)chunk * per_class > mem_cap)
                chunk = (int)(mem_cap / per_class);
            if (chunk < 8) chunk = 8;
            size_t sz_s = (size_t)chunk * per_class;
            size_t sz_l = N * sizeof(int);
            size_t sz_tv = (size_t)chunk * 16 * sizeof(float);
            size_t sz_ti = (size_t)chunk * 16 * sizeof(int);
            char* q = stage_descs(cy, sz_s + sz_l + N + sz_tv + sz_ti, stream,
                                  &blob, &dd);
            if (q != nullptr) {
                score_buf = (float*)q; q += sz_s;
                tlist = (int*)q; q += sz_l;
                topk_vals = (float*)q; q += sz_tv;
                topk_ids = (int*)q; q += sz_ti;
                touched = (uint8_t*)q;
            } else {
                chain_on = false;
            }
        }

        for (int j = 0; j < cy.n_jobs; ) {
            const int e = chain_on ? chain_run_end(j) : j;
            if (e - j < CHAIN_MIN) {
                run_job(j++);
                continue;
            }
            const int ce = cy.jobs[e - 1].class_end;
            for (int cc = cy.jobs[j].class_begin; cc < ce; cc += chunk) {
                int cend = cc + chunk < ce ? cc + chunk : ce;
                vamd_batch_score(cy, dd, cc, cend - cc, score_buf, stream);
                vamd_topk(score_buf, cend - cc, topk_vals, topk_ids, cy.N,
                          stream);
                vamd_select_chain(cy, dd, cc, cend, score_buf, topk_vals,
                                  topk_ids, touched, tlist, stream);
            }
            j = e;
        }
        if (blob != nullptr)
            (void)hipFreeAsync(blob, stream);
    }
};

}  // namespace

extern "C" int vamd_run_cycle(const VamdCycle* cy, hipStream_t stream)
{
    if (cy == nullptr || cy->struct_size != sizeof(VamdCycle)) return 1;
    Runner(*cy, stream).run(read_env());
    return 0;
}
