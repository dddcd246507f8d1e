// Dispatch trace of the whole-cycle runner (volcano_amd/ops/csrc/
// cycle_runner.hip, compiled as plain host C++).  Every launcher and HIP call
// the runner can reach is a recording stub here: one line per call with the
// scalars by name and every pointer as <array>+<element offset>.  To keep the
// lines short the array name is left out where it is the one the argument
// must point into (req=+3 is class_req + 3; a pointer into any other array
// prints in full), and a plan-wide pointer that is its array's base is left
// out altogether, as are N, R and W where they are the plan's.  main() runs a fixed list of hand-built plans, setting the
// VAMD_* environment itself; a plan whose calls repeat an earlier plan's
// (after any leading calls of its own) prints a reference to it, and a plan
// of more than FULL_MAX calls prints the sequence of launchers and a 64-bit
// FNV-1a hash of its lines (run with --full to see them all).  The output is compared byte for byte with
// tests/native/cycle_trace.expected (tests/test_cycle_runner_native.py).
// No GPU, no Python.

#include "vamd_api.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

// ---- named arrays: a pointer prints as the array it lies in + offset -------
struct Region { std::string name; const char* base; size_t bytes, elem; };
std::vector<Region> g_regions;
std::vector<std::unique_ptr<char[]>> g_store;
const hipStream_t STREAM = (hipStream_t)(uintptr_t)0x5eed;
int g_malloc_mode = 0;   // 0 = succeed, 1 = error, 2 = "success", null pointer

template <class T> T* arr(const char* name, size_t n) {
    size_t bytes = (n ? n : 1) * sizeof(T);
    g_store.emplace_back(new char[bytes]());
    g_regions.push_back({name, g_store.back().get(), bytes, sizeof(T)});
    return (T*)g_store.back().get();
}

std::string P(const void* p) {
    if (p == nullptr) return "null";
    const char* q = (const char*)p;
    for (const Region& r : g_regions)
        if (q >= r.base && q < r.base + r.bytes) {
            size_t off = (size_t)(q - r.base);
            if (off % r.elem == 0)
                return r.name + "+" + std::to_string(off / r.elem);
            return r.name + "+" + std::to_string(off) + "b";
        }
    return "WILD";
}

// the array each pointer argument must point into; '*' marks the plan-wide
// ones, which are expected at its base
const char* const CANON[][2] = {
    {"alloc", "*alloc"}, {"used", "*used"}, {"extra", "*extra"},
    {"ready", "*ready"}, {"taints", "*taints"}, {"planes", "*planes"},
    {"dim_w", "*dim_w"}, {"score", "*score"}, {"cap", "*cap"},
    {"bias", "*bias"}, {"bias_rows", "*bias_rows"},
    {"class_req", "*class_req"}, {"class_require", "*class_require"},
    {"class_forbid", "*class_forbid"}, {"sort_scratch", "*sort_scratch"},
    {"scratch", "*domain_scratch"}, {"classes_dev", "*blob"},
    {"req", "class_req"}, {"require", "class_require"},
    {"forbid", "class_forbid"}, {"queue_alloc", "queue_alloc"},
    {"queue_limit", "queue_limit"}, {"log_nodes", "log_nodes"},
    {"log_counts", "log_counts"}, {"log_len", "log_len"},
    {"placed", "class_placed"}, {"class_placed", "class_placed"},
    {"job_placed", "job_placed"}, {"flag", "job_flag"},
    {"job_flag", "job_flag"}, {"class_min", "class_min"},
    {"dom_of", "dom_of"}, {"dom_count", "count"}, {"jobs_dev", "blob"},
    {"class_tol_dev", "blob"}, {"score_buf", "blob"}, {"topk_vals", "blob"},
    {"topk_ids", "blob"}, {"touched", "blob"}, {"touched_list", "blob"},
    {"ptr", "blob"}, {"dst", "blob"}};

std::vector<std::string> g_trace;   // calls of the plan being run
int g_N, g_R, g_W;                  // its sizes
bool g_full = false;                // --full: never abridge
const size_t FULL_MAX = 24;

struct Line {
    std::string s;
    Line(const char* name, hipStream_t st) : s(name) {
        if (st != STREAM) s += " BAD-STREAM";
    }
    Line& p(const char* k, const void* v) {
        std::string t = P(v);
        for (auto& c : CANON) {
            if (strcmp(c[0], k) != 0) continue;
            const bool wide = c[1][0] == '*';
            const std::string base = c[1] + (wide ? 1 : 0);
            if (wide && t == base + "+0") return *this;
            if (t.compare(0, base.size() + 1, base + "+") == 0)
                t = t.substr(base.size());
        }
        s += std::string(" ") + k + "=" + t; return *this;
    }
    Line& i(const char* k, long long v) {
        s += std::string(" ") + k + "=" + std::to_string(v); return *this;
    }
    Line& f(const char* k, float v) {
        char b[32]; snprintf(b, sizeof b, "%g", (double)v);
        s += (*k ? std::string(" ") + k + "=" : std::string("/")) + b;
        return *this;
    }
    Line& node(const float* alloc, const float* used, const float* extra,
               const uint8_t* ready, const int64_t* taints,
               const int64_t* planes) {
        return p("alloc", alloc).p("used", used).p("extra", extra)
            .p("ready", ready).p("taints", taints).p("planes", planes);
    }
    Line& log(const int* nodes, const int* counts, const int* len,
              const int* placed, const int* job_placed) {
        return p("log_nodes", nodes).p("log_counts", counts).p("log_len", len)
            .p("placed", placed).p("job_placed", job_placed);
    }
    Line& dims(int N, int R, int W) {
        if (N != g_N) i("N", N);
        if (R != g_R) i("R", R);
        return (W >= 0 && W != g_W) ? i("W", W) : *this;
    }
    ~Line() { g_trace.push_back(s); }
};

// prints the calls of the plan just run; where they end with (or are) the
// whole of an earlier plan's calls, that part prints as a reference
void flush_plan(const std::string& header) {
    static std::vector<std::pair<std::string, std::vector<std::string>>> seen;
    puts(header.c_str());
    size_t own = g_trace.size();
    for (auto& e : seen) {
        const size_t n = e.second.size();
        if (n < 8 || n > g_trace.size() || g_trace.size() - n >= own) continue;
        if (!std::equal(e.second.begin(), e.second.end(),
                        g_trace.end() - (long)n)) continue;
        own = g_trace.size() - n;
        for (size_t k = 0; k < own; ++k) puts(g_trace[k].c_str());
        printf("  then %zu calls, the same as in: %s\n", n,
               e.first.c_str() + 3);
        break;
    }
    if (own == g_trace.size()) {
        seen.emplace_back(header, g_trace);
        if (g_full || own <= FULL_MAX) {
            for (auto& l : g_trace) puts(l.c_str());
        } else {
            unsigned long long h = 1469598103934665603ull;
            std::string seq, prev;
            size_t run = 0;
            auto close_run = [&] {
                if (run) seq += " " + prev + " x" + std::to_string(run);
            };
            for (auto& l : g_trace) {
                for (unsigned char ch : l + "\n") h = (h ^ ch) * 1099511628211ull;
                std::string name = l.substr(0, l.find(' '));
                if (name != prev) { close_run(); prev = name; run = 0; }
                ++run;
            }
            close_run();
            printf("  %zu calls:%s\n  fnv1a=%016llx\n", own, seq.c_str(), h);
        }
    }
    g_trace.clear();
}

}  // namespace

// ---- recording stubs ---------------------------------------------------------
extern "C" {

hipError_t hipMallocAsync(void** dev_ptr, size_t size, hipStream_t stream) {
    Line l("hipMallocAsync", stream);
    l.i("size", (long long)size);
    if (g_malloc_mode == 1) { l.s += " -> error"; return hipErrorOutOfMemory; }
    if (g_malloc_mode == 2) { l.s += " -> null"; *dev_ptr = nullptr; return hipSuccess; }
    *dev_ptr = arr<char>("blob", size);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t size,
                          hipMemcpyKind kind, hipStream_t stream) {
    Line("hipMemcpyAsync", stream).p("dst", dst).p("src", src)
        .i("size", (long long)size).i("kind", (int)kind);
    memcpy(dst, src, size);
    return hipSuccess;
}

hipError_t hipFreeAsync(void* dev_ptr, hipStream_t stream) {
    Line("hipFreeAsync", stream).p("ptr", dev_ptr);
    return hipSuccess;
}

void vamd_score_cap(
    const float* alloc, const float* used, const float* extra,
    const uint8_t* ready, const int64_t* taints, const int64_t* planes,
    const float* req, int64_t tolerated, const int64_t* require,
    const int64_t* forbid, float w_least, float w_most, float w_bal,
    const float* dim_w, const float* bias, float* score_out, int* cap_out,
    int N, int R, int W, hipStream_t stream)
{
    Line("score_cap", stream).node(alloc, used, extra, ready, taints, planes)
        .p("req", req).i("tol", tolerated).p("require", require)
        .p("forbid", forbid).f("w", w_least).f("", w_most).f("", w_bal).p("dim_w", dim_w).p("bias", bias)
        .p("score", score_out).p("cap", cap_out).dims(N, R, W);
}

void vamd_select_commit(
    float* score, const int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed, int fuse_min,
    unsigned* sort_scratch, int N, int R, int K, hipStream_t stream)
{
    Line("select_commit", stream).p("score", score).p("cap", cap)
        .p("req", req).i("ntasks", ntasks).p("used", used)
        .p("queue_alloc", queue_alloc).p("queue_limit", queue_limit)
        .log(log_nodes, log_counts, log_len, placed, job_placed)
        .i("fuse_min", fuse_min).p("sort_scratch", sort_scratch)
        .dims(N, R, -1).i("K", K);
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
    Line("fused_score_select", stream)
        .node(alloc, used, extra, ready, taints, planes)
        .p("req", req).i("tol", tolerated).p("require", require)
        .p("forbid", forbid).f("w", w_least).f("", w_most).f("", w_bal).p("dim_w", dim_w).p("bias", bias)
        .p("score", score).p("cap", cap).i("ntasks", ntasks)
        .p("queue_alloc", queue_alloc).p("queue_limit", queue_limit)
        .log(log_nodes, log_counts, log_len, placed, job_placed)
        .i("fuse_min", fuse_min).dims(N, R, W).i("K", K);
}

void vamd_finalize_job(
    const int* job_placed, int occupied, int min_available,
    const int* class_placed, const int* class_min, uint8_t* flag, int nc,
    hipStream_t stream)
{
    Line("finalize_job", stream).p("job_placed", job_placed)
        .i("occupied", occupied).i("min_available", min_available)
        .p("class_placed", class_placed).p("class_min", class_min)
        .p("flag", flag).i("nc", nc);
}

void vamd_cond_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, int N, int R, hipStream_t stream)
{
    Line("cond_revert", stream).p("flag", flag)
        .log(log_nodes, log_counts, log_len, placed, job_placed)
        .p("req", req).p("used", used).p("queue_alloc", queue_alloc)
        .dims(N, R, -1);
}

void vamd_spread_select(
    float* score, int* cap, const float* req, int ntasks, float* used,
    float* queue_alloc, const float* queue_limit, int* log_nodes,
    int* log_counts, int* log_len, int* placed, int* job_placed,
    const int* dom_of, int* dom_count, int D, int max_skew, int fuse_min,
    void* scratch, int N, int R, int K, hipStream_t stream)
{
    Line("spread_select", stream).p("score", score).p("cap", cap)
        .p("req", req).i("ntasks", ntasks).p("used", used)
        .p("queue_alloc", queue_alloc).p("queue_limit", queue_limit)
        .log(log_nodes, log_counts, log_len, placed, job_placed)
        .p("dom_of", dom_of).p("dom_count", dom_count).i("D", D)
        .i("skew", max_skew).i("fuse_min", fuse_min).p("scratch", scratch)
        .dims(N, R, -1).i("K", K);
}

void vamd_spread_revert(
    const uint8_t* flag, int* log_nodes, int* log_counts, const int* log_len,
    const float* req, float* used, float* queue_alloc, int* placed,
    int* job_placed, const int* dom_of, int* dom_count, int D, int N, int R,
    hipStream_t stream)
{
    Line("spread_revert", stream).p("flag", flag)
        .log(log_nodes, log_counts, log_len, placed, job_placed)
        .p("req", req).p("used", used).p("queue_alloc", queue_alloc)
        .p("dom_of", dom_of).p("dom_count", dom_count).i("D", D)
        .dims(N, R, -1);
}

void vamd_domain_mask(
    float* score, int* cap, const int* dom_of, const int* dom_count, int D,
    int mode, void* scratch, int N, hipStream_t stream)
{
    Line("domain_mask", stream).p("score", score).p("cap", cap)
        .p("dom_of", dom_of).p("dom_count", dom_count).i("D", D)
        .i("mode", mode).p("scratch", scratch).i("N", N);
}

void vamd_domain_count_add(
    const int* log_nodes, const int* log_counts, const int* log_len,
    const int* dom_of, int* dom_count, int D, int N, int K,
    hipStream_t stream)
{
    Line("domain_count_add", stream).p("log_nodes", log_nodes)
        .p("log_counts", log_counts).p("log_len", log_len)
        .p("dom_of", dom_of).p("dom_count", dom_count).i("D", D).i("N", N)
        .i("K", K);
}

void vamd_batch_score(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                      int count, float* score_buf, hipStream_t stream)
{
    Line("batch_score", stream).p("classes_dev", dd.classes).i("c0", c0)
        .i("count", count)
        .node(cy.alloc, cy.used, cy.extra, cy.ready, cy.taints, cy.planes)
        .p("bias", cy.bias).p("bias_rows", cy.bias_rows)
        .p("class_req", cy.class_req).p("class_tol_dev", dd.class_tol)
        .p("class_require", cy.class_require)
        .p("class_forbid", cy.class_forbid).p("dim_w", cy.dim_w)
        .p("score_buf", score_buf).dims(cy.N, cy.R, cy.W);
}

void vamd_topk(float* score_buf, int count, float* topk_vals, int* topk_ids,
               int N, hipStream_t stream)
{
    Line("topk", stream).p("score_buf", score_buf).i("count", count)
        .p("topk_vals", topk_vals).p("topk_ids", topk_ids).i("N", N);
}

void vamd_select_chain(const VamdCycle& cy, const VamdDevDescs& dd, int c0,
                       int c1, float* score_buf, const float* topk_vals,
                       const int* topk_ids, uint8_t* touched,
                       int* touched_list, hipStream_t stream)
{
    Line("select_chain", stream).p("classes_dev", dd.classes)
        .p("jobs_dev", dd.jobs).i("c0", c0).i("c1", c1)
        .node(cy.alloc, cy.used, cy.extra, cy.ready, cy.taints, cy.planes)
        .p("bias", cy.bias).p("bias_rows", cy.bias_rows)
        .p("class_req", cy.class_req).p("class_tol_dev", dd.class_tol)
        .p("class_require", cy.class_require)
        .p("class_forbid", cy.class_forbid).p("dim_w", cy.dim_w)
        .p("queue_alloc", cy.queue_alloc).p("queue_limit", cy.queue_limit)
        .p("score_buf", score_buf).p("topk_vals", topk_vals)
        .p("topk_ids", topk_ids)
        .log(cy.log_nodes, cy.log_counts, cy.log_len, cy.class_placed,
             cy.job_placed)
        .p("touched", touched).p("touched_list", touched_list)
        .dims(cy.N, cy.R, cy.W);
}

void vamd_megacycle(const VamdCycle& cy, const VamdDevDescs& dd,
                    hipStream_t stream)
{
    Line("megacycle", stream).p("classes_dev", dd.classes)
        .p("jobs_dev", dd.jobs).i("n_jobs", cy.n_jobs)
        .node(cy.alloc, cy.used, cy.extra, cy.ready, cy.taints, cy.planes)
        .p("bias", cy.bias).p("bias_rows", cy.bias_rows)
        .p("class_req", cy.class_req).p("class_tol_dev", dd.class_tol)
        .p("class_require", cy.class_require)
        .p("class_forbid", cy.class_forbid).p("class_min", cy.class_min)
        .p("dim_w", cy.dim_w).p("queue_alloc", cy.queue_alloc)
        .p("queue_limit", cy.queue_limit).p("score", cy.score_scratch)
        .p("cap", cy.cap_scratch)
        .log(cy.log_nodes, cy.log_counts, cy.log_len, cy.class_placed,
             cy.job_placed)
        .p("job_flag", cy.job_flag).dims(cy.N, cy.R, cy.W);
}

}  // extern "C"

namespace {

// ---- hand-built plans --------------------------------------------------------
struct ClassSpec {
    int ntasks;
    int min_needed = 0;
    int group = -1;      // domain-rule group, -1 = none
    int mode = 0;        // 0 spread / 1 affinity / 2 anti
    int skew = 1;
};

struct Plan {
    int N = 100, R = 3, W = 2, Q = 3, B = 2;
    std::vector<std::vector<ClassSpec>> jobs;   // classes of each job
    bool sort_scratch = true;
    bool plan_bias = true, bias_rows = true;
    // domain block: G groups of D domains each (0 = the plan has none)
    int G = 0, D = 4;
    bool mode_column = true;
    int null_one = -1;   // 0 class_group, 1 dom_of, 2 count, 3 scratch
};

void add_singles(Plan& p, int n, int ntasks = 2) {
    for (int k = 0; k < n; ++k) p.jobs.push_back({ClassSpec{ntasks, 1}});
}

void env(const char* k, const char* v) {
    if (v) setenv(k, v, 1); else unsetenv(k);
}

void run(const char* name, const Plan& p, const char* mega = nullptr,
         const char* chunk = nullptr, const char* no_chain = nullptr,
         int malloc_mode = 0)
{
    char header[200];
    snprintf(header, sizeof header,
             "== %s N=%d mega=%s chunk=%s no_chain=%s malloc=%d", name, p.N,
             mega ? mega : "-", chunk ? chunk : "-", no_chain ? no_chain : "-",
             malloc_mode);
    env("VAMD_MEGACYCLE", mega);
    env("VAMD_CHAIN_CHUNK", chunk);
    env("VAMD_NO_CHAIN", no_chain);
    g_malloc_mode = malloc_mode;
    g_regions.clear();
    g_store.clear();

    const int N = g_N = p.N, R = g_R = p.R, W = g_W = p.W;
    const int J = (int)p.jobs.size();
    int C = 0;
    for (auto& j : p.jobs) C += (int)j.size();
    auto* classes = arr<VamdClassDesc>("classes", C);
    auto* jobs = arr<VamdJobDesc>("jobs", J);
    auto* class_tol = arr<int64_t>("class_tol", C);
    auto* group = arr<int32_t>("class_group", C);
    auto* skew = arr<int32_t>("class_skew", C);
    auto* mode = arr<int32_t>("class_mode", C);
    int c = 0, log_total = 0;
    for (int j = 0; j < J; ++j) {
        jobs[j].class_begin = c;
        // occupied / min_available vary so that fuse_min takes each branch:
        // gap above the role minimum, below it, and negative
        jobs[j].occupied = j % 3;
        jobs[j].min_available = (j % 4) * 2;
        for (const ClassSpec& s : p.jobs[j]) {
            VamdClassDesc& cd = classes[c];
            cd.job_idx = j;
            cd.queue_idx = c % p.Q;
            cd.ntasks = s.ntasks;
            cd.min_needed = s.min_needed;
            cd.log_off = log_total;
            cd.log_cap = s.ntasks < N ? s.ntasks : N;
            cd.flags = c % 2;
            cd.bias_row = (c % 3 == 2) ? c % p.B : -1;
            cd.w_least = 1.0f + (float)(c % 5);
            cd.w_most = 0.25f * (float)(c % 3);
            cd.w_bal = (c % 2) ? 0.5f : 0.0f;
            log_total += cd.log_cap;
            class_tol[c] = 0x100 + c;
            group[c] = s.group;
            skew[c] = s.skew;
            mode[c] = s.mode;
            ++c;
        }
        jobs[j].class_end = c;
    }

    const float* alloc = arr<float>("alloc", (size_t)R * N);
    float* used = arr<float>("used", (size_t)R * N);
    const float* extra = arr<float>("extra", (size_t)R * N);
    const uint8_t* ready = arr<uint8_t>("ready", N);
    const int64_t* taints = arr<int64_t>("taints", N);
    const int64_t* planes = arr<int64_t>("planes", (size_t)W * N);
    const float* bias = p.plan_bias ? arr<float>("bias", N) : nullptr;
    const float* bias_rows =
        p.bias_rows ? arr<float>("bias_rows", (size_t)p.B * N) : nullptr;
    const float* class_req = arr<float>("class_req", (size_t)C * R);
    const int64_t* class_require = arr<int64_t>("class_require", (size_t)C * W);
    const int64_t* class_forbid = arr<int64_t>("class_forbid", (size_t)C * W);
    const int32_t* class_min = arr<int32_t>("class_min", C);
    const float* dim_w = arr<float>("dim_w", R);
    float* queue_alloc = arr<float>("queue_alloc", (size_t)p.Q * R);
    const float* queue_limit = arr<float>("queue_limit", (size_t)p.Q * R);
    float* score = arr<float>("score", N);
    int* cap = arr<int>("cap", N);
    int* log_nodes = arr<int>("log_nodes", log_total);
    int* log_counts = arr<int>("log_counts", log_total);
    int* log_len = arr<int>("log_len", C);
    int* class_placed = arr<int>("class_placed", C);
    int* job_placed = arr<int>("job_placed", J);
    uint8_t* job_flag = arr<uint8_t>("job_flag", J);
    unsigned* sort_scratch =
        p.sort_scratch ? arr<unsigned>("sort_scratch", (size_t)4 * N) : nullptr;

    const int32_t* dom_of = nullptr;
    int32_t* count = nullptr;
    int32_t* count_off = nullptr;
    int32_t* domains = nullptr;
    void* dscratch = nullptr;
    if (p.G > 0) {
        dom_of = arr<int32_t>("dom_of", (size_t)p.G * N);
        count_off = arr<int32_t>("count_off", p.G);
        domains = arr<int32_t>("domains", p.G);
        int total = 0;
        for (int g = 0; g < p.G; ++g) {
            count_off[g] = total;
            domains[g] = p.D + g;       // groups differ in size
            total += domains[g];
        }
        count = arr<int32_t>("count", total);
        dscratch = arr<int32_t>("domain_scratch", (size_t)3 * N);
    }
    const int32_t* grp = p.G > 0 ? group : nullptr;
    const int32_t* skw = p.G > 0 ? skew : nullptr;
    const int32_t* mod = (p.G > 0 && p.mode_column) ? mode : nullptr;
    if (p.null_one == 0) grp = nullptr;
    if (p.null_one == 1) dom_of = nullptr;
    if (p.null_one == 2) count = nullptr;
    if (p.null_one == 3) dscratch = nullptr;

    // a caller without domain tables leaves the whole block null; one
    // without affinity classes leaves the mode column null
    VamdCycle cy = {
        sizeof(VamdCycle), N, R, W, C, J, 0, classes, jobs,
        alloc, used, extra, ready, taints, planes, bias, bias_rows,
        class_req, class_tol, class_require, class_forbid, class_min, dim_w,
        queue_alloc, queue_limit, score, cap, log_nodes, log_counts, log_len,
        class_placed, job_placed, job_flag, sort_scratch,
        grp, skw, mod, dom_of, count, count_off, domains, dscratch};
    if (vamd_run_cycle(&cy, STREAM) != 0) puts("vamd_run_cycle FAILED");
    flush_plan(header);
    cy.struct_size += 8;
    if (vamd_run_cycle(&cy, STREAM) == 0) puts("size guard MISSED");
    if (!g_trace.empty()) puts("size guard LATE");
}

ClassSpec spread(int ntasks, int g, int skew) {
    ClassSpec s{ntasks, 1}; s.group = g; s.skew = skew; return s;
}
ClassSpec affine(int ntasks, int g, int mode) {
    ClassSpec s{ntasks, 1}; s.group = g; s.mode = mode; return s;
}

}  // namespace

int main(int argc, char** argv) {
    g_full = argc > 1 && strcmp(argv[1], "--full") == 0;
    // fused vs split by N (4096 is the last fused size)
    for (int N : {100, 4096, 4097, 5000}) {
        Plan p; p.N = N;
        add_singles(p, 4, 3);
        run("small classes", p);
    }
    {   // no plan bias, no bias rows: every class scores without a bias
        Plan p; p.plan_bias = false; p.bias_rows = false;
        add_singles(p, 3);
        run("no bias", p);
        p.plan_bias = true;
        run("plan bias only", p);
    }
    // a 600-task class: never fused, bulk needs sort_scratch
    for (int N : {100, 5000})
        for (bool ss : {true, false}) {
            Plan p; p.N = N; p.sort_scratch = ss;
            p.jobs = {{ClassSpec{600, 600}}, {ClassSpec{511, 0}},
                      {ClassSpec{512, 0}}};
            run(ss ? "bulk class" : "bulk class, no sort_scratch", p);
        }
    // multi-class jobs: finalize + one revert per class
    for (int N : {100, 5000}) {
        Plan p; p.N = N;
        p.jobs = {{ClassSpec{2, 1}, ClassSpec{3, 2}},
                  {ClassSpec{4, 0}},
                  {ClassSpec{1, 1}, ClassSpec{600, 5}, ClassSpec{2, 0}}};
        run("multi-class jobs", p);
    }
    {   // empty plan
        Plan p;
        run("empty plan", p);
        run("empty plan", p, "1", "8");
    }

    // ---- chain path -----------------------------------------------------------
    {
        Plan p;
        add_singles(p, 40);
        run("40 singles", p);
        run("40 singles", p, nullptr, "8");
        run("40 singles", p, nullptr, "512");
        run("40 singles", p, nullptr, "0");
        run("40 singles", p, nullptr, "abc");
        run("40 singles", p, nullptr, "");
        run("40 singles", p, nullptr, "3");          // floor of 8
        run("40 singles", p, nullptr, "8", "1");
        run("40 singles", p, nullptr, "8", "0");
        run("40 singles", p, nullptr, "8", "x");
        run("40 singles", p, nullptr, nullptr, "0");
        run("40 singles", p, nullptr, "8", nullptr, 1);
        run("40 singles", p, nullptr, "8", nullptr, 2);
        p.N = 5000;
        run("40 singles", p, nullptr, "16");
        run("40 singles", p, nullptr, "100000");     // 256 MiB cap
        run("40 singles", p, nullptr, "16", nullptr, 1);
    }
    for (int n : {31, 32}) {
        Plan p; add_singles(p, n);
        run("chain run length", p, nullptr, "8");
    }
    {   // runs of 33 and 36 around a multi-class job: both chained
        Plan p;
        add_singles(p, 33);
        p.jobs.push_back({ClassSpec{2, 1}, ClassSpec{2, 1}});
        add_singles(p, 36);
        run("chain broken by a multi-class job", p, nullptr, "16");
    }
    {   // 32 chained, then a run too short to chain
        Plan p;
        add_singles(p, 32);
        p.jobs.push_back({ClassSpec{2, 1}, ClassSpec{2, 1}});
        add_singles(p, 10);
        run("chain then short run", p, nullptr, "512");
    }
    {   // two runs of 20: never 32 in a row
        Plan p;
        add_singles(p, 20);
        p.jobs.push_back({ClassSpec{2, 1}, ClassSpec{2, 1}});
        add_singles(p, 20);
        run("chain never long enough", p, nullptr, "8");
    }
    {   // a bulk class and a spread class each break a run
        Plan p; p.N = 5000; p.G = 1;
        add_singles(p, 34);
        p.jobs.push_back({spread(3, 0, 2)});
        add_singles(p, 32);
        p.jobs.push_back({ClassSpec{512, 1}});
        add_singles(p, 33);
        run("chain broken by spread and bulk", p, nullptr, "32");
        p.mode_column = false;
        run("chain broken by spread and bulk, no mode column", p, nullptr,
            "32");
    }

    // ---- megacycle ------------------------------------------------------------
    for (int n : {32, 31}) {
        Plan p; add_singles(p, n);
        run("megacycle size", p, "1");
        run("megacycle size", p, "0");
        run("megacycle size", p, "yes");
    }
    {
        Plan p;
        add_singles(p, 20);
        p.jobs.push_back({ClassSpec{2, 1}, ClassSpec{3, 1}});
        add_singles(p, 20);
        run("megacycle with a multi-class job", p, "1");
        run("megacycle, allocation fails", p, "1", nullptr, nullptr, 1);
        run("megacycle, allocation null", p, "1", nullptr, nullptr, 2);
        run("megacycle wins over chain", p, "1", "8");
        run("megacycle fails, chain fails", p, "1", "8", nullptr, 1);
        p.jobs[5][0].ntasks = 512;
        run("megacycle with a bulk class", p, "1");
        p.jobs[5][0].ntasks = 511;
        run("megacycle with a 511 class", p, "1");
    }
    {
        Plan p; p.G = 2;
        add_singles(p, 40);
        run("megacycle, domain block without domain class", p, "1");
        p.jobs[7][0] = spread(2, 1, 1);
        run("megacycle with a spread class", p, "1");
        p.jobs[7][0] = affine(2, 1, 1);
        run("megacycle with an affinity class", p, "1");
        p.null_one = 1;
        run("megacycle, domain block dead", p, "1");
    }

    // ---- domain rules ---------------------------------------------------------
    for (int N : {100, 5000}) {
        Plan p; p.N = N; p.G = 3;
        p.jobs = {{spread(5, 0, 1)},
                  {affine(4, 1, 1)},
                  {affine(3, 2, 2)},
                  {ClassSpec{2, 1}},
                  {spread(2, 2, 3), affine(2, 0, 1), ClassSpec{3, 0},
                   affine(600, 1, 2)},
                  {spread(700, 1, 2)},
                  {affine(600, 0, 1)}};
        run("domain rules", p);
        p.sort_scratch = false;
        run("domain rules, no sort_scratch", p);
        p.sort_scratch = true;
        p.mode_column = false;
        run("domain rules, class_mode null", p);
        p.mode_column = true;
        for (int k = 0; k < 4; ++k) {
            p.null_one = k;
            run("domain block with one pointer null", p);
        }
        p.mode_column = false;
        p.null_one = 3;
        run("domain block dead, class_mode null", p);
    }
    puts("cycle trace done");
    return 0;
}
