// Stand-alone replay of the settle core's fixed cases and boundary sizes.
// Built by tests/test_settle_core_native.py with the host compiler and
// -fsanitize=address,undefined; exits 0 when every case matches and the
// sanitizers stay silent.  Output buffers are heap blocks of exactly the
// advertised capacity so a write past them is an ASan report.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "settle_core.h"

namespace {

using V = std::vector<int32_t>;
int failures = 0;

template <class T>
struct Block {                     // heap block of exactly n elements
    std::unique_ptr<T[]> p;
    size_t n = 0;
    void fill(size_t count, T v) {
        p.reset(new T[count]);
        n = count;
        for (size_t i = 0; i < n; ++i) p[i] = v;
    }
};

struct Run {
    Block<int32_t> p_entry, p_node, p_take, p_toff, rev_node, rev_cnt;
    Block<uint8_t> outcome, full;
    vamd::SettleOut so{};
    int status = 0;

    void size(size_t piece_cap, size_t rev_cap, size_t n_entries) {
        p_entry.fill(piece_cap, -7); p_node.fill(piece_cap, -7);
        p_take.fill(piece_cap, -7); p_toff.fill(piece_cap, -7);
        rev_node.fill(rev_cap, -7); rev_cnt.fill(rev_cap, -7);
        outcome.fill(n_entries, 9); full.fill(n_entries, 9);
        so.p_entry = p_entry.p.get(); so.p_node = p_node.p.get();
        so.p_take = p_take.p.get(); so.p_toff = p_toff.p.get();
        so.piece_cap = piece_cap;
        so.outcome = outcome.p.get(); so.full = full.p.get();
        so.rev_node = rev_node.p.get(); so.rev_cnt = rev_cnt.p.get();
        so.rev_cap = rev_cap;
    }
};

std::vector<uint8_t> mask(size_t n_nodes, std::initializer_list<int> lost) {
    std::vector<uint8_t> m(n_nodes, 0);
    for (int i : lost) m[static_cast<size_t>(i)] = 1;
    return m;
}

// caps < 0: the documented n + n_entries
Run bundle(const V& ln, const V& lc, const V& ntasks, const V& mins,
           const std::vector<uint8_t>& lost, long piece_cap = -1,
           long rev_cap = -1) {
    Run r;
    const size_t dflt = ln.size() + ntasks.size();
    r.size(piece_cap < 0 ? dflt : static_cast<size_t>(piece_cap),
           rev_cap < 0 ? dflt : static_cast<size_t>(rev_cap), ntasks.size());
    r.status = vamd::settle_bundle(
        ln.data(), lc.data(), static_cast<int64_t>(ln.size()), ntasks.data(),
        mins.data(), static_cast<int64_t>(ntasks.size()),
        lost.empty() ? nullptr : lost.data(),
        static_cast<int64_t>(lost.size()), &r.so);
    return r;
}

Run plain(const V& ln, const V& lc, const std::vector<uint8_t>& lost,
          long piece_cap = -1, long rev_cap = -1) {
    Run r;
    const size_t dflt = ln.size() + 1;
    r.size(piece_cap < 0 ? dflt : static_cast<size_t>(piece_cap),
           rev_cap < 0 ? dflt : static_cast<size_t>(rev_cap), 1);
    r.status = vamd::settle_plain(
        ln.data(), lc.data(), static_cast<int64_t>(ln.size()),
        lost.empty() ? nullptr : lost.data(),
        static_cast<int64_t>(lost.size()), &r.so);
    return r;
}

void expect(const char* name, bool ok) {
    if (!ok) {
        std::fprintf(stderr, "FAIL %s\n", name);
        ++failures;
    }
}

bool eq(const int32_t* got, size_t n, const V& want) {
    return n == want.size() &&
           (n == 0 || std::memcmp(got, want.data(), n * sizeof(int32_t)) == 0);
}

bool eq8(const Block<uint8_t>& got, std::initializer_list<int> want) {
    if (got.n != want.size()) return false;
    size_t i = 0;
    for (int w : want)
        if (got.p[i++] != w) return false;
    return true;
}

void check(const char* name, const Run& r, const V& entry, const V& node,
           const V& take, const V& toff, std::initializer_list<int> outcome,
           std::initializer_list<int> full, const V& rnode, const V& rcnt,
           size_t n_tail) {
    const bool ok =
        r.status == vamd::SETTLE_OK &&
        eq(r.so.p_entry, r.so.n_pieces, entry) &&
        eq(r.so.p_node, r.so.n_pieces, node) &&
        eq(r.so.p_take, r.so.n_pieces, take) &&
        eq(r.so.p_toff, r.so.n_pieces, toff) &&
        eq8(r.outcome, outcome) && eq8(r.full, full) &&
        eq(r.so.rev_node, r.so.n_rev, rnode) &&
        eq(r.so.rev_cnt, r.so.n_rev, rcnt) && r.so.n_tail == n_tail;
    expect(name, ok);
}

const int NONE = vamd::SETTLE_NONE, OK = vamd::SETTLE_COMMITTED,
          MISS = vamd::SETTLE_GANG_MISS, LOST = vamd::SETTLE_LOST;

}  // namespace

int main() {
    const std::vector<uint8_t> nolost;

    // gang miss, then a smaller entry places from the recycled slots
    check("gang_miss_recycle",
          bundle({2, 5}, {2, 1}, {4, 3}, {4, 3}, nolost),
          {1, 1}, {2, 5}, {2, 1}, {0, 2}, {MISS, OK}, {0, 1}, {}, {}, 0);

    // unclaimed tail that begins mid-entry (eoff > 0)
    check("tail_mid_entry", bundle({1, 4}, {5, 2}, {2}, {2}, nolost),
          {0}, {1}, {2}, {0}, {OK}, {1}, {1, 4}, {3, 2}, 2);

    // zero-count log entries inside a bundle yield zero-take pieces
    check("zero_count_bundle",
          bundle({0, 3, 6, 7, 1}, {1, 0, 2, 0, 2}, {3, 2}, {3, 1}, nolost),
          {0, 0, 0, 1, 1}, {0, 3, 6, 7, 1}, {1, 0, 2, 0, 2},
          {0, 1, 1, 0, 0}, {OK, OK}, {1, 1}, {}, {}, 0);

    // ... and are skipped inside a plain class
    check("zero_count_plain", plain({2, 5, 6, 0}, {0, 2, 0, 1}, nolost),
          {0, 0}, {5, 0}, {2, 1}, {0, 2}, {OK}, {0}, {}, {}, 0);

    // a lost node hitting a bundle entry reverts that entry only
    check("lost_bundle",
          bundle({1, 2, 3}, {2, 1, 2}, {3, 2}, {3, 2}, mask(8, {2})),
          {1}, {3}, {2}, {0}, {LOST, OK}, {0, 1}, {1, 2}, {2, 1}, 0);

    // a lost node hitting a plain class reverts it wholesale
    check("lost_plain", plain({1, 6}, {2, 2}, mask(8, {6})),
          {}, {}, {}, {}, {LOST}, {0}, {1, 6}, {2, 2}, 0);

    // partial gang: above the minimum, not fully placed
    check("partial_gang", bundle({3}, {2}, {4}, {2}, nolost),
          {0}, {3}, {2}, {0}, {OK}, {0}, {}, {}, 0);

    // a miss in the middle restores a mid-entry cursor
    check("miss_restores_mid_entry",
          bundle({0, 1}, {3, 1}, {2, 5, 2}, {2, 5, 2}, nolost),
          {0, 2, 2}, {0, 0, 1}, {2, 1, 1}, {0, 0, 1}, {OK, MISS, OK},
          {1, 0, 1}, {}, {}, 0);

    // -- boundary sizes ----------------------------------------------------
    check("n0_miss", bundle({}, {}, {2}, {1}, nolost),
          {}, {}, {}, {}, {MISS}, {0}, {}, {}, 0);
    check("n0_min0_commits_empty", bundle({}, {}, {2}, {0}, nolost),
          {}, {}, {}, {}, {OK}, {0}, {}, {}, 0);
    check("n0_no_entries", bundle({}, {}, {}, {}, nolost),
          {}, {}, {}, {}, {}, {}, {}, {}, 0);
    check("n0_plain", plain({}, {}, nolost),
          {}, {}, {}, {}, {NONE}, {0}, {}, {}, 0);
    check("one_entry", bundle({4}, {3}, {3}, {3}, nolost),
          {0}, {4}, {3}, {0}, {OK}, {1}, {}, {}, 0);

    // most pieces a walk can emit: every entry but the last leaves its
    // log entry open (n + n_entries - 1 = 4 for n = 2, three entries)
    check("max_pieces", bundle({0, 1}, {3, 1}, {1, 1, 2}, {1, 1, 2}, nolost),
          {0, 1, 2, 2}, {0, 0, 0, 1}, {1, 1, 1, 1}, {0, 0, 0, 1},
          {OK, OK, OK}, {1, 1, 1}, {}, {}, 0);
    check("max_pieces_tight_cap",
          bundle({0, 1}, {3, 1}, {1, 1, 2}, {1, 1, 2}, nolost, 4, 0),
          {0, 1, 2, 2}, {0, 0, 0, 1}, {1, 1, 1, 1}, {0, 0, 0, 1},
          {OK, OK, OK}, {1, 1, 1}, {}, {}, 0);
    expect("pieces_over_cap_refused",
           bundle({0, 1}, {3, 1}, {1, 1, 2}, {1, 1, 2}, nolost, 3, 0).status
               == vamd::SETTLE_ERR_CAPACITY);

    // reverted pairs exactly at n + n_entries: a lost entry's open piece
    // plus the partial tail of the same log entry (1 + 1 = 2)
    check("rev_at_bound", bundle({5}, {3}, {1}, {1}, mask(8, {5})),
          {}, {}, {}, {}, {LOST}, {0}, {5, 5}, {1, 2}, 1);
    expect("rev_over_cap_refused",
           bundle({5}, {3}, {1}, {1}, mask(8, {5}), -1, 1).status
               == vamd::SETTLE_ERR_CAPACITY);
    expect("tail_over_cap_refused",
           bundle({1, 4}, {5, 2}, {2}, {2}, nolost, -1, 1).status
               == vamd::SETTLE_ERR_CAPACITY);
    expect("plain_over_cap_refused",
           plain({1, 2}, {1, 1}, nolost, 1, 0).status
               == vamd::SETTLE_ERR_CAPACITY);
    expect("plain_rev_over_cap_refused",
           plain({1, 6}, {2, 2}, mask(8, {6}), -1, 1).status
               == vamd::SETTLE_ERR_CAPACITY);

    // malformed logs are refused, not walked
    expect("negative_count_refused",
           bundle({1, 2}, {-1, 2}, {2}, {2}, nolost).status
               == vamd::SETTLE_ERR_NEGATIVE);
    expect("node_outside_mask_refused",
           bundle({9}, {1}, {1}, {1}, mask(8, {2})).status
               == vamd::SETTLE_ERR_NODE_RANGE);
    expect("plain_node_outside_mask_refused",
           plain({-1}, {1}, mask(8, {2})).status
               == vamd::SETTLE_ERR_NODE_RANGE);

    if (failures) {
        std::fprintf(stderr, "%d case(s) failed\n", failures);
        return 1;
    }
    std::puts("settle core OK");
    return 0;
}
