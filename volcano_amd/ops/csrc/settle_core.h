// Host-side settle core: turns one class's placement log into per-entry
// pieces.  Plain C++17 over flat arrays -- no Python, no HIP -- so the
// CPython shell (vamd_host.cpp) and the stand-alone sanitizer harness
// (tests/native/settle_core_main.cpp) share one implementation.
//
// Mirrors the Python walk in scheduler/actions/allocate.py
// (AllocateAction._apply_py) statement for statement; that walk stays in
// the tree as the oracle.
#pragma once

#include <cstddef>
#include <cstdint>

namespace vamd {

enum SettleOutcome : uint8_t {
    SETTLE_NONE = 0,       // entry never reached / plain class without pieces
    SETTLE_COMMITTED = 1,
    SETTLE_GANG_MISS = 2,  // below the gang minimum; slots recycled
    SETTLE_LOST = 3,       // touched a lost node; slots reverted
};

enum SettleStatus : int {
    SETTLE_OK = 0,
    SETTLE_ERR_CAPACITY = -1,   // caller-sized output too small
    SETTLE_ERR_NEGATIVE = -2,   // negative log count (never produced by the
                                // decision plane; the walk is undefined)
    SETTLE_ERR_NODE_RANGE = -3, // node id outside the lost-node mask
};

// Caller-sized outputs.  piece_cap and rev_cap of n + n_entries always
// suffice (each entry emits one piece per log entry it finishes plus at
// most one that leaves its log entry open; the unclaimed tail is whatever
// the cursor never finished).  Both bounds are checked on every write.
struct SettleOut {
    int32_t* p_entry;      // [piece_cap] bundle entry index (0 for plain)
    int32_t* p_node;       // [piece_cap]
    int32_t* p_take;       // [piece_cap]
    int32_t* p_toff;       // [piece_cap] task offset within the entry
    size_t piece_cap;
    size_t n_pieces;       // committed pieces only
    uint8_t* outcome;      // [n_entries] SettleOutcome
    uint8_t* full;         // [n_entries] 1 = every task of the entry placed
    int32_t* rev_node;     // [rev_cap]
    int32_t* rev_cnt;      // [rev_cap]
    size_t rev_cap;
    size_t n_rev;
    size_t n_tail;         // reverted pairs that came from the unclaimed tail
};

inline bool settle_is_lost(const uint8_t* lost, int64_t n_nodes, int32_t nid,
                           int* status) {
    if (lost == nullptr) return false;
    if (nid < 0 || static_cast<int64_t>(nid) >= n_nodes) {
        *status = SETTLE_ERR_NODE_RANGE;
        return false;
    }
    return lost[nid] != 0;
}

// Bundled class: walk the entries over the placement stream.  An entry
// that misses its gang minimum hands its slots back (cursor restore); an
// entry touching a lost node reverts its slots; unclaimed slots revert at
// the end, a partially consumed first log entry with its remainder.
inline int settle_bundle(const int32_t* log_nodes, const int32_t* log_counts,
                         int64_t n, const int32_t* ntasks,
                         const int32_t* min_needed, int64_t n_entries,
                         const uint8_t* lost, int64_t n_nodes,
                         SettleOut* out) {
    out->n_pieces = out->n_rev = out->n_tail = 0;
    for (int64_t i = 0; i < n; ++i)
        if (log_counts[i] < 0) return SETTLE_ERR_NEGATIVE;
    int64_t ei = 0;
    int32_t eoff = 0;
    for (int64_t b = 0; b < n_entries; ++b) {
        out->outcome[b] = SETTLE_NONE;
        out->full[b] = 0;
        const int64_t ei0 = ei;
        const int32_t eoff0 = eoff;
        const size_t p0 = out->n_pieces;
        int32_t need = ntasks[b];
        int32_t toff = 0;
        while (need > 0 && ei < n) {
            const int32_t cnt = log_counts[ei];
            const int32_t avail = cnt - eoff;
            const int32_t take = avail < need ? avail : need;
            if (out->n_pieces >= out->piece_cap) return SETTLE_ERR_CAPACITY;
            const size_t p = out->n_pieces++;
            out->p_entry[p] = static_cast<int32_t>(b);
            out->p_node[p] = log_nodes[ei];
            out->p_take[p] = take;
            out->p_toff[p] = toff;
            toff += take;
            need -= take;
            eoff += take;
            if (eoff == cnt) {
                ++ei;
                eoff = 0;
            }
        }
        if (ntasks[b] - need < min_needed[b]) {
            ei = ei0;                       // recycle the slots
            eoff = eoff0;
            out->n_pieces = p0;
            out->outcome[b] = SETTLE_GANG_MISS;
            continue;
        }
        bool hit = false;
        if (lost != nullptr) {
            int status = SETTLE_OK;
            for (size_t p = p0; p < out->n_pieces && !hit; ++p)
                hit = settle_is_lost(lost, n_nodes, out->p_node[p], &status);
            if (status != SETTLE_OK) return status;
        }
        if (hit) {
            for (size_t p = p0; p < out->n_pieces; ++p) {
                if (out->n_rev >= out->rev_cap) return SETTLE_ERR_CAPACITY;
                out->rev_node[out->n_rev] = out->p_node[p];
                out->rev_cnt[out->n_rev] = out->p_take[p];
                ++out->n_rev;
            }
            out->n_pieces = p0;
            out->outcome[b] = SETTLE_LOST;
            continue;
        }
        out->outcome[b] = SETTLE_COMMITTED;
        out->full[b] = need == 0;
    }
    if (ei < n) {                           // slots the walk never claimed
        if (eoff) {
            if (out->n_rev >= out->rev_cap) return SETTLE_ERR_CAPACITY;
            out->rev_node[out->n_rev] = log_nodes[ei];
            out->rev_cnt[out->n_rev] = log_counts[ei] - eoff;
            ++out->n_rev;
            ++out->n_tail;
            ++ei;
        }
        for (; ei < n; ++ei) {
            if (out->n_rev >= out->rev_cap) return SETTLE_ERR_CAPACITY;
            out->rev_node[out->n_rev] = log_nodes[ei];
            out->rev_cnt[out->n_rev] = log_counts[ei];
            ++out->n_rev;
            ++out->n_tail;
        }
    }
    return SETTLE_OK;
}

// Plain (single-job) class: non-positive counts are skipped, tasks are
// taken consecutively, and one lost node reverts the whole class.  Uses
// entry index 0; outcome/full need one slot.
inline int settle_plain(const int32_t* log_nodes, const int32_t* log_counts,
                        int64_t n, const uint8_t* lost, int64_t n_nodes,
                        SettleOut* out) {
    out->n_pieces = out->n_rev = out->n_tail = 0;
    out->outcome[0] = SETTLE_NONE;
    out->full[0] = 0;
    bool hit = false;
    int32_t toff = 0;
    for (int64_t e = 0; e < n; ++e) {
        const int32_t cnt = log_counts[e];
        if (cnt <= 0) continue;
        const int32_t nid = log_nodes[e];
        int status = SETTLE_OK;
        if (settle_is_lost(lost, n_nodes, nid, &status)) hit = true;
        if (status != SETTLE_OK) return status;
        if (out->n_pieces >= out->piece_cap) return SETTLE_ERR_CAPACITY;
        const size_t p = out->n_pieces++;
        out->p_entry[p] = 0;
        out->p_node[p] = nid;
        out->p_take[p] = cnt;
        out->p_toff[p] = toff;
        toff += cnt;
    }
    if (out->n_pieces == 0) return SETTLE_OK;
    if (hit) {
        for (size_t p = 0; p < out->n_pieces; ++p) {
            if (out->n_rev >= out->rev_cap) return SETTLE_ERR_CAPACITY;
            out->rev_node[out->n_rev] = out->p_node[p];
            out->rev_cnt[out->n_rev] = out->p_take[p];
            ++out->n_rev;
        }
        out->n_pieces = 0;
        out->outcome[0] = SETTLE_LOST;
        return SETTLE_OK;
    }
    out->outcome[0] = SETTLE_COMMITTED;
    return SETTLE_OK;
}

}  // namespace vamd
