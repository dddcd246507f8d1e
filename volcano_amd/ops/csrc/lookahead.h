// Block lookahead for the per-job loops of vamd_host.cpp.
//
// Those loops compute nothing: each is a chain of dependent loads through
// CPython objects that are cold when the loop reaches them
// (job -> its dict -> the values array -> podgroup -> ... ), one cache miss
// after the other.  The loops therefore run in blocks.  Before the body of
// a block, the lookahead makes a few short passes over the block's
// elements; each pass takes ONE hop of the chain for every element and
// prefetches what the next pass will dereference, so the misses of a whole
// block are in flight together instead of one at a time.
//
// SAFETY INVARIANT — everything in this file and every lookahead built
// from it keeps to it:
//
//  * The lookahead changes nothing: no reference counts, no stores, no
//    allocation, no error indicator.
//  * It runs no Python code: no attribute protocol, no hashing, no
//    comparison of anything but exact `str` objects.  Hashes of non-str
//    keys (the status enums) are taken by the caller BEFORE the first
//    block, when nothing borrowed is held.
//  * It reads the type word of live objects, and beyond that dereferences
//    only what it has checked to be an exact `dict` or `list`, or an
//    object of the very type whose slot offsets the callers have already
//    resolved.  Anything else is dropped for that element (nullptr), and
//    the body then pays its misses as before.
//  * Because no Python code runs inside a lookahead, every pointer it
//    follows stays valid until it returns.  Nothing it found outlives it:
//    the body of the block may run arbitrary Python code (foreign types,
//    handlers, rich comparison) and re-reads everything through the
//    object protocol.  The only thing that survives is the prefetch
//    itself, and prefetching a stale address is harmless.
//  * Interpreter-internal layout (PyDictObject::ma_keys / ma_values, the
//    keys object, _PyObject_GetDictPtr) yields prefetch addresses only and
//    never decides a result.  It is compiled for CPython 3.10 alone; on
//    any other version these hops return nullptr ("no lookahead") and the
//    results are the same.
#pragma once

#include <Python.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace vamd {
namespace la {

constexpr Py_ssize_t kMaxBlock = 128;      // scratch array size
constexpr Py_ssize_t kDefaultBlock = 64;   // see profiles/BENCH_NOTES.md
#ifndef VAMD_LA_MIN_WINDOW
#define VAMD_LA_MIN_WINDOW 4               // measured: BENCH_NOTES.md
#endif
constexpr Py_ssize_t kMinWindow = VAMD_LA_MIN_WINDOW;   // shorter runs skip
constexpr Py_ssize_t kMaxTasks = 32;       // tasks prefetched per job
constexpr int kLine = 64;

#if PY_VERSION_HEX >= 0x030A0000 && PY_VERSION_HEX < 0x030B0000
#define VAMD_LA_DICT_LAYOUT 1
#else
#define VAMD_LA_DICT_LAYOUT 0
#endif

// Per-call switch: VAMD_HOST_PREFETCH=0 turns every lookahead off;
// VAMD_HOST_PREFETCH_BLOCK=<n> overrides the block size (8..128).
struct Config {
    bool on;
    Py_ssize_t block;
};

inline Config config() {
    Config c{true, kDefaultBlock};
    const char* v = std::getenv("VAMD_HOST_PREFETCH");
    if (v != nullptr && v[0] == '0' && v[1] == '\0') c.on = false;
    const char* b = std::getenv("VAMD_HOST_PREFETCH_BLOCK");
    if (b != nullptr && *b != '\0') {
        const long n = std::strtol(b, nullptr, 10);
        if (n >= 8 && n <= kMaxBlock) c.block = n;
    }
    return c;
}

inline void pf(const void* p) {
    if (p != nullptr) __builtin_prefetch(p, 0, 3);
}

// Every line of [p, p + bytes), at most `max_lines` of them.
inline void pf_span(const void* p, Py_ssize_t bytes, int max_lines = 8) {
    if (p == nullptr || bytes <= 0) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    uintptr_t line = a & ~static_cast<uintptr_t>(kLine - 1);
    const uintptr_t end = a + static_cast<uintptr_t>(bytes);
    for (int i = 0; line < end && i < max_lines; ++i, line += kLine)
        __builtin_prefetch(reinterpret_cast<const void*>(line), 0, 3);
}

// Object header hop: the type word and, for the small dict-backed classes,
// the dict pointer behind it.  Allocator blocks are 16-byte aligned, so
// 32 bytes can straddle two lines.
inline void pf_obj(const PyObject* o) { pf_span(o, 32, 2); }
inline void pf_dict(const PyObject* o) { pf_span(o, sizeof(PyDictObject), 2); }
inline void pf_list(const PyObject* o) { pf_span(o, sizeof(PyListObject), 2); }

// Cached hash of an exact str, or -1.
inline Py_hash_t str_hash(PyObject* s) {
    if (s == nullptr || !PyUnicode_CheckExact(s)) return -1;
    return reinterpret_cast<PyASCIIObject*>(s)->hash;
}

inline bool same_str(PyObject* a, PyObject* b) {
    if (!PyUnicode_CheckExact(a) || !PyUnicode_CheckExact(b)) return false;
    if (!PyUnicode_IS_READY(a) || !PyUnicode_IS_READY(b)) return false;
    const Py_ssize_t n = PyUnicode_GET_LENGTH(a);
    if (n != PyUnicode_GET_LENGTH(b) ||
        PyUnicode_KIND(a) != PyUnicode_KIND(b))
        return false;
    return std::memcmp(PyUnicode_DATA(a), PyUnicode_DATA(b),
                       static_cast<size_t>(n) * PyUnicode_KIND(a)) == 0;
}

#if VAMD_LA_DICT_LAYOUT
// Mirror of CPython 3.10's keys object (Objects/dict-common.h).
struct KeysHead {
    Py_ssize_t dk_refcnt;
    Py_ssize_t dk_size;            // power of two
    void* dk_lookup;
    Py_ssize_t dk_usable;
    Py_ssize_t dk_nentries;
    // char dk_indices[dk_size * width]; KeyEntry dk_entries[];
};
struct KeyEntry {
    Py_hash_t me_hash;
    PyObject* me_key;
    PyObject* me_value;            // unused in a split table
};

struct Keys {
    const KeysHead* h;
    Py_ssize_t size;
    int width;
    const char* indices;
    const KeyEntry* entries;

    explicit Keys(const PyDictObject* d)
        : h(reinterpret_cast<const KeysHead*>(d->ma_keys)) {
        size = h->dk_size;
        width = size <= 0xff ? 1 : size <= 0xffff ? 2
              : size <= 0xffffffffLL ? 4 : 8;
        indices = reinterpret_cast<const char*>(h + 1);
        entries = reinterpret_cast<const KeyEntry*>(indices + size * width);
    }
    bool sane() const { return size > 0 && (size & (size - 1)) == 0; }
    const char* index_addr(size_t i) const { return indices + i * width; }
    Py_ssize_t index(size_t i) const {
        const char* p = index_addr(i);
        switch (width) {
        case 1: return *reinterpret_cast<const int8_t*>(p);
        case 2: return *reinterpret_cast<const int16_t*>(p);
        case 4: return *reinterpret_cast<const int32_t*>(p);
        default: return static_cast<Py_ssize_t>(
                     *reinterpret_cast<const int64_t*>(p));
        }
    }
};
#endif

// Instance-dict hop, pass 1: the object's header is in cache; find its
// __dict__ and prefetch the dict object.  The result is not yet known to
// be a dict — dict_storage() checks that one pass later.
inline PyObject* inst_dict(PyObject* o) {
#if VAMD_LA_DICT_LAYOUT
    if (o == nullptr) return nullptr;
    PyObject** dp = _PyObject_GetDictPtr(o);
    if (dp == nullptr) return nullptr;
    PyObject* d = *dp;
    if (d != nullptr) pf_dict(d);
    return d;
#else
    (void)o;
    return nullptr;
#endif
}

// Pass 2 (also the first pass over a dict-valued attribute): the dict
// object is in cache; keep it only when it is an exact dict and prefetch
// its keys and values storage, sized from ma_used.  The keys of a split
// table are shared by all instances of the class, so one line suffices.
inline PyObject* dict_storage(PyObject* d) {
#if VAMD_LA_DICT_LAYOUT
    if (d == nullptr || !PyDict_CheckExact(d)) return nullptr;
    const PyDictObject* mp = reinterpret_cast<const PyDictObject*>(d);
    const Py_ssize_t used = mp->ma_used;
    if (mp->ma_values != nullptr) {
        pf(mp->ma_keys);
        pf_span(mp->ma_values, (used > 0 ? used : 1) * 8, 4);
    } else {
        // header, index table (about 2 bytes per entry), 24-byte entries
        pf_span(mp->ma_keys, 40 + used * 26, 8);
    }
    return d;
#else
    (void)d;
    return nullptr;
#endif
}

#if VAMD_LA_DICT_LAYOUT
inline bool keys_of(PyObject* d, Keys* out) {
    if (d == nullptr || !PyDict_CheckExact(d)) return false;
    *out = Keys(reinterpret_cast<const PyDictObject*>(d));
    return out->sane();
}
#endif

// Two extra passes for a dict too large for dict_storage(): the index
// slot of `hash`, then the entry it names (first probe position only).
inline void dict_pf_index(PyObject* d, Py_hash_t hash) {
#if VAMD_LA_DICT_LAYOUT
    if (d == nullptr || !PyDict_CheckExact(d)) return;
    Keys k(reinterpret_cast<const PyDictObject*>(d));
    if (!k.sane()) return;
    pf(k.index_addr(static_cast<size_t>(hash) &
                    static_cast<size_t>(k.size - 1)));
#else
    (void)d; (void)hash;
#endif
}

inline void dict_pf_entry(PyObject* d, Py_hash_t hash) {
#if VAMD_LA_DICT_LAYOUT
    if (d == nullptr || !PyDict_CheckExact(d)) return;
    Keys k(reinterpret_cast<const PyDictObject*>(d));
    if (!k.sane()) return;
    const Py_ssize_t ix = k.index(static_cast<size_t>(hash) &
                                  static_cast<size_t>(k.size - 1));
    if (ix >= 0 && ix < k.h->dk_nentries) pf_span(&k.entries[ix], 24, 2);
#else
    (void)d; (void)hash;
#endif
}

// Pass 3: borrowed value of `key` in an exact dict whose storage is in
// cache, or nullptr.  Keys match by identity, or as equal exact strs; no
// other comparison is made, so no Python code runs.  `hash` must be the
// key's hash (-1: skip).
inline PyObject* dict_value(PyObject* d, PyObject* key, Py_hash_t hash) {
#if VAMD_LA_DICT_LAYOUT
    if (d == nullptr || hash == -1 || !PyDict_CheckExact(d)) return nullptr;
    const PyDictObject* mp = reinterpret_cast<const PyDictObject*>(d);
    Keys k(mp);
    if (!k.sane()) return nullptr;
    const size_t mask = static_cast<size_t>(k.size - 1);
    size_t perturb = static_cast<size_t>(hash);
    size_t i = perturb & mask;
    for (Py_ssize_t tries = 0; tries <= k.size; ++tries) {
        const Py_ssize_t ix = k.index(i);
        if (ix == -1) return nullptr;                    // DKIX_EMPTY
        if (ix >= 0) {
            if (ix >= k.h->dk_nentries) return nullptr;
            const KeyEntry* ep = &k.entries[ix];
            if (ep->me_key == key ||
                (ep->me_hash == hash && ep->me_key != nullptr &&
                 same_str(ep->me_key, key)))
                return mp->ma_values != nullptr ? mp->ma_values[ix]
                                                : ep->me_value;
        }
        perturb >>= 5;
        i = (i * 5 + perturb + 1) & mask;
    }
    return nullptr;
#else
    (void)d; (void)key; (void)hash;
    return nullptr;
#endif
}

// List hop, pass 1: the list object is in cache; keep it only when it is
// an exact list and prefetch its item array (first `max_items`).
inline PyObject* list_items(PyObject* l, Py_ssize_t max_items = kMaxTasks) {
    if (l == nullptr || !PyList_CheckExact(l)) return nullptr;
    Py_ssize_t n = PyList_GET_SIZE(l);
    if (n > max_items) n = max_items;
    pf_span(reinterpret_cast<PyListObject*>(l)->ob_item, n * 8, 8);
    return l;
}

// The slot a list's next append writes (the tail of its item array).
inline void pf_list_tail(PyObject* l) {
    if (l == nullptr || !PyList_CheckExact(l)) return;
    PyObject** items = reinterpret_cast<PyListObject*>(l)->ob_item;
    if (items != nullptr) pf(items + PyList_GET_SIZE(l));
}

}  // namespace la
}  // namespace vamd
