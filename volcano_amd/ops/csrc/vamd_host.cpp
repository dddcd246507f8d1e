// _vamd_host: CPython shell around settle_core.h.  One call per cycle
// replaces the interpreted slot walk of AllocateAction._apply: it settles
// every class's placement log and performs the per-task object updates
// (node_name / status stores, node batch appends, per-job bind lists)
// through direct C-API calls.  Device-side reverts, event handlers, the
// binder and pod-group updates stay in Python and get their arguments
// back from here in walk order.
//
// The other per-job loops of a cycle live here too: the JobTable column
// scan (scan_jobs), the fused-run bundle entries of the plan builder
// (bundle_entries) and the bulk pod-group phase store
// (set_podgroup_phase).  Each has its Python loop as oracle and fallback.
//
// All five loops are chains of dependent loads through cold objects; they
// run in blocks with a prefetching lookahead in front of each block
// (lookahead.h states the technique and its safety invariant).
//
// Host-only C++ (no HIP); not linked against libpython.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <structmember.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "lookahead.h"
#include "settle_core.h"

namespace {

namespace la = vamd::la;

struct Ref {                       // owning reference, released on scope exit
    PyObject* p;
    explicit Ref(PyObject* o = nullptr) : p(o) {}
    ~Ref() { Py_XDECREF(p); }
    Ref(const Ref&) = delete;
    Ref& operator=(const Ref&) = delete;
    explicit operator bool() const { return p != nullptr; }
    PyObject* release() { PyObject* o = p; p = nullptr; return o; }
    void reset(PyObject* o) { Py_XDECREF(p); p = o; }
};

struct Buf {                       // contiguous buffer view
    Py_buffer v;
    bool held = false;
    ~Buf() { if (held) PyBuffer_Release(&v); }
    bool get(PyObject* o, Py_ssize_t itemsize, const char* what,
             int flags = PyBUF_C_CONTIGUOUS) {
        if (PyObject_GetBuffer(o, &v, flags) != 0) return false;
        held = true;
        if (v.itemsize != itemsize) {
            PyErr_Format(PyExc_TypeError, "%s: expected itemsize %zd, got %zd",
                         what, itemsize, v.itemsize);
            return false;
        }
        return true;
    }
    // A writable integer column of exactly `n` items.
    bool get_column(PyObject* o, Py_ssize_t itemsize, Py_ssize_t n,
                    const char* what, bool writable) {
        int flags = PyBUF_C_CONTIGUOUS | PyBUF_FORMAT;
        if (writable) flags |= PyBUF_WRITABLE;
        if (!get(o, itemsize, what, flags)) return false;
        const char* f = v.format ? v.format : "b";
        if (*f == '<' || *f == '=' || *f == '@') ++f;
        if (f[0] == '\0' || f[1] != '\0' ||
            std::strchr("bBhHiIlLqQnN", f[0]) == nullptr) {
            PyErr_Format(PyExc_TypeError, "%s: expected an integer column",
                         what);
            return false;
        }
        if (count() != n) {
            PyErr_Format(PyExc_ValueError, "%s: expected %zd rows, got %zd",
                         what, n, count());
            return false;
        }
        return true;
    }
    Py_ssize_t count() const { return v.len / v.itemsize; }
};

PyObject *s_bundle, *s_log_off, *s_job_key, *s_tclass, *s_tasks, *s_ntasks,
    *s_min_needed, *s_job, *s_key, *s_name, *s_batches, *s_node_name,
    *s_status, *s_f, *s_r, *s_task_status_index, *s_occ, *s_alloc_vec,
    *s_podgroup, *s_phase, *s_tver, *s_gated, *s_job_gated, *s_values;

struct TaskStore;

// Block lookaheads of the five loops, defined below the attribute caches
// they read.  Each obeys the invariant of lookahead.h: no stores, no
// reference counts, no Python code, nothing kept past its return.
void la_scan_block(PyObject* jobs, Py_ssize_t k0, Py_ssize_t n,
                   PyObject* pending, Py_hash_t h_pending, PyObject* failed,
                   Py_hash_t h_failed);
void la_phase_block(PyObject* jobs, Py_ssize_t k0, Py_ssize_t n);
void la_bundle_block(PyObject* jobs_l, Py_ssize_t k0, Py_ssize_t n,
                     PyObject* pending, Py_hash_t h_pending);
void la_finish_block(PyObject* by_job, Py_ssize_t pos, Py_ssize_t n,
                     PyObject* jobs, PyObject* pending, Py_hash_t h_pending,
                     PyObject* bound, Py_hash_t h_bound);
void la_entries(PyObject* bundle, Py_ssize_t b0, Py_ssize_t n);
void la_commit_block(PyObject* bundle, Py_ssize_t b0, Py_ssize_t n,
                     const vamd::SettleOut& so, size_t pp, PyObject* nodes,
                     const TaskStore& ts);

// Hash of a non-str dict key (a status enum: hashing one runs Python
// code), taken once per call before the first block; -1 turns the hops
// through that key off.
Py_hash_t la_key_hash(PyObject* key) {
    const Py_hash_t h = PyObject_Hash(key);
    if (h == -1) PyErr_Clear();
    return h;
}

// Offset of a plain object-valued __slots__ member of `tp`, or -1 when
// `name` is anything else (property, instance-dict attribute, read-only
// or typed member) or the type customizes attribute stores.
Py_ssize_t slot_offset(PyTypeObject* tp, PyObject* name) {
    if (tp->tp_setattro != PyObject_GenericSetAttr) return -1;
    Ref d(PyObject_GetAttr(reinterpret_cast<PyObject*>(tp), name));
    if (!d) {
        PyErr_Clear();
        return -1;
    }
    if (Py_TYPE(d.p) != &PyMemberDescr_Type) return -1;
    PyMemberDescrObject* md = reinterpret_cast<PyMemberDescrObject*>(d.p);
    if (md->d_member->type != T_OBJECT_EX || md->d_member->flags != 0 ||
        !PyType_IsSubtype(tp, PyDescr_TYPE(md)))
        return -1;
    return md->d_member->offset;
}

// Stores of node_name/status on tasks.  The task type seen first gets its
// two slot offsets resolved once; its instances are then written in place
// (what the member descriptor's setter does, minus the lookup).  Every
// other object goes through PyObject_SetAttr.
struct TaskStore {
    Ref type;
    Py_ssize_t off_node = -1, off_status = -1;

    static void put(PyObject* t, Py_ssize_t off, PyObject* v) {
        PyObject** slot = reinterpret_cast<PyObject**>(
            reinterpret_cast<char*>(t) + off);
        PyObject* old = *slot;
        Py_INCREF(v);
        *slot = v;
        Py_XDECREF(old);
    }

    bool store(PyObject* t, PyObject* name, PyObject* status) {
        if (!type) {
            PyTypeObject* tp = Py_TYPE(t);
            Py_INCREF(tp);
            type.reset(reinterpret_cast<PyObject*>(tp));
            off_node = slot_offset(tp, s_node_name);
            off_status = slot_offset(tp, s_status);
        }
        if (reinterpret_cast<PyObject*>(Py_TYPE(t)) == type.p &&
            off_node >= 0 && off_status >= 0) {
            put(t, off_node, name);
            put(t, off_status, status);
            return true;
        }
        return PyObject_SetAttr(t, s_node_name, name) == 0 &&
               PyObject_SetAttr(t, s_status, status) == 0;
    }
};

// The walk allocates one small list per piece and per job.  With the
// cyclic collector live, every few hundred of them start a young-
// generation pass that traverses the lists built so far, task by task —
// a third of the walk's time at 100k tasks.  None of these lists is
// garbage before the call returns, so the collector is paused for the
// bounded duration of the call and catches up on the next allocation.
struct GcPause {
#if PY_VERSION_HEX >= 0x030A0000
    int was = PyGC_Disable();
    ~GcPause() { if (was) PyGC_Enable(); }
#endif
};

// Lists created here that hold only task objects leave the collector's
// sight right after creation.  A TaskInfo is slotted and what it reaches
// (strings, numbers, its Resource, its Pod manifest) never refers back to
// a scheduler-side list, so such a list cannot sit on a reference cycle:
// it dies by reference count, and the collector no longer walks 100k task
// pointers per young-generation pass (the catch-up bill that used to
// arrive right after the GcPause below ended).
inline void untrack_task_list(PyObject* list) { PyObject_GC_UnTrack(list); }

struct Walk {
    TaskStore tstore;
    PyObject* jobs;
    PyObject* alias;
    PyObject* nodes;               // list, node_id order
    PyObject* bound;
    bool want_fire;
    Ref bind_by_job, committed, full, events;
    std::vector<int64_t> acc_rows, acc_cls;
    std::vector<double> acc_cnts;
    long n_committed = 0, n_missed = 0, n_lost = 0, n_tail = 0;

    // Assign pieces [p0, p1) of `so` to the next tasks of `job`.
    bool commit(PyObject* job, PyObject* tasks, Py_ssize_t c,
                const vamd::SettleOut& so, size_t p0, size_t p1,
                bool exact) {
        Ref key(PyObject_GetAttr(job, s_key));
        if (!key) return false;
        PyObject* jl = PyDict_GetItemWithError(bind_by_job.p, key.p);
        if (jl == nullptr) {
            if (PyErr_Occurred()) return false;
            Ref fresh(PyList_New(0));
            if (!fresh || PyDict_SetItem(bind_by_job.p, key.p, fresh.p) != 0)
                return false;
            untrack_task_list(fresh.p);
            jl = fresh.p;          // the dict keeps it alive
        }
        // the handler argument lists stay tracked: plugin code may store
        // anything in them
        Ref f_nodes, f_cnts, f_tasks;
        if (want_fire) {
            f_nodes.reset(PyList_New(0));
            f_cnts.reset(PyList_New(0));
            f_tasks.reset(PyList_New(0));
            if (!f_nodes || !f_cnts || !f_tasks) return false;
        }
        const Py_ssize_t n_nodes = PyList_GET_SIZE(nodes);
        for (size_t p = p0; p < p1; ++p) {
            const int32_t nid = so.p_node[p];
            const int32_t take = so.p_take[p];
            const int32_t toff = so.p_toff[p];
            if (nid < 0 || nid >= n_nodes) {
                PyErr_Format(PyExc_IndexError,
                             "placement log names node %d of %zd",
                             static_cast<int>(nid), n_nodes);
                return false;
            }
            PyObject* ni = PyList_GET_ITEM(nodes, nid);
            Ref name(PyObject_GetAttr(ni, s_name));
            if (!name) return false;
            Ref sl(PyList_GetSlice(tasks, toff,
                                   static_cast<Py_ssize_t>(toff) + take));
            if (!sl) return false;
            untrack_task_list(sl.p);
            const Py_ssize_t k = PyList_GET_SIZE(sl.p);
            if (exact && k != take) {
                PyErr_SetString(PyExc_RuntimeError,
                                "class has fewer tasks than its log places");
                return false;
            }
            for (Py_ssize_t i = 0; i < k; ++i) {
                PyObject* t = PyList_GET_ITEM(sl.p, i);
                if (!tstore.store(t, name.p, bound)) return false;
            }
            Ref batches(PyObject_GetAttr(ni, s_batches));
            if (!batches) return false;
            if (!PyList_Check(batches.p)) {
                PyErr_SetString(PyExc_TypeError, "_batches must be a list");
                return false;
            }
            if (PyList_Append(batches.p, sl.p) != 0) return false;
            acc_rows.push_back(nid);
            acc_cnts.push_back(static_cast<double>(take));
            acc_cls.push_back(c);
            const Py_ssize_t at = PyList_GET_SIZE(jl);
            if (PyList_SetSlice(jl, at, at, sl.p) != 0) return false;
            if (want_fire) {
                Ref a(PyLong_FromLong(nid)), b(PyLong_FromLong(take));
                if (!a || !b || PyList_Append(f_nodes.p, a.p) != 0 ||
                    PyList_Append(f_cnts.p, b.p) != 0)
                    return false;
                const Py_ssize_t ft = PyList_GET_SIZE(f_tasks.p);
                if (PyList_SetSlice(f_tasks.p, ft, ft, sl.p) != 0)
                    return false;
            }
        }
        if (PyDict_SetItem(committed.p, key.p, job) != 0) return false;
        if (want_fire) {
            Ref ev(Py_BuildValue("(OnOOO)", s_f, c, f_nodes.p, f_cnts.p,
                                 f_tasks.p));
            if (!ev || PyList_Append(events.p, ev.p) != 0) return false;
        }
        ++n_committed;
        return true;
    }

    bool revert(Py_ssize_t c, const vamd::SettleOut& so) {
        if (so.n_rev == 0) return true;
        Ref pairs(PyList_New(static_cast<Py_ssize_t>(so.n_rev)));
        if (!pairs) return false;
        for (size_t i = 0; i < so.n_rev; ++i) {
            PyObject* t = Py_BuildValue("(ii)", so.rev_node[i], so.rev_cnt[i]);
            if (t == nullptr) return false;
            PyList_SET_ITEM(pairs.p, static_cast<Py_ssize_t>(i), t);
        }
        Ref ev(Py_BuildValue("(OnO)", s_r, c, pairs.p));
        return ev && PyList_Append(events.p, ev.p) == 0;
    }
};

bool settle_error(int st) {
    switch (st) {
    case vamd::SETTLE_OK:
        return false;
    case vamd::SETTLE_ERR_CAPACITY:
        PyErr_SetString(PyExc_RuntimeError, "settle output capacity exceeded");
        break;
    case vamd::SETTLE_ERR_NEGATIVE:
        PyErr_SetString(PyExc_ValueError, "negative count in placement log");
        break;
    default:
        PyErr_SetString(PyExc_IndexError,
                        "placement log names a node outside the lost mask");
    }
    return true;
}

bool attr_long(PyObject* o, PyObject* name, long* out) {
    Ref v(PyObject_GetAttr(o, name));
    if (!v) return false;
    *out = PyLong_AsLong(v.p);
    return !(*out == -1 && PyErr_Occurred());
}

// Mapping lookup: borrowed-free new reference, nullptr without an error
// set when the key is absent.
PyObject* map_get(PyObject* m, PyObject* key) {
    if (PyDict_Check(m)) {
        PyObject* v = PyDict_GetItemWithError(m, key);
        Py_XINCREF(v);
        return v;
    }
    PyObject* v = PyObject_GetItem(m, key);
    if (v == nullptr && PyErr_ExceptionMatches(PyExc_KeyError)) PyErr_Clear();
    return v;
}

PyObject* vec_bytes(const void* data, size_t nbytes) {
    return PyBytes_FromStringAndSize(static_cast<const char*>(data),
                                     static_cast<Py_ssize_t>(nbytes));
}

PyObject* apply_walk(PyObject*, PyObject* args) {
    PyObject *classes, *jobs, *alias, *nodes, *o_jf, *o_cj, *o_ln, *o_lc,
        *o_ll, *o_lost, *bound;
    int want_fire;
    if (!PyArg_ParseTuple(args, "OOOOOOOOOOOp", &classes, &jobs, &alias,
                          &nodes, &o_jf, &o_cj, &o_ln, &o_lc, &o_ll, &o_lost,
                          &bound, &want_fire))
        return nullptr;
    if (!PyList_Check(classes) || !PyList_Check(nodes)) {
        PyErr_SetString(PyExc_TypeError, "classes and nodes must be lists");
        return nullptr;
    }
    Buf jf, cj, ln, lc, ll, lost;
    if (!jf.get(o_jf, 1, "job_flag") || !cj.get(o_cj, 4, "class_job") ||
        !ln.get(o_ln, 4, "log_nodes") || !lc.get(o_lc, 4, "log_counts") ||
        !ll.get(o_ll, 4, "log_len"))
        return nullptr;
    const uint8_t* lost_p = nullptr;
    int64_t lost_n = 0;
    if (o_lost != Py_None) {
        if (!lost.get(o_lost, 1, "lost mask")) return nullptr;
        lost_p = static_cast<const uint8_t*>(lost.v.buf);
        lost_n = lost.count();
    }
    const Py_ssize_t C = PyList_GET_SIZE(classes);
    const Py_ssize_t log_total = ln.count();
    if (cj.count() < C || ll.count() < C || lc.count() != log_total) {
        PyErr_SetString(PyExc_ValueError,
                        "result arrays do not cover the plan's classes");
        return nullptr;
    }
    const uint8_t* jf_p = static_cast<const uint8_t*>(jf.v.buf);
    const int32_t* cj_p = static_cast<const int32_t*>(cj.v.buf);
    const int32_t* ln_p = static_cast<const int32_t*>(ln.v.buf);
    const int32_t* lc_p = static_cast<const int32_t*>(lc.v.buf);
    const int32_t* ll_p = static_cast<const int32_t*>(ll.v.buf);
    const Py_ssize_t n_jobs = jf.count();
    const la::Config pfc = la::config();

    GcPause gc_pause;
    Walk w;
    w.jobs = jobs;
    w.alias = alias;
    w.nodes = nodes;
    w.bound = bound;
    w.want_fire = want_fire != 0;
    w.bind_by_job.reset(PyDict_New());
    w.committed.reset(PyDict_New());
    w.full.reset(PySet_New(nullptr));
    w.events.reset(PyList_New(0));
    if (!w.bind_by_job || !w.committed || !w.full || !w.events)
        return nullptr;

    std::vector<int32_t> p_entry, p_node, p_take, p_toff, rev_node, rev_cnt,
        e_ntasks, e_min;
    std::vector<uint8_t> outcome, full;

    for (Py_ssize_t c = 0; c < C; ++c) {
        const int32_t j = cj_p[c];
        if (j < 0 || j >= n_jobs) {
            PyErr_SetString(PyExc_IndexError, "class_job outside job_flag");
            return nullptr;
        }
        if (!jf_p[j]) continue;
        const int64_t n = ll_p[c];
        if (n == 0) continue;
        PyObject* cp = PyList_GET_ITEM(classes, c);
        long off;
        if (!attr_long(cp, s_log_off, &off)) return nullptr;
        if (n < 0 || off < 0 || off + n > log_total) {
            PyErr_SetString(PyExc_IndexError,
                            "class log slice outside the log arrays");
            return nullptr;
        }
        Ref bundle(PyObject_GetAttr(cp, s_bundle));
        if (!bundle) return nullptr;
        const bool plain = bundle.p == Py_None;
        if (!plain && !PyList_Check(bundle.p)) {
            PyErr_SetString(PyExc_TypeError, "bundle must be a list or None");
            return nullptr;
        }
        const Py_ssize_t n_entries = plain ? 1 : PyList_GET_SIZE(bundle.p);
        const size_t cap = static_cast<size_t>(n) +
                           static_cast<size_t>(n_entries);
        p_entry.resize(cap); p_node.resize(cap);
        p_take.resize(cap); p_toff.resize(cap);
        rev_node.resize(cap); rev_cnt.resize(cap);
        outcome.resize(static_cast<size_t>(n_entries) + 1);
        full.resize(static_cast<size_t>(n_entries) + 1);
        vamd::SettleOut so{};
        so.p_entry = p_entry.data(); so.p_node = p_node.data();
        so.p_take = p_take.data(); so.p_toff = p_toff.data();
        so.piece_cap = cap;
        so.outcome = outcome.data(); so.full = full.data();
        so.rev_node = rev_node.data(); so.rev_cnt = rev_cnt.data();
        so.rev_cap = cap;

        if (plain) {
            Ref jkey(PyObject_GetAttr(cp, s_job_key));
            if (!jkey) return nullptr;
            Ref job(map_get(jobs, jkey.p));
            if (!job && PyErr_Occurred()) return nullptr;
            int truth = job ? PyObject_IsTrue(job.p) : 0;
            if (truth < 0) return nullptr;
            if (!truth) {
                Ref real(PyObject_GetItem(alias, jkey.p));
                if (!real) return nullptr;
                job.reset(PyObject_GetItem(jobs, real.p));
                if (!job) return nullptr;
            }
            if (settle_error(vamd::settle_plain(ln_p + off, lc_p + off, n,
                                                lost_p, lost_n, &so)))
                return nullptr;
            if (so.outcome[0] == vamd::SETTLE_LOST) {
                ++w.n_lost;
                if (!w.revert(c, so)) return nullptr;
            } else if (so.outcome[0] == vamd::SETTLE_COMMITTED) {
                Ref tclass(PyObject_GetAttr(cp, s_tclass));
                if (!tclass) return nullptr;
                Ref tasks(PyObject_GetAttr(tclass.p, s_tasks));
                if (!tasks) return nullptr;
                if (!PyList_Check(tasks.p)) {
                    PyErr_SetString(PyExc_TypeError, "tasks must be a list");
                    return nullptr;
                }
                if (!w.commit(job.p, tasks.p, c, so, 0, so.n_pieces, true))
                    return nullptr;
            }
            continue;
        }

        e_ntasks.resize(static_cast<size_t>(n_entries));
        e_min.resize(static_cast<size_t>(n_entries));
        const bool ahead = pfc.on && n_entries >= la::kMinWindow;
        for (Py_ssize_t b = 0; b < n_entries; ++b) {
            // one hop only (the sizes are small cached ints), so this
            // pass fetches the block AFTER the one it is about to read
            if (ahead && b % pfc.block == 0) {
                if (b == 0) la_entries(bundle.p, 0, pfc.block);
                la_entries(bundle.p, b + pfc.block, pfc.block);
            }
            PyObject* be = PyList_GET_ITEM(bundle.p, b);
            long nt, mn;
            if (!attr_long(be, s_ntasks, &nt) ||
                !attr_long(be, s_min_needed, &mn))
                return nullptr;
            if (nt < INT32_MIN || nt > INT32_MAX || mn < INT32_MIN ||
                mn > INT32_MAX) {
                PyErr_SetString(PyExc_OverflowError, "bundle entry size");
                return nullptr;
            }
            e_ntasks[b] = static_cast<int32_t>(nt);
            e_min[b] = static_cast<int32_t>(mn);
        }
        if (settle_error(vamd::settle_bundle(ln_p + off, lc_p + off, n,
                                             e_ntasks.data(), e_min.data(),
                                             n_entries, lost_p, lost_n, &so)))
            return nullptr;
        size_t pp = 0;
        for (Py_ssize_t b = 0; b < n_entries; ++b) {
            if (ahead && b % pfc.block == 0)
                la_commit_block(bundle.p, b, pfc.block, so, pp, nodes,
                                w.tstore);
            const uint8_t oc = so.outcome[b];
            if (oc == vamd::SETTLE_GANG_MISS) { ++w.n_missed; continue; }
            if (oc == vamd::SETTLE_LOST) { ++w.n_lost; continue; }
            if (oc != vamd::SETTLE_COMMITTED) continue;
            size_t pe = pp;
            while (pe < so.n_pieces && so.p_entry[pe] == b) ++pe;
            PyObject* be = PyList_GET_ITEM(bundle.p, b);
            Ref job(PyObject_GetAttr(be, s_job));
            if (!job) return nullptr;
            Ref jkey(PyObject_GetAttr(be, s_job_key));
            if (!jkey) return nullptr;
            if (job.p == Py_None) {
                job.reset(PyObject_GetItem(jobs, jkey.p));
                if (!job) return nullptr;
            }
            Ref tasks(PyObject_GetAttr(be, s_tasks));
            if (!tasks) return nullptr;
            if (!PyList_Check(tasks.p)) {
                PyErr_SetString(PyExc_TypeError, "tasks must be a list");
                return nullptr;
            }
            if (!w.commit(job.p, tasks.p, c, so, pp, pe, false))
                return nullptr;
            if (so.full[b] && PySet_Add(w.full.p, jkey.p) != 0)
                return nullptr;
            pp = pe;
        }
        w.n_tail += static_cast<long>(so.n_tail);
        if (!w.revert(c, so)) return nullptr;
    }

    Ref rows(vec_bytes(w.acc_rows.data(), w.acc_rows.size() * 8));
    Ref cnts(vec_bytes(w.acc_cnts.data(), w.acc_cnts.size() * 8));
    Ref cls(vec_bytes(w.acc_cls.data(), w.acc_cls.size() * 8));
    if (!rows || !cnts || !cls) return nullptr;
    return Py_BuildValue("(OOOOOOO(llll))", rows.p, cnts.p, cls.p,
                         w.bind_by_job.p, w.committed.p, w.full.p,
                         w.events.p, w.n_committed, w.n_missed, w.n_lost,
                         w.n_tail);
}

// JobInfo.finish_bind for every (key, tasks) of by_job, in one call: the
// walk already stored BOUND on the tasks, only the status-bucket move and
// the occupancy count remain.  Wholesale when the batch is the job's whole
// pending bucket (the gang case).
PyObject* finish_binds(PyObject*, PyObject* args) {
    PyObject *by_job, *jobs, *pending, *bound;
    if (!PyArg_ParseTuple(args, "O!OOO", &PyDict_Type, &by_job, &jobs,
                          &pending, &bound))
        return nullptr;
    GcPause gc_pause;                  // one fresh bucket dict per job
    const la::Config pfc = la::config();
    const bool ahead = pfc.on && PyDict_GET_SIZE(by_job) >= la::kMinWindow;
    const Py_hash_t h_pending = ahead ? la_key_hash(pending) : -1;
    const Py_hash_t h_bound = ahead ? la_key_hash(bound) : -1;
    Py_ssize_t pos = 0, seen = 0;
    PyObject *key, *ts;
    for (;;) {
        if (ahead && seen % pfc.block == 0)
            la_finish_block(by_job, pos, pfc.block, jobs, pending, h_pending,
                            bound, h_bound);
        if (!PyDict_Next(by_job, &pos, &key, &ts)) break;
        ++seen;
        Ref job(map_get(jobs, key));
        if (!job) {
            if (PyErr_Occurred()) return nullptr;
            continue;
        }
        if (job.p == Py_None) continue;
        const Py_ssize_t n = PyObject_Length(ts);
        if (n < 0) return nullptr;
        Ref idx(PyObject_GetAttr(job.p, s_task_status_index));
        if (!idx) return nullptr;
        if (!PyDict_Check(idx.p)) {
            PyErr_SetString(PyExc_TypeError,
                            "task_status_index must be a dict");
            return nullptr;
        }
        Ref src(PyDict_GetItemWithError(idx.p, pending));
        if (!src && PyErr_Occurred()) return nullptr;
        Py_XINCREF(src.p);
        if (src && !PyDict_Check(src.p)) {
            PyErr_SetString(PyExc_TypeError, "status bucket must be a dict");
            return nullptr;
        }
        Ref dst(PyDict_GetItemWithError(idx.p, bound));
        if (!dst && PyErr_Occurred()) return nullptr;
        Py_XINCREF(dst.p);
        if (dst && !PyDict_Check(dst.p)) {
            PyErr_SetString(PyExc_TypeError, "status bucket must be a dict");
            return nullptr;
        }
        if (src && PyDict_GET_SIZE(src.p) == n) {
            if (dst && PyDict_GET_SIZE(dst.p) > 0) {
                if (PyDict_Update(dst.p, src.p) != 0) return nullptr;
            } else if (PyDict_SetItem(idx.p, bound, src.p) != 0) {
                return nullptr;
            }
            Ref fresh(PyDict_New());
            if (!fresh || PyDict_SetItem(idx.p, pending, fresh.p) != 0)
                return nullptr;
        } else {
            if (!dst) {
                dst.reset(PyDict_New());
                if (!dst || PyDict_SetItem(idx.p, bound, dst.p) != 0)
                    return nullptr;
            }
            Ref seq(PySequence_Fast(ts, "bind list must be a sequence"));
            if (!seq) return nullptr;
            for (Py_ssize_t i = 0; i < PySequence_Fast_GET_SIZE(seq.p); ++i) {
                PyObject* t = PySequence_Fast_GET_ITEM(seq.p, i);
                Ref tkey(PyObject_GetAttr(t, s_key));
                if (!tkey) return nullptr;
                if (src && PyDict_DelItem(src.p, tkey.p) != 0) {
                    if (!PyErr_ExceptionMatches(PyExc_KeyError))
                        return nullptr;
                    PyErr_Clear();
                }
                if (PyDict_SetItem(dst.p, tkey.p, t) != 0) return nullptr;
            }
        }
        Ref occ(PyObject_GetAttr(job.p, s_occ));
        if (!occ) return nullptr;
        Ref add(PyLong_FromSsize_t(n));
        if (!add) return nullptr;
        Ref sum(PyNumber_Add(occ.p, add.p));   // BOUND occupies, PENDING not
        if (!sum || PyObject_SetAttr(job.p, s_occ, sum.p) != 0 ||
            PyObject_SetAttr(job.p, s_alloc_vec, Py_None) != 0)
            return nullptr;
    }
    Py_RETURN_NONE;
}

// ---- per-job loops of a cycle --------------------------------------------

// One attribute of the objects of one type.  The type seen first gets the
// slot offset resolved once per module; its instances are then read and
// written in place.  Every other object (and every non-slot attribute)
// goes through PyObject_GetAttr / PyObject_SetAttr.
struct SlotAttr {
    PyObject** name;               // interned at module init
    PyTypeObject* type = nullptr;  // strong, kept for the module's life
    Py_ssize_t off = -1;

    explicit SlotAttr(PyObject** n) : name(n) {}

    PyObject** slot(PyObject* o) {
        if (type == nullptr) {
            type = Py_TYPE(o);
            Py_INCREF(type);
            off = slot_offset(type, *name);
        }
        if (Py_TYPE(o) != type || off < 0) return nullptr;
        return reinterpret_cast<PyObject**>(reinterpret_cast<char*>(o) + off);
    }
    PyObject* get(PyObject* o) {   // new reference
        PyObject** s = slot(o);
        if (s != nullptr && *s != nullptr) {
            Py_INCREF(*s);
            return *s;
        }
        return PyObject_GetAttr(o, *name);   // raises for an empty slot
    }
    bool set(PyObject* o, PyObject* v) {
        PyObject** s = slot(o);
        if (s == nullptr) return PyObject_SetAttr(o, *name, v) == 0;
        PyObject* old = *s;
        Py_INCREF(v);
        *s = v;
        Py_XDECREF(old);
        return true;
    }
    // Lookahead only: the borrowed value without the attribute protocol —
    // the slot when it is already resolved for o's type (never resolved
    // here: that runs Python code), else the entry of o's instance dict
    // `d` — or nullptr.
    PyObject* peek(PyObject* o, PyObject* d) const {
        if (o == nullptr) return nullptr;
        if (type != nullptr && Py_TYPE(o) == type && off >= 0)
            return *reinterpret_cast<PyObject**>(
                reinterpret_cast<char*>(o) + off);
        return la::dict_value(d, *name, la::str_hash(*name));
    }
};

SlotAttr a_job_idx(&s_task_status_index), a_job_occ(&s_occ),
    a_job_pg(&s_podgroup), a_job_tver(&s_tver), a_job_key(&s_key),
    a_pg_status(&s_status), a_st_phase(&s_phase), a_task_gated(&s_gated),
    a_node_name(&s_name), a_node_batches(&s_batches);   // peeked only

// getattr(o, name, <absent>): 1 found (new reference in *out), 0 absent,
// -1 error.
int optional_attr(PyObject* o, PyObject* name, PyObject** out) {
#if PY_VERSION_HEX >= 0x030D0000
    return PyObject_GetOptionalAttr(o, name, out);
#else
    return _PyObject_LookupAttr(o, name, out);
#endif
}

// `len(b) if b else 0` for the status bucket `key` of a job's index.
bool bucket_len(PyObject* idx, PyObject* key, int64_t* out) {
    Ref b(map_get(idx, key));
    *out = 0;
    if (!b) return !PyErr_Occurred();
    if (PyDict_Check(b.p)) {
        *out = PyDict_GET_SIZE(b.p);
        return true;
    }
    const int truth = PyObject_IsTrue(b.p);
    if (truth < 0) return false;
    if (truth) {
        const Py_ssize_t n = PyObject_Length(b.p);
        if (n < 0) return false;
        *out = n;
    }
    return true;
}

bool as_i64(PyObject* v, int64_t* out) {
    const long long x = PyLong_AsLongLong(v);
    if (x == -1 && PyErr_Occurred()) return false;
    *out = x;
    return true;
}

// JobTable's per-cycle pass over the jobs: fills the dynamic columns and
// returns the rows whose static-shape version moved.
PyObject* scan_jobs(PyObject*, PyObject* args) {
    PyObject *jobs, *pending, *failed, *pmap, *o_vers, *o_occ, *o_npend,
        *o_nfailed, *o_phase;
    int ph_pending, ph_other;
    if (!PyArg_ParseTuple(args, "O!OOO!iiOOOOO", &PyList_Type, &jobs,
                          &pending, &failed, &PyDict_Type, &pmap, &ph_pending,
                          &ph_other, &o_vers, &o_occ, &o_npend, &o_nfailed,
                          &o_phase))
        return nullptr;
    const Py_ssize_t J = PyList_GET_SIZE(jobs);
    Buf vers, occ, npend, nfailed, phase;
    if (!vers.get_column(o_vers, 8, J, "vers", false) ||
        !occ.get_column(o_occ, 8, J, "occ", true) ||
        !npend.get_column(o_npend, 8, J, "npend", true) ||
        !nfailed.get_column(o_nfailed, 8, J, "nfailed", true) ||
        !phase.get_column(o_phase, 1, J, "phase", true))
        return nullptr;
    if (ph_pending < INT8_MIN || ph_pending > INT8_MAX ||
        ph_other < INT8_MIN || ph_other > INT8_MAX) {
        PyErr_SetString(PyExc_OverflowError, "phase code outside int8");
        return nullptr;
    }
    const int64_t* vers_p = static_cast<const int64_t*>(vers.v.buf);
    int64_t* occ_p = static_cast<int64_t*>(occ.v.buf);
    int64_t* npend_p = static_cast<int64_t*>(npend.v.buf);
    int64_t* nfailed_p = static_cast<int64_t*>(nfailed.v.buf);
    int8_t* phase_p = static_cast<int8_t*>(phase.v.buf);

    Ref dirty(PyList_New(0));
    if (!dirty) return nullptr;
    const la::Config pfc = la::config();
    const bool ahead = pfc.on && J >= la::kMinWindow;
    const Py_hash_t h_pending = ahead ? la_key_hash(pending) : -1;
    const Py_hash_t h_failed = ahead ? la_key_hash(failed) : -1;
    for (Py_ssize_t k = 0; k < J; ++k) {
        if (PyList_GET_SIZE(jobs) != J) {   // an attribute hook resized it
            PyErr_SetString(PyExc_RuntimeError, "job list changed size");
            return nullptr;
        }
        if (ahead && k % pfc.block == 0)
            la_scan_block(jobs, k, pfc.block, pending, h_pending, failed,
                          h_failed);
        Ref job(PyList_GET_ITEM(jobs, k));
        Py_INCREF(job.p);
        Ref v(a_job_occ.get(job.p));
        if (!v || !as_i64(v.p, &occ_p[k])) return nullptr;
        Ref idx(a_job_idx.get(job.p));
        if (!idx || !bucket_len(idx.p, pending, &npend_p[k]) ||
            !bucket_len(idx.p, failed, &nfailed_p[k]))
            return nullptr;
        Ref pg(a_job_pg.get(job.p));
        if (!pg) return nullptr;
        long code = ph_pending;
        if (pg.p != Py_None) {
            Ref st(a_pg_status.get(pg.p));
            if (!st) return nullptr;
            Ref ph(a_st_phase.get(st.p));
            if (!ph) return nullptr;
            PyObject* c = PyDict_GetItemWithError(pmap, ph.p);   // borrowed
            if (c == nullptr) {
                if (PyErr_Occurred()) return nullptr;
                code = ph_other;
            } else {
                code = PyLong_AsLong(c);
                if (code == -1 && PyErr_Occurred()) return nullptr;
                if (code < INT8_MIN || code > INT8_MAX) {
                    PyErr_SetString(PyExc_OverflowError,
                                    "phase code outside int8");
                    return nullptr;
                }
            }
        }
        phase_p[k] = static_cast<int8_t>(code);
        int64_t tver;
        v.reset(a_job_tver.get(job.p));
        if (!v || !as_i64(v.p, &tver)) return nullptr;
        if (tver != vers_p[k]) {
            Ref row(PyLong_FromSsize_t(k));
            if (!row || PyList_Append(dirty.p, row.p) != 0) return nullptr;
        }
    }
    return dirty.release();
}

// The five slots of the plan's BundleEntry type, resolved once per type
// object.  `direct` holds when every one is a plain object slot of exactly
// that type, so an instance can be made by tp_alloc plus five stores.
struct EntryType {
    PyTypeObject* type = nullptr;  // strong
    Py_ssize_t off[5] = {-1, -1, -1, -1, -1};
    bool direct = false;

    void resolve(PyTypeObject* tp) {
        if (tp == type) return;
        Py_INCREF(tp);
        Py_XDECREF(type);
        type = tp;
        PyObject* names[5] = {s_job_key, s_tasks, s_ntasks, s_min_needed,
                              s_job};
        direct = (tp->tp_flags & Py_TPFLAGS_HEAPTYPE) != 0 &&
                 (tp->tp_flags & Py_TPFLAGS_IS_ABSTRACT) == 0 &&
                 tp->tp_alloc != nullptr && tp->tp_itemsize == 0;
        for (int i = 0; i < 5; ++i) {
            off[i] = slot_offset(tp, names[i]);
            if (off[i] < 0 ||
                off[i] + static_cast<Py_ssize_t>(sizeof(PyObject*)) >
                    tp->tp_basicsize)
                direct = false;
        }
    }

    // Steals nothing; returns a new entry.
    PyObject* make(PyObject* key, PyObject* tasks, PyObject* ntasks,
                   PyObject* min_needed, PyObject* job) {
        if (!direct)
            return PyObject_CallFunctionObjArgs(
                reinterpret_cast<PyObject*>(type), key, tasks, ntasks,
                min_needed, job, nullptr);
        PyObject* e = type->tp_alloc(type, 0);   // zeroed slots
        if (e == nullptr) return nullptr;
        PyObject* vals[5] = {key, tasks, ntasks, min_needed, job};
        for (int i = 0; i < 5; ++i) {
            Py_INCREF(vals[i]);
            *reinterpret_cast<PyObject**>(reinterpret_cast<char*>(e) +
                                          off[i]) = vals[i];
        }
        return e;
    }
};

EntryType entry_type;

// ---- block lookaheads ------------------------------------------------------
// Every pass below takes one hop for all elements of the block and
// prefetches what the next pass dereferences; nullptr drops an element.

// Elements [k0, k0 + n) of an exact list, clamped to its current size;
// prefetches their headers and returns the count.
Py_ssize_t la_load(PyObject* list, Py_ssize_t k0, Py_ssize_t n,
                   PyObject** out) {
    const Py_ssize_t size = PyList_GET_SIZE(list);
    if (n > la::kMaxBlock) n = la::kMaxBlock;
    if (k0 < 0 || k0 >= size) return 0;
    if (k0 + n > size) n = size - k0;
    for (Py_ssize_t e = 0; e < n; ++e) {
        out[e] = PyList_GET_ITEM(list, k0 + e);
        la::pf_obj(out[e]);
    }
    return n;
}

// Instance dicts of obj[0..n): two passes (dict object, then its storage).
void la_dicts(PyObject* const* obj, Py_ssize_t n, PyObject** d) {
    for (Py_ssize_t e = 0; e < n; ++e) d[e] = la::inst_dict(obj[e]);
    for (Py_ssize_t e = 0; e < n; ++e) d[e] = la::dict_storage(d[e]);
}

// One attribute hop: obj[e] (header in cache) -> out[e], header
// prefetched.  `out` may be `obj`.
void la_hop(PyObject* const* obj, Py_ssize_t n, const SlotAttr& a,
            PyObject** out) {
    PyObject* d[la::kMaxBlock];
    la_dicts(obj, n, d);
    for (Py_ssize_t e = 0; e < n; ++e) {
        out[e] = a.peek(obj[e], d[e]);
        la::pf_obj(out[e]);
    }
}

void la_phase_block(PyObject* jobs, Py_ssize_t k0, Py_ssize_t n) {
    PyObject* o[la::kMaxBlock];
    n = la_load(jobs, k0, n, o);
    la_hop(o, n, a_job_pg, o);         // job -> podgroup
    la_hop(o, n, a_pg_status, o);      // -> status
    la_hop(o, n, a_st_phase, o);       // -> phase
}

void la_scan_block(PyObject* jobs, Py_ssize_t k0, Py_ssize_t n,
                   PyObject* pending, Py_hash_t h_pending, PyObject* failed,
                   Py_hash_t h_failed) {
    PyObject *job[la::kMaxBlock], *d[la::kMaxBlock], *idx[la::kMaxBlock],
        *pg[la::kMaxBlock];
    n = la_load(jobs, k0, n, job);
    la_dicts(job, n, d);
    for (Py_ssize_t e = 0; e < n; ++e) {
        idx[e] = a_job_idx.peek(job[e], d[e]);
        la::pf_dict(idx[e]);
        pg[e] = a_job_pg.peek(job[e], d[e]);
        la::pf_obj(pg[e]);
        la::pf(a_job_occ.peek(job[e], d[e]));
        la::pf(a_job_tver.peek(job[e], d[e]));
    }
    for (Py_ssize_t e = 0; e < n; ++e) idx[e] = la::dict_storage(idx[e]);
    for (Py_ssize_t e = 0; e < n; ++e) {   // bucket lengths only
        la::pf_dict(la::dict_value(idx[e], pending, h_pending));
        la::pf_dict(la::dict_value(idx[e], failed, h_failed));
    }
    la_hop(pg, n, a_pg_status, pg);
    la_hop(pg, n, a_st_phase, pg);
}

void la_bundle_block(PyObject* jobs_l, Py_ssize_t k0, Py_ssize_t n,
                     PyObject* pending, Py_hash_t h_pending) {
    PyObject *job[la::kMaxBlock], *d[la::kMaxBlock], *b[la::kMaxBlock];
    n = la_load(jobs_l, k0, n, job);
    la_dicts(job, n, d);
    for (Py_ssize_t e = 0; e < n; ++e) {
        b[e] = a_job_idx.peek(job[e], d[e]);
        la::pf_dict(b[e]);
        la::pf(a_job_key.peek(job[e], d[e]));
    }
    for (Py_ssize_t e = 0; e < n; ++e) b[e] = la::dict_storage(b[e]);
    for (Py_ssize_t e = 0; e < n; ++e) {   // index -> pending bucket
        b[e] = la::dict_value(b[e], pending, h_pending);
        la::pf_dict(b[e]);
    }
    for (Py_ssize_t e = 0; e < n; ++e) b[e] = la::dict_storage(b[e]);
    // the tasks get an incref (first line); the head's `gated` slot is
    // read.  Its address is only prefetched, so the task's type, not yet
    // in cache, need not be checked.
    const Py_ssize_t g_off =
        a_task_gated.type != nullptr ? a_task_gated.off : -1;
    for (Py_ssize_t e = 0; e < n; ++e) {
        if (b[e] == nullptr) continue;
        Py_ssize_t pos = 0, cnt = 0;
        PyObject* t;
        while (cnt < la::kMaxTasks && PyDict_Next(b[e], &pos, nullptr, &t)) {
            la::pf(t);
            if (cnt == 0 && g_off >= 0)
                la::pf(reinterpret_cast<char*>(t) + g_off);
            ++cnt;
        }
    }
}

void la_finish_block(PyObject* by_job, Py_ssize_t pos, Py_ssize_t n,
                     PyObject* jobs, PyObject* pending, Py_hash_t h_pending,
                     PyObject* bound, Py_hash_t h_bound) {
    PyObject *key[la::kMaxBlock], *job[la::kMaxBlock], *d[la::kMaxBlock],
        *idx[la::kMaxBlock];
    Py_hash_t h[la::kMaxBlock];
    if (n > la::kMaxBlock) n = la::kMaxBlock;
    Py_ssize_t m = 0;
    PyObject *k, *ts;
    while (m < n && PyDict_Next(by_job, &pos, &k, &ts)) {
        key[m++] = k;
        la::pf_obj(k);                 // its cached hash
        la::pf_list(ts);               // its length
    }
    n = m;
    // the job table is large: index slot, entry, then the job itself
    const bool probe = PyDict_CheckExact(jobs);
    for (Py_ssize_t e = 0; e < n; ++e) {
        h[e] = probe ? la::str_hash(key[e]) : -1;
        if (h[e] != -1) la::dict_pf_index(jobs, h[e]);
    }
    for (Py_ssize_t e = 0; e < n; ++e)
        if (h[e] != -1) la::dict_pf_entry(jobs, h[e]);
    for (Py_ssize_t e = 0; e < n; ++e) {
        job[e] = h[e] != -1 ? la::dict_value(jobs, key[e], h[e]) : nullptr;
        la::pf_obj(job[e]);
    }
    la_dicts(job, n, d);
    for (Py_ssize_t e = 0; e < n; ++e) {   // `_alloc_vec` shares the storage
        idx[e] = a_job_idx.peek(job[e], d[e]);
        la::pf_dict(idx[e]);
        la::pf(a_job_occ.peek(job[e], d[e]));
    }
    for (Py_ssize_t e = 0; e < n; ++e) idx[e] = la::dict_storage(idx[e]);
    for (Py_ssize_t e = 0; e < n; ++e) {
        la::pf_dict(la::dict_value(idx[e], pending, h_pending));
        la::pf_dict(la::dict_value(idx[e], bound, h_bound));
    }
}

// Bundle entries [b0, b0 + n): their slots (one or two lines each).
void la_entries(PyObject* bundle, Py_ssize_t b0, Py_ssize_t n) {
    const Py_ssize_t size = PyList_GET_SIZE(bundle);
    if (b0 < 0 || b0 >= size) return;
    if (b0 + n > size) n = size - b0;
    for (Py_ssize_t e = 0; e < n; ++e)
        la::pf_span(PyList_GET_ITEM(bundle, b0 + e), 56, 2);
}

// The commits of entries [b0, b0 + n): entry -> job (-> key), job_key,
// tasks list -> items -> the task lines the walk writes; and for the
// pieces of the block, node -> name, _batches -> its tail.
void la_commit_block(PyObject* bundle, Py_ssize_t b0, Py_ssize_t n,
                     const vamd::SettleOut& so, size_t pp, PyObject* nodes,
                     const TaskStore& ts) {
    PyObject *be[la::kMaxBlock], *job[la::kMaxBlock], *tl[la::kMaxBlock],
        *d[la::kMaxBlock];
    const Py_ssize_t size = PyList_GET_SIZE(bundle);
    if (n > la::kMaxBlock) n = la::kMaxBlock;
    if (b0 < 0 || b0 >= size) return;
    if (b0 + n > size) n = size - b0;
    Py_ssize_t m = 0;
    for (Py_ssize_t b = b0; b < b0 + n; ++b) {
        if (so.outcome[b] != vamd::SETTLE_COMMITTED) continue;
        be[m] = PyList_GET_ITEM(bundle, b);
        la::pf_span(be[m], 56, 2);
        ++m;
    }
    // nodes of the block's pieces (a run on one node counts once)
    PyObject* nd[la::kMaxBlock];
    Py_ssize_t nn = 0;
    const Py_ssize_t n_nodes = PyList_GET_SIZE(nodes);
    int32_t last = -1;
    for (size_t p = pp; p < so.n_pieces && so.p_entry[p] < b0 + n &&
                        nn < la::kMaxBlock; ++p) {
        const int32_t nid = so.p_node[p];
        if (nid == last || nid < 0 || nid >= n_nodes) continue;
        last = nid;
        nd[nn] = PyList_GET_ITEM(nodes, nid);
        la::pf_obj(nd[nn]);
        ++nn;
    }
    bool slots = entry_type.type != nullptr;
    for (int i = 0; i < 5; ++i) slots = slots && entry_type.off[i] >= 0;
    for (Py_ssize_t e = 0; e < m; ++e) {
        job[e] = tl[e] = nullptr;
        if (!slots || Py_TYPE(be[e]) != entry_type.type) continue;
        char* base = reinterpret_cast<char*>(be[e]);
        la::pf(*reinterpret_cast<PyObject**>(base + entry_type.off[0]));
        tl[e] = *reinterpret_cast<PyObject**>(base + entry_type.off[1]);
        job[e] = *reinterpret_cast<PyObject**>(base + entry_type.off[4]);
        la::pf_list(tl[e]);
        la::pf_obj(job[e]);
    }
    for (Py_ssize_t e = 0; e < m; ++e) {
        tl[e] = la::list_items(tl[e]);
        d[e] = la::inst_dict(job[e]);
    }
    const bool tslots = ts.type && ts.off_node >= 0 && ts.off_status >= 0;
    for (Py_ssize_t e = 0; e < m; ++e) {
        d[e] = la::dict_storage(d[e]);
        if (tl[e] == nullptr) continue;
        Py_ssize_t k = PyList_GET_SIZE(tl[e]);
        if (k > la::kMaxTasks) k = la::kMaxTasks;
        for (Py_ssize_t i = 0; i < k; ++i) {
            char* t = reinterpret_cast<char*>(PyList_GET_ITEM(tl[e], i));
            la::pf(t);
            if (tslots) {              // addresses only, type unchecked
                la::pf(t + ts.off_node);
                la::pf(t + ts.off_status);
            }
        }
    }
    for (Py_ssize_t e = 0; e < m; ++e) la::pf(a_job_key.peek(job[e], d[e]));

    PyObject* bt[la::kMaxBlock];
    la_dicts(nd, nn, d);
    for (Py_ssize_t e = 0; e < nn; ++e) {
        la::pf(a_node_name.peek(nd[e], d[e]));
        bt[e] = a_node_batches.peek(nd[e], d[e]);
        la::pf_list(bt[e]);
    }
    for (Py_ssize_t e = 0; e < nn; ++e) la::pf_list_tail(bt[e]);
}

// The values of a pending bucket as a fresh list, or nullptr with *skip
// set when the job has nothing to plan (empty bucket, or a gated head).
PyObject* pending_tasks(PyObject* pend, bool* skip) {
    *skip = false;
    Ref tasks;
    if (PyDict_CheckExact(pend)) {
        const Py_ssize_t n = PyDict_GET_SIZE(pend);
        if (n == 0) { *skip = true; return nullptr; }
        tasks.reset(PyList_New(n));
        if (!tasks) return nullptr;
        Py_ssize_t pos = 0, at = 0;
        PyObject* t;
        while (at < n && PyDict_Next(pend, &pos, nullptr, &t)) {
            Py_INCREF(t);
            PyList_SET_ITEM(tasks.p, at++, t);
        }
        if (at != n) {
            PyErr_SetString(PyExc_RuntimeError, "pending bucket changed size");
            return nullptr;
        }
    } else {
        const int truth = PyObject_IsTrue(pend);
        if (truth < 0) return nullptr;
        if (!truth) { *skip = true; return nullptr; }
        Ref vals(PyObject_CallMethodObjArgs(pend, s_values, nullptr));
        if (!vals) return nullptr;
        tasks.reset(PySequence_List(vals.p));
        if (!tasks) return nullptr;
        if (PyList_GET_SIZE(tasks.p) == 0) { *skip = true; return nullptr; }
    }
    // see untrack_task_list: the list holds tasks only.  Done before the
    // gated read below, which may run Python code for a foreign task type.
    untrack_task_list(tasks.p);
    Ref first(PyList_GET_ITEM(tasks.p, 0));
    Py_INCREF(first.p);
    Ref gated(a_task_gated.get(first.p));
    if (!gated) return nullptr;
    const int g = PyObject_IsTrue(gated.p);
    if (g < 0) return nullptr;
    if (g) { *skip = true; return nullptr; }
    return tasks.release();
}

// The bundle entries of one fused run jobs_l[i:j] of the plan builder.
PyObject* bundle_entries(PyObject*, PyObject* args) {
    PyObject *jobs_l, *gm_l, *pending, *etype;
    Py_ssize_t i, j;
    if (!PyArg_ParseTuple(args, "O!nnO!OO!", &PyList_Type, &jobs_l, &i, &j,
                          &PyList_Type, &gm_l, &pending, &PyType_Type,
                          &etype))
        return nullptr;
    if (i < 0 || j < i || j > PyList_GET_SIZE(jobs_l) ||
        j > PyList_GET_SIZE(gm_l)) {
        PyErr_SetString(PyExc_IndexError, "run outside the worksheet");
        return nullptr;
    }
    entry_type.resolve(reinterpret_cast<PyTypeObject*>(etype));
    GcPause gc_pause;              // one entry and one list per job
    Ref entries(PyList_New(0));
    if (!entries) return nullptr;
    long long total = 0, mn = 1LL << 60;
    // short runs (the mixed workload makes thousands) go without
    const la::Config pfc = la::config();
    const bool ahead = pfc.on && j - i >= la::kMinWindow;
    const Py_hash_t h_pending = ahead ? la_key_hash(pending) : -1;
    for (Py_ssize_t k = i; k < j; ++k) {
        if (k >= PyList_GET_SIZE(jobs_l) || k >= PyList_GET_SIZE(gm_l)) {
            PyErr_SetString(PyExc_RuntimeError, "worksheet changed size");
            return nullptr;
        }
        if (ahead && (k - i) % pfc.block == 0) {
            const Py_ssize_t n = j - k < pfc.block ? j - k : pfc.block;
            la_bundle_block(jobs_l, k, n, pending, h_pending);
        }
        Ref jb(PyList_GET_ITEM(jobs_l, k));
        Py_INCREF(jb.p);
        Ref gm(PyList_GET_ITEM(gm_l, k));
        Py_INCREF(gm.p);
        Ref idx(a_job_idx.get(jb.p));
        if (!idx) return nullptr;
        Ref pend(map_get(idx.p, pending));
        if (!pend) {
            if (PyErr_Occurred()) return nullptr;
            continue;
        }
        if (pend.p == Py_None) continue;
        bool skip;
        Ref tasks(pending_tasks(pend.p, &skip));
        if (!tasks) {
            if (skip) continue;
            return nullptr;
        }
        const Py_ssize_t n = PyList_GET_SIZE(tasks.p);
        int64_t g;
        if (!as_i64(gm.p, &g)) return nullptr;
        Ref key(a_job_key.get(jb.p));
        if (!key) return nullptr;
        Ref nt(PyLong_FromSsize_t(n));
        if (!nt) return nullptr;
        Ref e(entry_type.make(key.p, tasks.p, nt.p, gm.p, jb.p));
        if (!e || PyList_Append(entries.p, e.p) != 0) return nullptr;
        total += n;
        if (g < mn) mn = g;
    }
    return Py_BuildValue("(OLL)", entries.p, total, mn);
}

// job.podgroup.status.phase = phase for every job with a pod group.
// Returns (changed, gated): the jobs whose phase was another value, and,
// when asked for, the jobs with a truthy `_gated` count.
PyObject* set_podgroup_phase(PyObject*, PyObject* args) {
    PyObject *jobs, *phase;
    int want_gated = 0;
    if (!PyArg_ParseTuple(args, "O!O|p", &PyList_Type, &jobs, &phase,
                          &want_gated))
        return nullptr;
    Ref changed(PyList_New(0)), gated(PyList_New(0));
    if (!changed || !gated) return nullptr;
    const la::Config pfc = la::config();
    const bool ahead = pfc.on && PyList_GET_SIZE(jobs) >= la::kMinWindow;
    for (Py_ssize_t k = 0; k < PyList_GET_SIZE(jobs); ++k) {
        if (ahead && k % pfc.block == 0)
            la_phase_block(jobs, k, pfc.block);
        Ref job(PyList_GET_ITEM(jobs, k));
        Py_INCREF(job.p);
        Ref pg(a_job_pg.get(job.p));
        if (!pg) return nullptr;
        if (pg.p != Py_None) {
            Ref st(a_pg_status.get(pg.p));
            if (!st) return nullptr;
            Ref cur(a_st_phase.get(st.p));
            if (!cur) return nullptr;
            const int ne = cur.p == phase
                ? 0 : PyObject_RichCompareBool(cur.p, phase, Py_NE);
            if (ne < 0) return nullptr;
            if (ne) {
                if (!a_st_phase.set(st.p, phase) ||
                    PyList_Append(changed.p, job.p) != 0)
                    return nullptr;
            }
        }
        if (want_gated) {
            PyObject* raw = nullptr;
            const int have = optional_attr(job.p, s_job_gated, &raw);
            if (have < 0) return nullptr;
            if (have) {
                Ref g(raw);
                const int truth = PyObject_IsTrue(g.p);
                if (truth < 0) return nullptr;
                if (truth && PyList_Append(gated.p, job.p) != 0)
                    return nullptr;
            }
        }
    }
    return Py_BuildValue("(OO)", changed.p, gated.p);
}

PyMethodDef methods[] = {
    {"scan_jobs", scan_jobs, METH_VARARGS,
     "scan_jobs(jobs, PENDING, FAILED, phase_map, ph_pending, ph_other, "
     "vers, occ, npend, nfailed, phase) -> dirty rows; fills the four "
     "columns"},
    {"bundle_entries", bundle_entries, METH_VARARGS,
     "bundle_entries(jobs_l, i, j, gm_l, PENDING, BundleEntry) -> "
     "(entries, total, min_gang)"},
    {"set_podgroup_phase", set_podgroup_phase, METH_VARARGS,
     "set_podgroup_phase(jobs, phase, want_gated=False) -> (changed, gated)"},
    {"finish_binds", finish_binds, METH_VARARGS,
     "finish_binds(by_job, jobs, pending, bound): JobInfo.finish_bind for "
     "every job of by_job found in jobs"},
    {"apply_walk", apply_walk, METH_VARARGS,
     "apply_walk(classes, jobs, alias, nodes, job_flag, class_job, "
     "log_nodes, log_counts, log_len, lost_mask, bound, want_fire) -> "
     "(rows, counts, classes, bind_by_job, committed, full_keys, events, "
     "(n_committed, n_gang_missed, n_lost, n_tail))"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef moddef = {PyModuleDef_HEAD_INIT, "_vamd_host",
                      "Host-native per-job loops of a scheduling cycle.", -1,
                      methods,
                      nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__vamd_host(void) {
    struct { PyObject** slot; const char* text; } names[] = {
        {&s_bundle, "bundle"}, {&s_log_off, "log_off"},
        {&s_job_key, "job_key"}, {&s_tclass, "tclass"}, {&s_tasks, "tasks"},
        {&s_ntasks, "ntasks"}, {&s_min_needed, "min_needed"},
        {&s_job, "job"}, {&s_key, "key"}, {&s_name, "name"},
        {&s_batches, "_batches"}, {&s_node_name, "node_name"},
        {&s_status, "status"}, {&s_f, "f"}, {&s_r, "r"},
        {&s_task_status_index, "task_status_index"}, {&s_occ, "_occ"},
        {&s_alloc_vec, "_alloc_vec"}, {&s_podgroup, "podgroup"},
        {&s_phase, "phase"}, {&s_tver, "_tver"}, {&s_gated, "gated"},
        {&s_job_gated, "_gated"}, {&s_values, "values"}};
    for (auto& nm : names) {
        *nm.slot = PyUnicode_InternFromString(nm.text);
        // the lookahead reads the cached hash of these names
        if (*nm.slot == nullptr || PyObject_Hash(*nm.slot) == -1)
            return nullptr;
    }
    PyObject* m = PyModule_Create(&moddef);
    if (m != nullptr &&
        PyModule_AddIntConstant(m, "PREFETCH_BLOCK", la::kDefaultBlock) != 0) {
        Py_DECREF(m);
        return nullptr;
    }
    return m;
}
