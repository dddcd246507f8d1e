// Stand-alone check of lookahead.h against the interpreter's own lookups.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <cstdio>
#include "lookahead.h"
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }
namespace la = vamd::la;
static long checked = 0;
static int check_dict(PyObject* d) {
    Py_ssize_t pos = 0; PyObject *k, *v;
    la::dict_storage(d);
    while (PyDict_Next(d, &pos, &k, &v)) {
        Py_hash_t h = PyObject_Hash(k);
        la::dict_pf_index(d, h); la::dict_pf_entry(d, h);
        PyObject* got = la::dict_value(d, k, h);
        if (got != v) { std::printf("MISMATCH size=%zd\n", PyDict_GET_SIZE(d)); return 1; }
        ++checked;
    }
    PyObject* absent = PyUnicode_FromString("definitely-absent-key");
    if (la::dict_value(d, absent, PyObject_Hash(absent)) != nullptr) { std::printf("FOUND ABSENT\n"); return 1; }
    Py_DECREF(absent);
    return 0;
}
int main() {
    Py_Initialize();
    int bad = 0;
    const char* code =
        "class J:\n"
        "    def __init__(s, i):\n"
        "        s.key = 'k%d' % i; s.podgroup = None; s.idx = {}; s._occ = i\n"
        "class S:\n"
        "    __slots__ = ('a', 'b')\n"
        "    def __init__(s): s.a = 1; s.b = 2\n"
        "import enum\n"
        "class E(enum.IntEnum):\n"
        "    P = 1; B = 2; F = 3\n"
        "objs = [J(i) for i in range(50)]\n"
        "objs[7].extra = 1\n"              // leaves the shared keys
        "del objs[9].podgroup\n"
        "dicts = [{}, {'a': 1}, {E.P: {}, E.B: {'x': 1}}, {1: 2, (1, 2): 3, 'z': 4}]\n"
        "for n in (5, 6, 10, 11, 85, 86, 170, 171, 300, 40000, 70000):\n"
        "    d = {'key-%d' % i: i for i in range(n)}\n"
        "    dicts.append(d)\n"
        "    e = dict(d)\n"
        "    for i in range(0, n, 3): del e['key-%d' % i]\n"   // dummies
        "    dicts.append(e)\n"
        "slotted = S()\n"
        "lists = [[], [1], list(range(100))]\n";
    PyObject* g = PyDict_New();
    PyDict_SetItemString(g, "__builtins__", PyEval_GetBuiltins());
    PyObject* r = PyRun_String(code, Py_file_input, g, g);
    if (!r) { PyErr_Print(); return 2; }
    PyObject* dicts = PyDict_GetItemString(g, "dicts");
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(dicts); ++i) bad |= check_dict(PyList_GET_ITEM(dicts, i));
    PyObject* objs = PyDict_GetItemString(g, "objs");
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(objs); ++i) {
        PyObject* o = PyList_GET_ITEM(objs, i);
        la::pf_obj(o);
        PyObject* d = la::inst_dict(o);
        PyObject* real = PyObject_GenericGetDict(o, nullptr);
        if (d != real) { std::printf("inst_dict mismatch\n"); bad = 1; }
        Py_XDECREF(real);
        if (la::dict_storage(d) != d) { std::printf("storage\n"); bad = 1; }
        bad |= check_dict(d);
    }
    PyObject* s = PyDict_GetItemString(g, "slotted");
    if (la::inst_dict(s) != nullptr) { std::printf("slotted has dict\n"); bad = 1; }
    if (la::inst_dict(Py_None) != nullptr) { std::printf("None has dict\n"); bad = 1; }
    if (la::dict_storage(Py_None) != nullptr || la::dict_value(Py_None, s, 5) != nullptr) bad = 1;
    PyObject* lists = PyDict_GetItemString(g, "lists");
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(lists); ++i) {
        PyObject* l = PyList_GET_ITEM(lists, i);
        if (la::list_items(l) != l) bad = 1;
        la::pf_list_tail(l);
    }
    if (la::list_items(Py_None) != nullptr) bad = 1;
    std::printf("%s: %ld lookups checked\n", bad ? "FAILED" : "lookahead OK", checked);
    Py_DECREF(g);
    return bad;
}
