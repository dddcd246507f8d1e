"""Cost of the re-scoring select (nodeorder ``exact: true``) on the device.

Times ``rescore_select`` at N = 10k nodes for a class of 1,000 instances
under ``w_least = 1`` (about one block reduce per instance), ``w_most = 1``
(the run-length regime: one reduce per node) and ``w_bal = 1``, next to the
static ``select_commit`` of the same class, serial and sort-based, in the
same run.

    python benchmark/rescore.py

Needs a GPU.  Every launch is timed on its own between two events, after
its inputs are restored; 300 launches after 20 of warm-up; median and the
10th / 90th percentile in microseconds (this includes the launch), and the
median per placed instance.  Before any timing the ``w_most`` class must log
what the static select logs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from benchmark.device_share import DEV, show, time_op
from volcano_amd.ops import hip

N, R, W, T = 10000, 4, 1, 1000
WEIGHTS = {"w_least=1": (1.0, 0.0, 0.0), "w_most=1": (0.0, 1.0, 0.0),
           "w_bal=1": (0.0, 0.0, 1.0)}


def setup():
    """-> (ops, select, restore, outputs): ``ops[weights][kind]()`` launches
    one select of that class (kind: rescore, serial or sorted) and
    ``select(weights)`` names the class whose scores ``restore`` puts back."""
    rng = np.random.RandomState(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    alloc = d(np.full((R, N), 64.0, dtype=np.float32))
    used0 = d(rng.randint(0, 32, size=(R, N)).astype(np.float32))
    used, extra = used0.clone(), torch.zeros_like(used0)
    ready = torch.ones(N, dtype=torch.uint8, device=DEV)
    taints = torch.zeros(N, dtype=torch.int64, device=DEV)
    planes = torch.zeros((W, N), dtype=torch.int64, device=DEV)
    zw = torch.zeros(W, dtype=torch.int64, device=DEV)
    req = d(np.ones(R, dtype=np.float32))
    dim_w = d(np.ones(R, dtype=np.float32))
    score = torch.empty(N, dtype=torch.float32, device=DEV)
    cap = torch.empty(N, dtype=torch.int32, device=DEV)
    qa = torch.zeros(R, dtype=torch.float32, device=DEV)
    ql = torch.full((R,), 1.0e18, dtype=torch.float32, device=DEV)
    ln, lc = (torch.zeros(T, dtype=torch.int32, device=DEV) for _ in range(2))
    ll, placed, jp = (torch.zeros(1, dtype=torch.int32, device=DEV)
                      for _ in range(3))
    slot = torch.empty(N, dtype=torch.int32, device=DEV)
    sort_scratch = torch.empty(4 * N, dtype=torch.int32, device=DEV)
    scores = {}
    for name, (wl, wm, wb) in WEIGHTS.items():
        hip.score_cap(alloc, used0, extra, ready, taints, planes, req, 0, zw,
                      zw, wl, wm, wb, dim_w, None, score, cap)
        scores[name] = score.clone()
    current = [None]

    def restore():
        score.copy_(scores[current[0]])
        used.copy_(used0)
        qa.zero_()

    tail = (qa, ql, ln, lc, ll, placed, jp, -1)

    def op(name, kind):
        wl, wm, wb = WEIGHTS[name]

        def run():
            if kind == "rescore":
                hip.rescore_select(alloc, used, extra, ready, taints, planes,
                                   req, 0, zw, zw, wl, wm, wb, dim_w, None,
                                   score, cap, T, *tail, slot)
            else:
                hip.select_commit(score, cap, req, T, used, *tail,
                                  sort_scratch if kind == "sorted" else None)
        return run

    def select(name):
        current[0] = name

    ops = {name: {kind: op(name, kind)
                  for kind in ("rescore", "serial", "sorted")}
           for name in WEIGHTS}
    return ops, select, restore, (ln, lc, ll, placed)


def main():
    hip._load()
    ops, select, restore, (ln, lc, ll, placed) = setup()

    select("w_most=1")
    logs = []
    for kind in ("serial", "rescore"):
        restore()
        ops["w_most=1"][kind]()
        torch.cuda.synchronize()
        assert int(placed) == T
        logs.append((ln.clone(), lc.clone(), int(ll)))
    assert logs[0][2] == logs[1][2] and torch.equal(logs[0][0], logs[1][0]) \
        and torch.equal(logs[0][1], logs[1][1]), "the two selects differ"

    for name in ops:
        select(name)
        for kind in ("rescore", "serial", "sorted"):
            m = time_op(ops[name][kind], restore)
            assert int(placed) == T
            show(f"{kind} {name} ({int(ll)} nodes)", m)
            print(f"{'':34s} {m[0] / T:7.3f} us per placed instance")


if __name__ == "__main__":
    main()
