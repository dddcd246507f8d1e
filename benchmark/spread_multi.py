"""Cost of the multi-rule topology-spread select on the device.

Times ``spread_multi_select`` at N = 10k nodes for a class of 1,000 replicas
under the rule sets (N,), (3,), (3, N) and (3, 65, N) — hostname, zone, zone +
hostname, zone + rack + hostname, every maxSkew 1 — next to the existing
``spread_select`` on (N,) and (3,) in the same run.

    python benchmark/spread_multi.py

Needs a GPU.  Every launch is timed on its own between two events, after
its inputs are restored; 300 launches after 20 of warm-up; median and the
10th / 90th percentile in microseconds (this includes the launch).  Before
any timing the two kernels must agree on the single-rule logs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from benchmark.device_share import DEV, show, time_op
from volcano_amd.ops import hip


def main():
    hip._load()
    N, R, T = 10000, 4, 1000
    rng = np.random.RandomState(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    score0 = d(rng.uniform(0.0, 1.0, size=N).astype(np.float32))
    cap0 = d(rng.randint(1, 5, size=N).astype(np.int32))
    score, cap = score0.clone(), cap0.clone()
    req = d(np.ones(R, dtype=np.float32))
    used = torch.zeros((R, N), dtype=torch.float32, device=DEV)
    qa = torch.zeros(R, dtype=torch.float32, device=DEV)
    ql = torch.full((R,), 1.0e18, dtype=torch.float32, device=DEV)
    ln, lc = (torch.zeros(T, dtype=torch.int32, device=DEV) for _ in range(2))
    ll, placed, jp = (torch.zeros(1, dtype=torch.int32, device=DEV)
                      for _ in range(3))
    scratch = hip.spread_scratch(N, DEV)
    idx = np.arange(N, dtype=np.int32)
    maps = {3: d(idx % 3), 65: d(idx % 65), N: d(idx)}
    counts = {D: torch.zeros(D, dtype=torch.int32, device=DEV) for D in maps}

    def restore():
        score.copy_(score0)
        cap.copy_(cap0)
        used.zero_()
        qa.zero_()
        for c in counts.values():
            c.zero_()

    head = (score, cap, req, T, used, qa, ql, ln, lc, ll, placed, jp)

    def multi(ds):
        rules = [(maps[D], counts[D], 1) for D in ds]
        return lambda: hip.spread_multi_select(*head, rules, -1, scratch)

    def single(D):
        return lambda: hip.spread_select(*head, maps[D], counts[D], 1, -1,
                                         scratch)

    for D in (N, 3):
        logs = []
        for fn in (single(D), multi((D,))):
            restore()
            fn()
            torch.cuda.synchronize()
            assert int(placed) == T
            logs.append((ln.clone(), lc.clone(), int(ll)))
        assert logs[0][2] == logs[1][2] and torch.equal(logs[0][0], logs[1][0]) \
            and torch.equal(logs[0][1], logs[1][1]), "the two selects differ"

    for D in (N, 3):
        show(f"spread_select ({D},)", time_op(single(D), restore))
    for ds in ((N,), (3,), (3, N), (3, 65, N)):
        show(f"spread_multi_select {ds}", time_op(multi(ds), restore))
        assert int(placed) == T


if __name__ == "__main__":
    main()
