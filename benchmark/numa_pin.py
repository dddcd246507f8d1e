"""Cost of NUMA pinning on the device.

Times ``numa_cap``, ``numa_commit`` and ``numa_revert`` with HIP events at
N = 10k nodes of Z = 8 zones, for a class of 1,000 instances (a log of 1,000
entries, one pod each), next to ``score_cap`` on the same node arrays in the
same run.

    python benchmark/numa_pin.py

Needs a GPU.  Every launch is timed on its own between two events, after
its inputs are restored; 300 launches after 20 of warm-up; median and the
10th / 90th percentile in microseconds (this includes the launch)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from benchmark.device_share import DEV, show, time_op
from volcano_amd.ops import hip


def main():
    hip._load()
    N, Z, R, W, L = 10000, 8, 4, 1, 1000
    rng = np.random.RandomState(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # 16-core zones in millicores, each with 0..15 cores taken
    free0 = d(((16 - rng.randint(0, 16, size=(Z, N))) * 1000).astype(np.int32))
    free = free0.clone()
    cpu = 2500

    alloc = d(np.full((R, N), 64.0, dtype=np.float32))
    used = d(rng.randint(0, 32, size=(R, N)).astype(np.float32))
    extra = torch.zeros_like(used)
    ready = torch.ones(N, dtype=torch.uint8, device=DEV)
    taints = torch.zeros(N, dtype=torch.int64, device=DEV)
    lplanes = torch.zeros((W, N), dtype=torch.int64, device=DEV)
    req = d(np.ones(R, dtype=np.float32))
    zero_w = torch.zeros(W, dtype=torch.int64, device=DEV)
    dim_w = torch.ones(R, dtype=torch.float32, device=DEV)
    score = torch.empty(N, dtype=torch.float32, device=DEV)
    cap = torch.empty(N, dtype=torch.int32, device=DEV)

    def score_cap():
        hip.score_cap(alloc, used, extra, ready, taints, lplanes, req, -1,
                      zero_w, zero_w, 1.0, 0.0, 0.0, dim_w, None, score, cap)

    show("score_cap", time_op(score_cap, lambda: None))
    score_cap()
    score0, cap0 = score.clone(), cap.clone()

    def restore():
        score.copy_(score0)
        cap.copy_(cap0)
        free.copy_(free0)

    show("numa_cap", time_op(lambda: hip.numa_cap(score, cap, free, cpu),
                             restore))

    restore()
    hip.numa_cap(score, cap, free, cpu)
    nodes = torch.nonzero(cap > 0).flatten()[:L].to(torch.int32)
    assert nodes.shape[0] == L
    counts = torch.ones(L, dtype=torch.int32, device=DEV)
    length = d(np.array([L], dtype=np.int32))
    assign = torch.zeros((L, Z), dtype=torch.int32, device=DEV)
    show("numa_commit, 1000 entries", time_op(
        lambda: hip.numa_commit(nodes, counts, length, free, assign, cpu),
        restore))
    flag = torch.zeros(1, dtype=torch.uint8, device=DEV)
    show("numa_revert, 1000 entries", time_op(
        lambda: hip.numa_revert(flag, nodes, length, free, assign, cpu),
        lambda: (restore(), hip.numa_commit(nodes, counts, length, free,
                                            assign, cpu))))
    torch.cuda.synchronize()
    # the last revert gave everything back
    assert torch.equal(free, free0) and not assign.any()


if __name__ == "__main__":
    main()
