"""Cost of per-card packing on the device.

Times ``device_cap`` and ``device_commit`` with HIP events at N = 10k nodes
of K = 8 cards, for a class of 1,000 instances (a log of 1,000 entries, one
pod each), next to ``score_cap`` on the same node arrays in the same run.

    python benchmark/device_share.py

Needs a GPU.  Every launch is timed on its own between two events, after
its inputs are restored; 300 launches after 20 of warm-up; median and the
10th / 90th percentile in microseconds (this includes the launch)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from volcano_amd.ops import hip

DEV = "cuda"
ITERS = 300


def time_op(fn, restore):
    times = []
    for it in range(ITERS + 20):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= 20:
            times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return statistics.median(times), times[len(times) // 10], \
        times[-len(times) // 10]


def show(label, m):
    print(f"{label:34s} median {m[0]:7.1f} us  [p10 {m[1]:.1f} - p90 {m[2]:.1f}]")


def main():
    hip._load()
    N, K, R, W, L = 10000, 8, 4, 1, 1000
    rng = np.random.RandomState(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # 288 GiB cards in MiB, half of them partly used
    total = np.full(N, 288 * 1024, dtype=np.int32)
    mem0 = d((rng.randint(0, 3, size=(K, N)) * 65536).astype(np.int32))
    cores0 = d((rng.randint(0, 3, size=(K, N)) * 25).astype(np.int32))
    state0 = d(rng.randint(0, 3, size=(K, N)).astype(np.int32))
    planes = [mem0.clone(), cores0.clone(), state0.clone(), d(total)]
    request = (1, 160 * 1024, 25)

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
        for p, p0 in zip(planes, (mem0, cores0, state0)):
            p.copy_(p0)

    show("device_cap", time_op(
        lambda: hip.device_cap(score, cap, *planes, request), restore))

    restore()
    hip.device_cap(score, cap, *planes, request)
    nodes = torch.nonzero(cap > 0).flatten()[:L].to(torch.int32)
    assert nodes.shape[0] == L
    counts = torch.ones(L, dtype=torch.int32, device=DEV)
    length = d(np.array([L], dtype=np.int32))
    assign = torch.zeros((L, K), dtype=torch.int32, device=DEV)
    show("device_commit, 1000 entries", time_op(
        lambda: hip.device_commit(nodes, counts, length, *planes, assign,
                                  request), restore))
    flag = torch.zeros(1, dtype=torch.uint8, device=DEV)
    show("device_revert, 1000 entries", time_op(
        lambda: hip.device_revert(flag, nodes, length, *planes, assign,
                                  request),
        lambda: (restore(), hip.device_commit(
            nodes, counts, length, *planes, assign, request))))
    torch.cuda.synchronize()
    # the last revert gave everything back
    assert all(torch.equal(p, p0)
               for p, p0 in zip(planes, (mem0, cores0, state0)))


if __name__ == "__main__":
    main()
