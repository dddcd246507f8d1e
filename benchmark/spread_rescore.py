"""Cost of re-scoring per placement under topology spread on the device.

Times ``spread_rescore_select`` at N = 10k nodes for a class of 1,000 replicas
under the rule sets (N,), (3,), (3, N) and (3, 65, N) — hostname, zone, zone +
hostname, zone + rack + hostname, every maxSkew 1 — with ``w_least = 1`` and
with ``w_most = 1``, next to the static select of the same class in the same
run: ``spread_select`` for one rule, ``spread_multi_select`` for several.

    python benchmark/spread_rescore.py

Needs a GPU.  Every launch is timed on its own between two events, after
its inputs are restored; 300 launches after 20 of warm-up; median and the
10th / 90th percentile in microseconds (this includes the launch), and the
median per placed instance."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from benchmark.device_share import DEV, show, time_op
from volcano_amd.ops import hip


def main(static=True):
    """``static``: also time the static select of every class."""
    hip._load()
    N, R, W, T = 10000, 4, 1, 1000
    rng = np.random.RandomState(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    alloc = d(np.full((R, N), 64.0, dtype=np.float32))
    used0 = d(rng.randint(0, 32, size=(R, N)).astype(np.float32))
    used = used0.clone()
    extra = torch.zeros_like(used)
    ready = torch.ones(N, dtype=torch.uint8, device=DEV)
    taints = torch.zeros(N, dtype=torch.int64, device=DEV)
    planes = torch.zeros((W, N), dtype=torch.int64, device=DEV)
    zero_w = torch.zeros(W, dtype=torch.int64, device=DEV)
    req = d(np.ones(R, dtype=np.float32))
    dim_w = torch.ones(R, dtype=torch.float32, device=DEV)
    score0 = torch.empty(N, dtype=torch.float32, device=DEV)
    cap0 = torch.empty(N, dtype=torch.int32, device=DEV)
    score, cap = score0.clone(), cap0.clone()
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
        used.copy_(used0)
        qa.zero_()
        for c in counts.values():
            c.zero_()

    tail = (ln, lc, ll, placed, jp)

    def per_instance(label, fn):
        m = time_op(fn, restore)
        assert int(placed) == T
        show(label, m)
        print(f"{'':34s} {m[0] / T:7.3f} us per placed instance")

    for w_least, w_most in ((1.0, 0.0), (0.0, 1.0)):
        hip.score_cap(alloc, used0, extra, ready, taints, planes, req, 0,
                      zero_w, zero_w, w_least, w_most, 0.0, dim_w, None,
                      score0, cap0)
        print(f"w_least = {w_least:g}, w_most = {w_most:g}")
        for ds in ((N,), (3,), (3, N), (3, 65, N)):
            rules = [(maps[D], counts[D], 1) for D in ds]
            per_instance(
                f"spread_rescore_select {ds}",
                lambda: hip.spread_rescore_select(
                    alloc, used, extra, req, w_least, w_most, 0.0, dim_w,
                    None, score, cap, T, qa, ql, *tail, rules, -1, scratch))
            if not static:
                continue
            if len(ds) == 1:
                per_instance(
                    f"spread_select {ds}",
                    lambda: hip.spread_select(score, cap, req, T, used, qa,
                                              ql, *tail, *rules[0], -1,
                                              scratch))
            else:
                per_instance(
                    f"spread_multi_select {ds}",
                    lambda: hip.spread_multi_select(score, cap, req, T, used,
                                                    qa, ql, *tail, rules, -1,
                                                    scratch))


if __name__ == "__main__":
    main()
