"""Cost of scoring ScheduleAnyway topology spread per placement on the device.

Times ``spread_soft_select`` at N = 10k nodes for a class of 1,000 replicas
under the rule sets (S3), (S7168) — the largest soft table — and (H3, S7168),
static and re-scoring, next to its neighbours on the same class with the soft
rule made hard (maxSkew 1): ``spread_multi_select`` for the static run,
``spread_rescore_select`` for the re-scoring one.

    python benchmark/spread_soft.py

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
from volcano_amd.ops.reference import (SPREAD_SOFT_LDS_DOMAINS as S,
                                       SPREAD_SOFT_SKEW)


def main():
    hip._load()
    N, R, W, T, TW = 10000, 4, 1, 1000, 0.02
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
    maps = {3: d(idx % 3), S: d(idx % S)}
    counts = {D: torch.zeros(D, dtype=torch.int32, device=DEV) for D in maps}

    def restore():
        score.copy_(score0)
        cap.copy_(cap0)
        used.copy_(used0)
        qa.zero_()
        for c in counts.values():
            c.zero_()

    tail = (ln, lc, ll, placed, jp)
    hip.score_cap(alloc, used0, extra, ready, taints, planes, req, 0, zero_w,
                  zero_w, 1.0, 0.0, 0.0, dim_w, None, score0, cap0)

    def per_instance(label, fn):
        m = time_op(fn, restore)
        assert int(placed) == T
        show(label, m)
        print(f"{'':34s} {m[0] / T:7.3f} us per placed instance")
        return m[0]

    for ds in (("S3",), (f"S{S}",), ("H3", f"S{S}")):
        soft = [(maps[int(x[1:])], counts[int(x[1:])],
                 SPREAD_SOFT_SKEW if x[0] == "S" else 1,
                 TW if x[0] == "S" else 0.0) for x in ds]
        hard = [(dom, cnt, 1) for dom, cnt, _, _ in soft]
        for rescore in (False, True):
            mine = per_instance(
                f"spread_soft_select {ds} rescore={int(rescore)}",
                lambda: hip.spread_soft_select(
                    alloc, used, extra, req, 1.0, 0.0, 0.0, dim_w, None,
                    score, cap, T, qa, ql, *tail, soft, rescore, -1, scratch))
            if rescore:
                other = per_instance(
                    f"spread_rescore_select {ds} hard",
                    lambda: hip.spread_rescore_select(
                        alloc, used, extra, req, 1.0, 0.0, 0.0, dim_w, None,
                        score, cap, T, qa, ql, *tail, hard, -1, scratch))
            else:
                other = per_instance(
                    f"spread_multi_select {ds} hard",
                    lambda: hip.spread_multi_select(
                        score, cap, req, T, used, qa, ql, *tail, hard, -1,
                        scratch))
            print(f"{'':34s} {mine / other:7.3f} x the hard neighbour")


if __name__ == "__main__":
    main()
