#!/usr/bin/env python3
"""Flagship benchmark: pods scheduled per second through the MI355X
decision plane on the BASELINE synthetic inventory (10k nodes / 100k pods
in 10k gang jobs — BASELINE.json config #3 shape; the reference's headline
is ≈40-55 pods/s for 10k pods on a KWOK cluster).

One *step* = scheduling the full inventory from empty: reset cluster state
(all pods pending, nodes idle — inside the timed region, as pod intake is
part of the reference's measurement too) + one full scheduler cycle
(snapshot → tensor pack → enqueue → allocate plan → HIP kernel cycle →
readback → bind).  All placement decisions for all 100k pods happen in
that cycle.

Multi-GPU (--gpus N, launched by torch.distributed.run): nodes and jobs
are hard-sharded round-robin across ranks (the reference's NodeShard
hard-sharding mode) — each rank schedules its jobs on
its nodes, no cross-rank conflicts by construction; ranks sync per step
and the reported value is the whole-job aggregate.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch

from volcano_amd.api.info import JobInfo, NodeInfo, QueueInfo, TaskInfo
from volcano_amd.api.resource import CPU, MEMORY, PODS, Resource
from volcano_amd.api.types import PodGroupPhase, TaskStatus
from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                   default_config)
from volcano_amd.utils import synth

GI = 1024 ** 3

# --dump-outputs budget: every array of a run together stays under this
DUMP_BYTES_MAX = 64 * 1000 * 1000


def stamp_creation(pg, seq: int) -> None:
    """Fixed creation time per job sequence number: job order ties break
    on it, so the inventory is identical from run to run instead of
    carrying the wall clock of the moment it was built."""
    pg.meta.creation_timestamp = 1.0e9 + seq * 1.0e-3


def build_cluster(cache: SchedulerCache, n_nodes: int, n_jobs: int,
                  pods_per_job: int, rank: int, world: int,
                  node_rank: int = None, node_world: int = None,
                  mix: bool = False):
    """Synthetic inventory: jobs sharded round-robin by rank; nodes by
    (node_rank, node_world) — full replication in soft mode.

    ``mix``: heterogeneous inventory (varied gang sizes/requests/
    priorities across 4 weighted queues, zoned nodes) — defeats the
    uniform-gang fast paths on purpose."""
    import random
    rng = random.Random(12345)
    node_rank = rank if node_rank is None else node_rank
    node_world = world if node_world is None else node_world
    for i in range(node_rank, n_nodes, node_world):
        labels = {"zone": f"z{i % 4}"} if mix else None
        node = synth.make_node(f"node-{i:06d}", cpu_milli=32000,
                               mem=256 * GI, pods=256, labels=labels)
        cache.add_node_info(NodeInfo(node))
    queues = ["default"] if not mix else ["default", "batch", "svc", "ml"]
    for qn in queues:
        cache.add_queue_info(QueueInfo(synth.make_queue(
            qn, weight=1 if qn == "default" else rng.randint(1, 4))))
    jobs = []
    for j in range(rank, n_jobs, world):
        name = f"job-{j:06d}"
        if mix:
            size = rng.choice([1, 2, 4, 8, 16])
            cpu = float(rng.choice([250, 500, 1000, 2000, 4000]))
            mem = float(rng.choice([1, 2, 4])) * GI
            queue = rng.choice(queues)
            prio = rng.randint(0, 10)
            selector = {"zone": f"z{rng.randrange(4)}"} \
                if rng.random() < 0.2 else None
        else:
            size, cpu, mem = pods_per_job, 1000.0, float(GI)
            queue, prio, selector = "default", 0, None
        pg = synth.make_podgroup(name, queue=queue, min_member=size,
                                 min_resources={CPU: cpu * size,
                                                MEMORY: mem * size})
        stamp_creation(pg, j)
        job = JobInfo(f"default/{name}", pg)
        for p in range(size):
            pod = synth.make_pod(f"{name}-w-{p}", name, queue=queue,
                                 cpu_milli=cpu, mem=mem, role="worker",
                                 priority=prio, node_selector=selector)
            job.add_task(TaskInfo.from_pod(pod, job.key))
        cache.add_job_info(job)
        jobs.append(job)
    return jobs


def reset_cluster(cache: SchedulerCache, jobs):
    """All pods pending again, all nodes idle (start-of-step state)."""
    for job in jobs:
        if job.podgroup is not None:
            job.podgroup.status.phase = PodGroupPhase.PENDING.value
        for t in job.tasks.values():
            t.status = TaskStatus.PENDING
            t.node_name = ""
        job.task_status_index = {TaskStatus.PENDING: dict(job.tasks)}
        job._occ = 0                       # counter matches the fresh index
        job._alloc_vec = None
    cache.reset_usage()
    if isinstance(cache.binder, FakeBinder):
        cache.binder.clear()


def dump_outputs(cache: SchedulerCache, out_dir: str, rank: int) -> None:
    """Write what the last timed step decided as ``<name>.npy`` (float64).

    ``pod_node``: one entry per pod, jobs and their pods in key order —
    the index (in node-name order) of the node the pod was bound to, -1
    for a pod left unbound.  ``node_pod_count``: pods bound per node, same
    node order.  Ranks other than 0 add ``_rank<r>`` to the name.  Past
    the byte budget a fixed seeded sample of the entries is kept."""
    import numpy as np
    node_idx = {name: i for i, name in enumerate(sorted(cache.nodes))}
    pod_node = []
    for jkey in sorted(cache.jobs):
        tasks = cache.jobs[jkey].tasks
        for tkey in sorted(tasks):
            t = tasks[tkey]
            bound = t.status == TaskStatus.BOUND and t.node_name
            pod_node.append(node_idx.get(t.node_name, -1) if bound else -1)
    pod_node = np.asarray(pod_node, dtype=np.float64)
    placed = pod_node[pod_node >= 0].astype(np.int64)
    arrays = {
        "pod_node": pod_node,
        "node_pod_count": np.bincount(
            placed, minlength=len(node_idx)).astype(np.float64),
    }
    budget = DUMP_BYTES_MAX // len(arrays) // 8      # entries per array
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if rank == 0 else f"_rank{rank}"
    for name, arr in arrays.items():
        if arr.size > budget:
            keep = np.random.default_rng(20240607).choice(
                arr.size, size=budget, replace=False)
            arr = arr[np.sort(keep)]
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--jobs", type=int, default=10000)
    ap.add_argument("--pods-per-job", type=int, default=10)
    ap.add_argument("--cpu", action="store_true",
                    help="force the CPU torch-oracle path (no GPU)")
    ap.add_argument("--timing", action="store_true",
                    help="print per-phase timing summaries to stderr")
    ap.add_argument("--shard-mode", choices=["hard", "soft"], default="hard",
                    help="hard: nodes+jobs sharded (conflict-free); "
                         "soft: nodes replicated, delta all-reduce")
    ap.add_argument("--extra-actions", default="",
                    help="comma list appended to the action pipeline "
                         "(e.g. preempt,reclaim — BASELINE config 4)")
    ap.add_argument("--extra-plugins", default="",
                    help="comma list of extra plugins for the last tier "
                         "(e.g. task-topology,numaaware — BASELINE config 5)")
    ap.add_argument("--mix", action="store_true",
                    help="heterogeneous inventory (varied gangs/queues/"
                         "priorities/selectors)")
    ap.add_argument("--churn", action="store_true",
                    help="sustained arrivals/completions at steady load; "
                         "reports pods/s plus true p99 pod latency "
                         "(creation->bind) — the reference's measurement "
                         "methodology (audit-exporter "
                         "pod_scheduling_latency_seconds)")
    ap.add_argument("--churn-gangs", type=int, default=200,
                    help="new gangs per churn cycle")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's "
                         "placement decisions to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: today the "
                         "per-phase timing summary of --timing (other "
                         "shapes and modes have flags of their own)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank =int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = world > 1
    use_gpu = torch.cuda.is_available() and not args.cpu
    if dist:
        backend = os.environ.get("VAMD_DIST_BACKEND") or \
            ("nccl" if use_gpu else "gloo")
        local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
        if use_gpu:
            # modulo: lets N ranks share fewer GPUs (rehearsal on 1 GPU)
            dev_idx = local_rank % torch.cuda.device_count()
            torch.cuda.set_device(dev_idx)
        if use_gpu and backend == "nccl":
            # pin the communicator device: barrier() otherwise guesses
            # cuda:<global rank>, which breaks when ranks share GPUs
            torch.distributed.init_process_group(
                backend=backend, device_id=torch.device("cuda", dev_idx))
        else:
            torch.distributed.init_process_group(backend=backend)
    elif use_gpu:
        torch.cuda.set_device(0)

    device = "cuda" if use_gpu else "cpu"
    config = default_config()
    if args.extra_plugins:
        from volcano_amd.scheduler.config import PluginOption
        for name in args.extra_plugins.split(","):
            if name.strip():
                config.tiers[-1].plugins.append(PluginOption(name.strip()))
    if args.extra_actions:
        for name in args.extra_actions.split(","):
            if name.strip() and name.strip() not in config.actions:
                config.actions.append(name.strip())
    config.use_hip = use_gpu
    config.device = device
    if use_gpu:
        # fail loudly if the HIP library is missing — no silent eager path
        from volcano_amd.ops import hip as vamd_hip
        vamd_hip._load()

    cache = SchedulerCache(store=None, binder=FakeBinder(), device=device)
    sched = Scheduler(cache, config)
    coord = None
    if dist and args.shard_mode == "soft":
        from volcano_amd.parallel.softshard import SoftShardCoordinator
        from volcano_amd.scheduler.actions.allocate import AllocateAction
        coord = SoftShardCoordinator(rank, world)
        for a in sched._actions:
            if isinstance(a, AllocateAction):
                a.coordinator = coord
    node_world = 1 if (dist and args.shard_mode == "soft") else world
    node_rank = 0 if (dist and args.shard_mode == "soft") else rank
    jobs = build_cluster(cache, args.nodes,
                         0 if args.churn else args.jobs, args.pods_per_job,
                         rank, world, node_rank, node_world, mix=args.mix)
    if args.mix:
        my_pods = sum(len(j.tasks) for j in jobs)
        if dist:
            tp = torch.tensor([float(my_pods)])
            torch.distributed.all_reduce(tp)
            total_pods = int(tp.item())
        else:
            total_pods = my_pods
    else:
        total_pods = args.jobs * args.pods_per_job   # whole-job, all ranks

    soft = dist and args.shard_mode == "soft"

    # -- churn mode: steady-state arrivals + completions -------------------
    # (reference methodology: sustained pods/s + per-pod creation->bind
    # latency, third_party/kube-apiserver-audit-exporter metrics.go:31)
    churn_state = {"i": 0, "latencies": [], "seen": set()}

    def churn_step() -> int:
        import random
        rng = random.Random(1000 + churn_state["i"])
        now0 = time.perf_counter()
        new_jobs = []
        for _ in range(args.churn_gangs):
            churn_state["i"] += 1
            j = churn_state["i"]
            name = f"churn-{rank}-{j:06d}"
            pg = synth.make_podgroup(name, min_member=args.pods_per_job)
            stamp_creation(pg, j)
            job = JobInfo(f"default/{name}", pg)
            for p in range(args.pods_per_job):
                pod = synth.make_pod(f"{name}-w-{p}", name, cpu_milli=1000.0,
                                     mem=float(GI), role="worker")
                job.add_task(TaskInfo.from_pod(pod, job.key))
            job._ctime = now0
            cache.add_job_info(job)
            new_jobs.append(job)
        before = cache.binder.bound_count
        sched.run_once()
        now1 = time.perf_counter()
        bound_now = cache.binder.bound_count - before
        # latency: every task bound THIS cycle was created at its job's
        # _ctime (fresh jobs) or an earlier cycle's stamp
        lats = churn_state["latencies"]
        for key, job in list(cache.jobs.items()):
            if not key.startswith("default/churn-"):
                continue
            if job.occupied_count and key not in churn_state["seen"]:
                churn_state["seen"].add(key)
                ct = getattr(job, "_ctime", now1)
                lats.append(now1 - ct)
        # completions: retire ~half of the bound churn jobs to hold the
        # cluster at steady utilization
        bound_jobs = [j for k, j in cache.jobs.items()
                      if k.startswith("default/churn-") and j.is_ready()]
        for job in bound_jobs[: len(bound_jobs) // 2]:
            for t in job.tasks.values():
                ni = cache.nodes.get(t.node_name)
                if ni is not None:
                    ni.remove_task(t)
            cache.jobs.pop(job.key, None)
            churn_state["seen"].discard(job.key)
            cache.jobs_epoch += 1
        cache._used_dirty = True
        return bound_now

    def step() -> int:
        if args.churn:
            return churn_step()
        reset_cluster(cache, jobs)
        sched.run_once()
        if soft:
            # soft mode: conflict losers retry next cycle — a step is
            # schedule-to-completion (convergence cost measured honestly)
            my_pods = len(jobs) * args.pods_per_job
            for _ in range(world + 3):
                if cache.binder.bound_count >= my_pods:
                    break
                sched.run_once()
        return cache.binder.bound_count

    def sync():
        if use_gpu:
            torch.cuda.synchronize()
        if dist:
            torch.distributed.barrier()

    # the inventory objects are permanent for the run — freeze them out
    # of the cyclic GC's generational scans (a gen-2 pass over millions
    # of TaskInfo/Pod objects otherwise lands mid-step as a ~400 ms spike)
    import gc
    gc.collect()
    gc.freeze()
    if os.environ.get("VAMD_GC_DISABLE"):
        gc.disable()

    for _ in range(args.warmup):
        n = step()
    sync()
    churn_state["latencies"].clear()   # p99 over the measured window only

    # Freeze the long-lived inventory graph (nodes/pods/tensors built
    # above): CPython's gen-2 collector otherwise re-scans the ~2M-object
    # cluster every few thousand allocations — measured 500 ms p99 stalls
    # in churn mode.  Young garbage still collects normally.
    import gc
    gc.collect()
    gc.freeze()
    # churn allocates ~40k tracked objects per cycle — default thresholds
    # fire a full collection every other cycle; space them out (young
    # gens still run at the default cadence)
    gc.set_threshold(700, 10, 1000)

    cycle_times = []
    t0 = time.perf_counter()
    bound = 0
    for _ in range(args.steps):
        ts = time.perf_counter()
        bound += step()
        cycle_times.append(time.perf_counter() - ts)
    sync()
    elapsed = time.perf_counter() - t0

    # MAX elapsed over ranks; SUM of bound pods
    if dist:
        te = torch.tensor([elapsed])
        tb = torch.tensor([float(bound)])
        if use_gpu and torch.distributed.get_backend() == "nccl":
            te, tb = te.cuda(), tb.cuda()
        torch.distributed.all_reduce(te, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(tb, op=torch.distributed.ReduceOp.SUM)
        elapsed = float(te.item())
        bound = int(tb.item())

    # soft-shard reconcile stats (conflict rate in the
    # bench JSON): sum of lost-node incidents across ranks / reconciles
    soft_stats = None
    if coord is not None:
        cs = torch.tensor([float(coord.conflict_nodes),
                           float(coord.reconciles)])
        if use_gpu and torch.distributed.get_backend() == "nccl":
            cs = cs.cuda()
        torch.distributed.all_reduce(cs, op=torch.distributed.ReduceOp.SUM)
        soft_stats = {
            "conflict_nodes_total": int(cs[0].item()),
            "reconciles_total": int(cs[1].item()),
            "conflict_rate": round(
                float(cs[0].item()) / max(float(cs[1].item()), 1.0), 4),
        }

    expected = args.steps * total_pods
    if bound != expected and not args.churn:
        # report honestly; a shortfall means capacity/plan bug, not a perf win
        print(f"WARNING: bound {bound} != expected {expected}", flush=True)

    value = bound / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    if cycle_times:
        import math
        n = len(cycle_times)
        p99 = sorted(cycle_times)[min(n - 1, math.ceil(n * 0.99) - 1)]
    else:
        p99 = 0.0

    if args.dump_outputs:
        dump_outputs(cache, args.dump_outputs, rank)

    if (args.timing or args.full) and rank == 0:
        import sys
        from volcano_amd.utils.metrics import METRICS
        for name in ("open_session_duration",
                     "action_scheduling_latency:enqueue",
                     "action_scheduling_latency:allocate",
                     "action_scheduling_latency:backfill",
                     "allocate:plan_build", "allocate:plan_run",
                     "allocate:apply", "e2e_scheduling_latency"):
            s = METRICS.summary(name)
            if s:
                print(f"[timing] {name}: mean={s['mean']*1000:.1f}ms "
                      f"max={s['max']*1000:.1f}ms n={s['count']}",
                      file=sys.stderr, flush=True)

    if rank == 0:
        out = {
            "metric": "pods_scheduled_per_sec",
            "value": round(value, 2),
            "unit": "pods/s",
            "n_gpus": world if dist else 1,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": round(value / 40.0, 2),
            # second half of the BASELINE metric ("pods scheduled/sec +
            # p99 scheduling-cycle latency")
            "p99_cycle_ms": round(p99 * 1000.0, 2),
            "per_rank_pods_per_sec": round(value / max(world, 1), 2),
            "soft_shard": soft_stats,
            "p99_pod_latency_ms": round(
                (sorted(churn_state["latencies"])[
                    max(0, int(len(churn_state["latencies"]) * 0.99) - 1)]
                 * 1000.0), 2) if churn_state["latencies"] else None,
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": "gang-schedule-10kn-100kp",
                "mode": "churn" if args.churn else "from-empty",
                "global_batch": total_pods,
                "seq_len": args.nodes,
                "parallelism": f"{args.shard_mode}shard{world}",
                "nodes": args.nodes,
                "jobs": args.jobs,
                "pods_per_job": args.pods_per_job,
                "mix": args.mix,
                "decision_plane": "hip-gfx950" if use_gpu else "torch-cpu-oracle",
                "p99_cycle_ms": round(p99 * 1000.0, 2),
            },
        }
        print(json.dumps(out), flush=True)

    if dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
