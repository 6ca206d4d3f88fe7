#!/usr/bin/env python3
"""bench.py -- MNER samples/s (forward + backward) on MI355X, the metric of BASELINE.json.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1], "c2"): bert-base text encoder (H768 L12 h12 I3072) + 36 x 2048 region features,
seq_len 128, per-GPU batch 32, 1 cross-attention layer, gated head, 13 labels; bf16 MFMA compute with fp32
accumulation/statistics; train mode (dropout 0.1 active); loss = token-level cross-entropy over valid tokens;
synthetic Twitter-2015-shaped batches and seeded random-init weights (icka_amd.synth).  One step = forward +
backward of one batch per GPU (+ RCCL gradient all-reduce when N > 1, overlapped with backward).  The optimizer
step is outside the metric and reported beside it: ``with_optimizer_ms_per_step`` = the same step
followed by clip_grad_norm_(1.0) + AdamW.step() (the reference's update, My_cross_attention.py:831-844) with one re-cast
of the bf16 weight shadow per step, measured over a bounded number of steps after the timed region.

A plain run sets up, warms up, times exactly --steps steps, writes the outputs of the last timed step if --dump-outputs DIR
is given, and prints the result line; the side legs below and the optimizer leg are null in it.  --full adds everything
else this file measures: the block of --steps steps timed --repeats times (default 5), the eager / wrapped-module /
host-input / optimizer legs, c4 in pure bf16, the shadow-cast cost, the roofline and the CPU baseline.

Rank 0 prints ONE JSON line with the contract's keys plus (--full)
  roofline      -- the dominant kernel class (the MFMA GEMMs: >= 97 % of algorithmic FLOPs): algorithmic FLOPs of the
                   GEMM launches of one step / their duration, measured live after the timed region: the launches of one
                   step are recorded and re-issued back to back between ONE pair of HIP events on the launch stream;
                   peak = 2.5 PFLOP/s dense bf16 (MI355X_MICROARCH); traffic = PMC bytes per launch from the committed
                   rocprofv3 passes (profiles/r0N_gemm_traffic.json, the newest one).
  cpu_baseline  -- the CPU oracle (oracle/mner_oracle.py; PyTorch CPU eager fp32, same op sequence as the reference)
                   timed on this box's host cores on a bounded sample of the same workload.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md


def log(msg):
    """progress on stderr (the JSON line is the only thing on stdout)"""
    print("[bench %7.1fs] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota (a container on a
    big host reports every host core in os.cpu_count(); oversubscribing the quota makes the CPU leg crawl)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def flops_per_sample(S, R, H, I, L, Lc, C):
    """Algorithmic GEMM FLOPs, forward, per sample; fwd+bwd = 3x."""
    bert = L * (S * (8 * H * H + 4 * H * I) + 4 * S * S * H)
    cross = Lc * (S * (4 * H * H + 4 * H * I) + 4 * R * H * H + 4 * S * R * H)
    return bert + cross + 2 * R * 2048 * H + 4 * S * H * H + 4 * S * H * C


def build_model(args, dev):
    from icka_amd import synth
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(30522, hidden_size=args.hidden, num_hidden_layers=args.layers,
                     num_attention_heads=args.hidden // 64, intermediate_size=4 * args.hidden)
    model = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=args.cross_layers, num_labels=args.labels,
                                                 regions=args.regions, cross_attention_fp8=args.fp8_cross)
    synth.fill_module_(model)
    import icka_amd
    icka_amd.set_precision(model, args.precision)   # explicit: the library default ("auto") would pick by depth
    return model.to(dev).train(), cfg


# BASELINE.json configs[1], [3], [4] (configs[2] = c2 on 8 GPUs: --gpus 8); per-GPU batch 32 unless the config names one
PRESETS = {
    "c2": dict(hidden=768, layers=12, seq=128, regions=36, batch=32, fp8_cross=False),
    "c4": dict(hidden=1024, layers=24, seq=256, regions=50, batch=32, fp8_cross=False, precision="mixed16"),
    "c5": dict(hidden=768, layers=12, seq=128, regions=36, batch=64, fp8_cross=True),
}


def workload_name(args) -> str:
    """BASELINE.json config names: c2/c3 bert-base S128 R36 B32 (the default), c4 bert-large S256 R50, c5 = c2 at B64 with
    fp8 cross-attention; anything else is 'custom'."""
    base = (args.hidden, args.layers, args.seq, args.regions)
    if base == (768, 12, 128, 36) and args.batch == 32 and not args.fp8_cross:
        return "c2"
    if base == (768, 12, 128, 36) and args.batch == 64 and args.fp8_cross:
        return "c5"
    if base == (1024, 24, 256, 50):
        return "c4"
    return "custom"


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(args, fl_sample):
    """Oracle (CPU restatement of the reference path), fwd+bwd, train mode, on a bounded sample of the workload: the
    workload's OWN per-GPU batch when one iteration is at most ~2.5e12 FLOP (c2's batch 32: ~3-5 s per iteration on 16
    threads), else the largest power-of-two batch under that bound (c4, c5) -- stated in ``sample``."""
    from icka_amd import synth
    from oracle import mner_oracle as O
    cores = usable_cores()
    torch.set_num_threads(cores)
    log("cpu baseline on %d threads (os.cpu_count()=%s, %s)" % (cores, os.cpu_count(), cpu_model()))
    if args.cpu_batch <= 0:
        args.cpu_batch = args.batch
        while args.cpu_batch > 1 and args.cpu_batch * fl_sample > 2.5e12:
            args.cpu_batch //= 2
    ocfg = O.OracleConfig(vocab_size=30522, hidden_size=args.hidden, num_hidden_layers=args.layers,
                          num_attention_heads=args.hidden // 64, intermediate_size=4 * args.hidden)
    shapes = O.hot_path_keys(ocfg, args.cross_layers, args.labels)
    P = {k: v.requires_grad_(True) for k, v in synth.seeded_state_dict(shapes).items()}
    bs = args.cpu_batch
    b = synth.synthetic_batch(bs, args.seq, args.regions, num_labels=args.labels)
    times = []
    for it in range(1 + args.cpu_iters):
        for p in P.values():
            p.grad = None
        t0 = time.perf_counter()
        logits = O.mner_logits(P, ocfg, b["input_ids"], b["segment_ids"], b["input_mask"], b["added_attention_mask"],
                               b["visual_embeds_att"], args.cross_layers, args.regions, training=True)
        O.token_ce_loss(logits, b["labels"], b["input_mask"]).backward()
        dt = time.perf_counter() - t0
        log("cpu baseline iteration %d: %.2f s" % (it, dt))
        if it > 0:
            times.append(dt)
    times.sort()
    med = times[len(times) // 2]
    return {"value": round(bs / med, 3), "unit": "samples/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
            "sample": "oracle (PyTorch CPU eager fp32, train mode) fwd+bwd, batch %d%s x seq %d x %d regions, 1 warm-up + "
                      "median of %d iterations, %d threads"
                      % (bs, " (= the workload's per-GPU batch)" if bs == args.batch else " (workload batch %d)" % args.batch,
                         args.seq, args.regions, args.cpu_iters, cores)}


DUMP_BUDGET = 8 << 20   # float32 elements written by --dump-outputs in all (32 MB)


def dump_outputs(path, loss, model):
    """--dump-outputs: what a caller of the timed step holds after its last call -- the loss and every parameter's gradient
    -- as float32 files ``loss.npy`` and ``grad.<parameter name>.npy``.  A gradient larger than its share of DUMP_BUDGET is
    written as a fixed sample: the sorted flat indices drawn by numpy.random.default_rng(crc32 of the parameter name), the
    same in every run and every build at the same arguments."""
    import zlib
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().cpu().numpy())
    grads = [(n, p.grad) for n, p in model.named_parameters() if p.grad is not None]
    cap = DUMP_BUDGET // max(1, len(grads))
    for name, g in grads:
        flat = g.detach().reshape(-1)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(flat.numel(), cap, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(path, "grad.%s.npy" % name), flat.float().cpu().numpy())
    log("outputs of the last timed step: loss + %d gradients -> %s" % (len(grads), path))


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(n: int, json_fd: int) -> int:
    """`python bench.py --gpus N` without a launcher (the reference's launch line, My_cross_attention.py:1104, is
    `python -m torch.distributed.launch --nproc_per_node=N ...`): start `python -m torch.distributed.run` with N ranks as a
    CHILD process, pass the ranks' stderr through, write rank 0's JSON line (the only JSON object on the children's stdout)
    to our stdout and return the launcher's exit status.  Must be called before anything in this process touches the GPU."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    env.pop("MASTER_PORT", None)
    log("self-launch: %s" % " ".join(cmd))
    # the launcher and its ranks get a process group of their own, so that a run that never ends (a collective waiting for a
    # rank that died, a hung device) can be stopped as a whole -- by exactly the group started here -- once the deadline passes
    import signal
    import threading
    deadline = float(os.environ.get("ICKA_BENCH_LAUNCH_TIMEOUT", "1500"))
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, env=env, start_new_session=True)   # stderr inherited
    timed_out = []

    def stop_group(sig):
        try:
            os.killpg(p.pid, sig)
        except (ProcessLookupError, PermissionError):
            pass

    def on_deadline():
        timed_out.append(True)
        log("self-launch: no result after %.0f s (ICKA_BENCH_LAUNCH_TIMEOUT): stopping the ranks" % deadline)
        stop_group(signal.SIGTERM)
        t2 = threading.Timer(20.0, stop_group, args=(signal.SIGKILL,))
        t2.daemon = True
        t2.start()

    timer = threading.Timer(deadline, on_deadline)
    timer.daemon = True
    timer.start()
    line = None
    rc = 1
    try:
        for raw in p.stdout:
            txt = raw.decode("utf-8", "replace").rstrip("\n")
            ok = False
            if txt.startswith("{"):
                try:
                    ok = "metric" in json.loads(txt)
                except ValueError:
                    ok = False
            if ok:
                line = txt
            elif txt:
                print(txt, file=sys.stderr, flush=True)
        rc = p.wait()
    finally:
        timer.cancel()
        if p.poll() is None:     # our own child (its process group), e.g. on KeyboardInterrupt
            stop_group(signal.SIGTERM)
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                stop_group(signal.SIGKILL)
    if timed_out:
        return 124
    if line is not None:
        os.write(json_fd, (line + "\n").encode())
    elif rc == 0:
        log("self-launch: the ranks exited with status 0 but printed no JSON line")
        rc = 1
    return rc


def dry_rank(args, json_fd, world, rank, local_rank):
    """ICKA_BENCH_DRY=1: rehearsal of the N-rank FLOW of this file without a GPU -- what can be proven about `--gpus 8` on a
    box with fewer devices (this pool allows at most 6 processes on a card): launcher, port, rendezvous over gloo, the
    rank -> device map (LOCAL_RANK, as the reference's `--local_rank`, My_cross_attention.py:653-657), barrier + max-over-ranks
    timing, legs that only rank 0 runs while the others wait at the barrier, and the relay of rank 0's single JSON line.  The
    step itself is a sleep: the JSON line says so ("dry": true) and carries no roofline / cpu_baseline."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    dev_index = 0 if os.environ.get("ICKA_BENCH_ONE_GPU") else local_rank
    devs = [None] * world
    dist.all_gather_object(devs, (rank, dev_index))
    for _ in range(args.warmup):
        time.sleep(0.001)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 + 0.0005 * rank)           # the slowest rank sets the time
    dist.barrier()
    tmax = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = tmax.item()
    if rank == 0:
        time.sleep(0.2)                              # rank-0-only legs (roofline, cpu baseline): the others wait below
    dist.barrier()
    if rank == 0:
        # NOT the headline metric's name: a harness that ignores "dry" must not book a sleep as a throughput
        out = {"metric": "DRY RUN of the bench.py launch flow (sleeps, no kernels): ranks x batch %d / slowest rank's sleep" % args.batch,
               "value": round(args.batch * world * args.steps / dt, 2), "unit": "samples/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none (dry run)", "data": "none",
               "dry": True, "rank_devices": sorted(devs),
               "config": {"workload": "DRY RUN of the launch flow: no kernels ran", "global_batch": args.batch * world,
                          "parallelism": "dp%d" % world}, "roofline": None, "cpu_baseline": None}
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=None,
                    help="the block of --steps timed steps is run this many times back to back (same graph, same batch pool, each "
                         "block bracketed by barrier + synchronize and reduced by MAX over ranks); value / ms_per_step come from "
                         "the MEDIAN block, ms_per_step_min / _max give the run's own spread (default: 5 with --full, else 1)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: --repeats 5, the eager / wrapped-module / host-input / optimizer "
                         "legs, c4 in pure bf16, the shadow-cast cost, the roofline and the CPU baseline (each can be left out "
                         "with its --no-* flag)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss and the parameter gradients of the last timed step to DIR/*.npy (float32; large "
                         "gradients as a fixed sample, see dump_outputs)")
    ap.add_argument("--config", choices=sorted(PRESETS), default=None,
                    help="BASELINE.json configuration preset (default: c2, the configuration the metric is quoted on); "
                         "explicit shape flags override the preset")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch")
    ap.add_argument("--seq", type=int, default=None)
    ap.add_argument("--regions", type=int, default=None)
    ap.add_argument("--hidden", type=int, default=None)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--cross-layers", type=int, default=1)
    ap.add_argument("--labels", type=int, default=13)
    ap.add_argument("--fp8-cross", action="store_true", default=None,
                    help="BASELINE config c5: fp8 QK^T / PV in the cross-attention")
    ap.add_argument("--precision", choices=("bf16", "mixed16"), default=None,
                    help="arithmetic of the 16-bit path: bf16 (default for c2 / c5), or mixed16 = fp16 operands in the forward "
                         "GEMMs of the encoder layers + bf16 backward (default for c4, whose 24 layers exceed the 2e-2 logit "
                         "bar in pure bf16: DESIGN.md section 2)")
    ap.add_argument("--cpu-batch", type=int, default=0, help="0 = the workload's batch, bounded (see cpu_baseline)")
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--bucket-mb", type=float, default=50.0,
                    help="minimum gradient bucket size in MB of fp32 gradients (the embedding tables are always a bucket of "
                         "their own): every bucket is a fork/join of the captured graph, see DESIGN.md section 6")
    ap.add_argument("--comm-f32", action="store_true", help="fp32 gradient buckets on the wire (the library default; the "
                                                            "bench's default at N > 1 is bf16, see DESIGN.md section 6)")
    ap.add_argument("--comm-bf16", action="store_true", help="force bf16 buckets (already the bench's default at N > 1)")
    ap.add_argument("--sparse-embeddings", action="store_true",
                    help="data parallel: exchange the word-embedding gradient as all-gathered token rows instead of the dense "
                         "[vocab, H] all-reduce (dp.GradReducer(sparse_embeddings=True); halves the bytes of the exposed tail at "
                         "N <= 4, about even at N = 8 x 4096 tokens: profiles/r04_dp_budget.md)")
    ap.add_argument("--dp-step", choices=("flagged", "segmented"), default="flagged",
                    help="data parallel: 'flagged' = ONE hipGraph whose bucket-ready points are flag words waited for on the "
                         "communication stream (graph.FlaggedStep); 'segmented' = linear graph segments with the all-reduces "
                         "between them (graph.SegmentedStep, the round-2 form and the fallback)")
    ap.add_argument("--dp-diag", default="", help="DIAGNOSTIC: GradReducer(diag=...) -- 'none', 'cast', 'comm', 'cast,comm': "
                                                  "prices parts of the exchange, the gradients are wrong")
    ap.add_argument("--with-optimizer", action="store_true", help="(kept for round-1/2 command lines; the optimizer leg "
                                                                  "runs with --full unless --no-optimizer-leg)")
    ap.add_argument("--no-optimizer-leg", action="store_true", help="skip the fwd+bwd+clip+AdamW leg")
    ap.add_argument("--accumulate", type=int, default=1,
                    help="micro-batches per gradient exchange / zero_grad (the reference's gradient_accumulation_steps, "
                         "My_cross_attention.py:587-590; default 1 = the metric's one exchange per forward+backward).  A step "
                         "stays one forward+backward of one batch per GPU; with k > 1 the captured step accumulates and, "
                         "data-parallel, only every k-th step exchanges (graph.FlaggedStep(accumulate=k))")
    ap.add_argument("--no-eager-leg", action="store_true", help="skip the eager (no hipGraph) timing of the same step")
    ap.add_argument("--eager-leg-dist", action="store_true",
                    help="run the eager leg at N > 1 as well (default: N = 1 only -- it is a report about the import swap, and a "
                         "side leg must not put a multi-rank run at risk)")
    ap.add_argument("--eager-steps", type=int, default=10, help="steps of the eager leg (bounded: it is a side report)")
    ap.add_argument("--optimizer-steps", type=int, default=20, help="steps of the optimizer leg (bounded: it is a side report)")
    ap.add_argument("--shadow-always", action="store_true",
                    help="keep the library default: re-cast the bf16 weight shadow in every forward.  The bench's default is "
                         "the 'tracked' policy: the optimizer is outside the metric (SURVEY.md section 8d), so the weights do "
                         "not change between the timed steps and the cast -- the tail of an optimizer step -- has nothing to do; "
                         "its cost is reported as shadow_cast_us")
    ap.add_argument("--capture-collectives", action="store_true",
                    help="data parallel: capture the all-reduces INSIDE one hipGraph (side-stream branches) instead of the "
                         "default linear segments with eager all-reduces between them")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying the captured hipGraph")
    ap.add_argument("--force-dist", action="store_true", help="init the process group even with one rank (tests the "
                                                              "RCCL path on a single GPU)")
    args = ap.parse_args()
    for k, v in PRESETS[args.config or "c2"].items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    if args.precision is None:
        args.precision = "bf16"
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if not args.full:   # a plain run: set-up, warm-up, the timed steps, the outputs and the result line only
        args.no_eager_leg = args.no_optimizer_leg = args.no_roofline = args.no_cpu_baseline = True

    # stdout carries exactly ONE line (the JSON).  Native libraries write there too -- RCCL prints a five-line version banner
    # to fd 1 when its first communicator is created -- so fd 1 is pointed at stderr for the whole run and the JSON line is
    # written to a duplicate of the original stdout at the end.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` started directly: become the launcher.  Nothing in this process has touched the GPU
        # yet (no HIP call, no torch.cuda.is_available()); the N ranks are CHILD processes of a torch.distributed.run
        # child -- never an exec of this process -- and this process relays rank 0's JSON line and the exit status.
        sys.exit(self_launch(args.gpus, json_fd))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if os.environ.get("ICKA_BENCH_DRY"):
        return dry_rank(args, json_fd, world, rank, local_rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path in icka_amd)")
    if os.environ.get("ICKA_BENCH_ONE_GPU"):   # rehearsal of the N > 1 flow on a one-GPU box (with ICKA_BENCH_BACKEND=gloo)
        local_rank = 0
        # several ranks share the card: launches whose blocks wait for each other inside the kernel (icka_gemm_ln) cannot
        # count on the whole chip -- from the very first step on, before any reducer has reserved CUs
        from icka_amd import ops as _ops
        _ops.FUSE_DENSE_LN = False
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    import torch.distributed as dist
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        backend = os.environ.get("ICKA_BENCH_BACKEND", "nccl")   # "nccl" = RCCL; gloo only for the one-GPU rehearsal
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    from icka_amd import kernels as K
    from icka_amd import synth
    torch.manual_seed(synth.REFERENCE_SEED)
    log("building model")
    model, cfg = build_model(args, dev)
    # each rank draws a disjoint slice of the synthetic stream (reference: DistributedSampler, :707).  The reference's loop
    # feeds a NEW batch every step (My_cross_attention.py:797-798): the timed steps rotate through POOL different batches
    # that are resident in HBM before the timed region starts, and the captured step copies each into its static input
    # buffers before the replay (graph.StaticInputs; the copy is inside the timed region and reported as refresh_us).
    NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att",
             "labels")
    POOL = 4
    pool = []
    for i in range(POOL):
        b = synth.synthetic_batch(args.batch, args.seq, args.regions, num_labels=args.labels,
                                  seed=synth.REFERENCE_SEED + rank + 1000 * i)
        pool.append(tuple(b[k].to(dev) for k in NAMES))
    g = dict(zip(NAMES, pool[0]))

    one = torch.ones((), dtype=torch.float32, device=dev)   # root gradient (else autograd fills a fresh ones_like per step)

    def step(ids, seg, mask, added, vmean, vatt, labels):
        loss = model(ids, seg, mask, added, vmean, vatt, labels=labels)
        loss.backward(gradient=one)
        if reducer is not None:
            reducer.finish()
        return loss

    reducer = None
    step_loss = None
    log("first step (builds the parameter arena)")
    # first step builds the arena; attach the reducer afterwards
    model.zero_grad()
    loss = model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"],
                 g["visual_embeds_mean"], g["visual_embeds_att"], labels=g["labels"])
    loss.backward()
    arena = model._icka_arena
    if not args.shadow_always:
        arena.shadow_policy = "tracked"
    if use_dist:
        from icka_amd.dp import GradReducer
        reducer = GradReducer(arena, bucket_mb=args.bucket_mb, comm_dtype="f32" if args.comm_f32 else "bf16",
                              diag=args.dp_diag, sparse_embeddings=args.sparse_embeddings)
        reducer.broadcast_parameters(0)
        arena.reducer = reducer
    opt = None
    if not args.no_optimizer_leg:
        from icka_amd.optim import ArenaAdamW
        # the reference's update (My_cross_attention.py:743-751, :831-844): two weight-decay groups, clip at 1.0, lr 3e-5
        opt = ArenaAdamW(model, lr=3e-5, weight_decay=0.01, max_grad_norm=1.0)

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- the form the step runs in: ONE decision point (graph.build_step).  At N = 1: one hipGraph, else eager launches.
    #      Under data parallelism the chain flagged -> segmented -> captured compute + eager all-reduces -> eager is walked by
    #      ALL ranks together: each form warms up (collectives, identical on every rank), captures in a phase without
    #      process-group traffic, and the ranks vote over the c10d store before anyone uses the result
    from icka_amd.graph import build_step
    run_step, mode = build_step(model, step, inputs=pool[0], reducer=reducer, accumulate=args.accumulate,
                                prefer=args.dp_step, graph=not args.no_graph, capture_collectives=args.capture_collectives,
                                log=log)

    log("warm-up %d steps" % args.warmup)
    acc_k = max(1, args.accumulate)
    if acc_k > 1 and reducer is not None and not mode.startswith("hipgraph+flag-waits"):
        raise SystemExit("--accumulate > 1 under data parallelism needs the flagged step (the other forms exchange every step)")
    for i in range(args.warmup):
        if i % acc_k == 0:
            model.zero_grad()
        step_loss = run_step(*pool[i % POOL])
    model.zero_grad()
    sync()
    repeats = max(1, args.repeats)
    log("timing %d x %d steps (%s)" % (repeats, args.steps, mode))
    blocks = []
    ctr = 0
    for rep in range(repeats):
        sync()
        t0 = time.perf_counter()
        for i in range(args.steps):
            # the reference drops the gradients after every optimisation step (:843); set_to_none: the next backward overwrites
            # the gradient arena (no memset) -- a captured step replays its overwrite capture
            if ctr % acc_k == 0:
                model.zero_grad()
            step_loss = run_step(*pool[ctr % POOL])
            ctr += 1
        sync()
        dt = time.perf_counter() - t0
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        blocks.append(tmax.item())
    order = sorted(blocks)
    dt = order[(len(order) - 1) // 2]            # the median block (the lower one of an even count)
    ms_per_step = 1e3 * dt / args.steps
    ms_blocks = [round(1e3 * b / args.steps, 4) for b in blocks]
    samples_per_s = args.batch * world * args.steps / dt
    final_loss = float(step_loss.item())
    log("%.3f ms/step (median of %d blocks: %s), %.1f samples/s, loss %.4f"
        % (ms_per_step, repeats, " ".join("%.3f" % m for m in ms_blocks), samples_per_s, final_loss))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_loss, model)

    # ---- what the import swap of INTEGRATION.md section 1 costs WITHOUT the capture harness: the same step launched eagerly
    #      from Python (autograd + ctypes launches), bounded steps; and what the per-call input refresh of the harness costs
    eager_ms, refresh_us, wrapped_ms, host_ms, host_pf_ms, host_bytes = None, None, None, None, None, 0
    try:       # side reports: never allowed to take the headline down with them
        if not args.no_eager_leg and (world == 1 or args.eager_leg_dist):
            n_eager = max(2, min(args.steps, args.eager_steps))
            for i in range(2):
                model.zero_grad()
                step(*pool[i % POOL])
            sync()
            t1 = time.perf_counter()
            for i in range(n_eager):
                model.zero_grad()
                step(*pool[i % POOL])
            sync()
            te = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
            if use_dist:
                dist.all_reduce(te, op=dist.ReduceOp.MAX)
            eager_ms = 1e3 * te.item() / n_eager
            log("eager launches (no hipGraph): %.3f ms/step over %d steps" % (eager_ms, n_eager))
        if not args.no_eager_leg and world == 1 and not args.no_graph:
            # the same loop body as the eager leg -- loss = model(...); loss.backward() -- through graph.GraphedModule (a forward
            # and a backward hipGraph behind the module's own call): what the import swap + ONE wrapping line gets
            from icka_amd.graph import GraphedModule
            gm = None
            try:
                gm = GraphedModule(model, pool[0][:6], {"labels": pool[0][6]})
                n_w = max(2, min(args.steps, 2 * args.eager_steps))
                for i in range(3):
                    model.zero_grad()
                    gm(*pool[i % POOL][:6], labels=pool[i % POOL][6]).backward(gradient=one)
                sync()
                t1 = time.perf_counter()
                for i in range(n_w):
                    model.zero_grad()
                    gm(*pool[i % POOL][:6], labels=pool[i % POOL][6]).backward(gradient=one)
                sync()
                wrapped_ms = 1e3 * (time.perf_counter() - t1) / n_w
                log("GraphedModule (loop body unchanged): %.3f ms/step over %d steps" % (wrapped_ms, n_w))
            finally:
                if gm is not None:
                    gm.close()
                if getattr(run_step, "nonce", None) is not None:   # the timed step's dropout nonce is the registered one again,
                    K.set_dropout_nonce(run_step.nonce)            # also when this side leg failed half-way
        static = getattr(run_step, "inputs", None)
        if static is not None and args.full:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            static.refresh(pool[1], {})
            torch.cuda.synchronize()
            e0.record()
            for i in range(20):
                static.refresh(pool[i % POOL], {})
            e1.record()
            torch.cuda.synchronize()
            refresh_us = 50.0 * e0.elapsed_time(e1)
            if world == 1 and hasattr(run_step, "inputs"):
                # the PCIe-inclusive rate: the reference's loop moves every batch from the host inside the step
                # (My_cross_attention.py:797-798); here the POOL batches sit in pinned host memory and each timed call hands
                # the host tensors to the captured step (copy_ on the step's stream, then the replay).  Never the headline.
                host_pool = [tuple(t.cpu().pin_memory() for t in b) for b in pool]
                n_h = max(2, min(args.steps, 20))
                for i in range(2):
                    model.zero_grad()
                    run_step(*host_pool[i % POOL])
                sync()
                t1 = time.perf_counter()
                for i in range(n_h):
                    model.zero_grad()
                    run_step(*host_pool[i % POOL])
                sync()
                host_ms = 1e3 * (time.perf_counter() - t1) / n_h
                host_bytes = sum(t.numel() * t.element_size() for t in host_pool[0])
                log("host-resident (pinned) batches, %.1f MB over PCIe per step: %.3f ms/step" % (host_bytes / 1e6, host_ms))
                # the same host batches one step ahead on a copy stream (graph.DevicePrefetcher): PCIe off the critical path
                from icka_amd.graph import DevicePrefetcher
                feed = iter(DevicePrefetcher((host_pool[i % POOL] for i in range(n_h + 2)), dev))
                for _ in range(2):
                    model.zero_grad()
                    run_step(*next(feed))
                sync()
                t1 = time.perf_counter()
                for b in feed:
                    model.zero_grad()
                    run_step(*b)
                sync()
                host_pf_ms = 1e3 * (time.perf_counter() - t1) / n_h
                log("the same through DevicePrefetcher (next batch copied under the current step): %.3f ms/step" % host_pf_ms)

    except Exception as e:  # noqa: BLE001
        log("eager / refresh side report failed (%s: %s): reported as null" % (type(e).__name__, e))
        torch.cuda.synchronize()

    # ---- BASELINE config 4 says bf16; the step above runs c4 in "mixed16" (fp16 forward operands), because pure bf16 measures
    #      2.2e-2 .. 2.5e-2 max abs logit error at 24 layers, above north_star's 2e-2 (tests/test_fullsize_gpu.py).  The
    #      configuration AS STATED goes on the record beside it: the same step captured again in pure bf16, same batches.
    stated = None
    if workload_name(args) == "c4" and args.precision != "bf16" and world == 1 and not args.no_graph and not args.no_eager_leg:
        gs2 = None
        try:
            import icka_amd
            from icka_amd.graph import GraphedStep
            icka_amd.set_precision(model, "bf16")
            gs2 = GraphedStep(model, step, inputs=pool[0])
            for i in range(3):
                model.zero_grad()
                gs2(*pool[i % POOL])
            sync()
            t1 = time.perf_counter()
            for i in range(args.steps):
                model.zero_grad()
                gs2(*pool[i % POOL])
            sync()
            ms2 = 1e3 * (time.perf_counter() - t1) / args.steps
            stated = {"precision": "bf16 (the configuration as BASELINE.json states it)", "ms_per_step": round(ms2, 3),
                      "samples_per_s": round(args.batch / (ms2 * 1e-3), 2), "steps": args.steps,
                      "max_abs_logit_err_vs_oracle": "2.2e-2 .. 2.5e-2 at 24 layers (tests/test_fullsize_gpu.py, documented 3e-2 "
                                                     "leg): above north_star's 2e-2 bar, which is why the headline of this line "
                                                     "runs mixed16 (3.9e-3)"}
            log("c4 in pure bf16 (configuration as stated): %.3f ms/step" % ms2)
        except Exception as e:  # noqa: BLE001
            log("pure-bf16 side leg failed (%s: %s): reported as null" % (type(e).__name__, e))
            torch.cuda.synchronize()
        finally:
            import icka_amd
            icka_amd.set_precision(model, args.precision)
            if gs2 is not None:
                gs2.close()
            if getattr(run_step, "nonce", None) is not None:
                K.set_dropout_nonce(run_step.nonce)

    # what the default ("always") shadow policy adds to a step: one f32 -> bf16 cast of the GEMM weights
    shadow_cast_us = None
    if args.full:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        arena.sync(force=True)
        e0.record()
        for _ in range(10):
            arena.sync(force=True)
        e1.record()
        torch.cuda.synchronize()
        shadow_cast_us = 100.0 * e0.elapsed_time(e1)

    # ---- the optimizer beside the metric: the same step + clip_grad_norm_(1.0) + AdamW.step(), as the
    #      reference's loop does after backward (My_cross_attention.py:831-844).  Every optimizer step is seen by the arena
    #      (global post-step hook), so each of these steps re-casts the bf16 weight shadow once -- what the library's default
    #      "always" policy does per forward -- and the figure prices the "tracked" policy's exclusion from the headline number.
    opt_ms, opt_steps, opt_torch_ms = None, 0, None
    if opt is not None:
        params = [p for p in model.parameters()]
        opt_steps = max(1, min(args.steps, args.optimizer_steps))

        def time_update(update):
            ctr = [0]

            def one():
                model.zero_grad()
                run_step(*pool[ctr[0] % POOL])
                ctr[0] += 1
                update()
            for _ in range(3):
                one()
            sync()
            t1 = time.perf_counter()
            for _ in range(opt_steps):
                one()
            sync()
            tt = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
            if use_dist:
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return 1e3 * tt.item() / opt_steps
        opt_ms = time_update(opt.step)       # clip + AdamW on the flat arena buffers: three launches (icka_amd/optim.py)
        log("with clip + AdamW (ArenaAdamW): %.3f ms/step over %d steps" % (opt_ms, opt_steps))
        # the same update through the stock per-tensor optimizer, for the record (what round 2's loop would have paid)
        from icka_amd.optim import reference_param_groups
        topt = torch.optim.AdamW(reference_param_groups(model, 0.01), lr=3e-5)

        def torch_update():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            topt.step()
        opt_torch_ms = time_update(torch_update)
        log("with clip_grad_norm_ + torch.optim.AdamW: %.3f ms/step" % opt_torch_ms)
        del topt

    # ---- roofline of the dominant kernel class (MFMA GEMMs), instrumented pass, rank 0 only, N = 1 semantics
    roof = None
    fl_sample = 3 * flops_per_sample(args.seq, args.regions, args.hidden, 4 * args.hidden, args.layers,
                                     args.cross_layers, args.labels)
    if rank == 0 and not args.no_roofline:
        # one eager step records every GEMM launch (descriptor + operands); the recorded launches are then re-issued
        # back to back nprof times between one pair of HIP events on the launch stream, so the bracket holds GEMM
        # kernels only (no host gaps, no per-launch event cost) -- comparable with rocprofv3's per-kernel durations
        K.profile_gemm(True)
        nprof = 5
        model.zero_grad()
        # forward + backward WITHOUT the gradient reducer: at N > 1 only rank 0 runs this leg, a collective issued here
        # would pair with the other ranks' barrier below
        arena.reducer = None
        rl = model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"],
                   g["visual_embeds_mean"], g["visual_embeds_att"], labels=g["labels"])
        rl.backward()
        arena.reducer = reducer
        torch.cuda.synchronize()
        flops, ms, launches, abytes = K.profile_gemm(False, reps=nprof)
        fused, fused_qa = K.last_fused_profile, K.last_fused_qkv_profile
        traffic, traffic_src = None, None
        tpath = None
        for tag in ("r05", "r04", "r03", "r02", "r01"):      # the newest committed PMC passes
            cand = os.path.join(ROOT, "profiles", "%s_gemm_traffic.json" % tag)
            if os.path.exists(cand):
                tpath = cand
                break
        # PMC passes cannot run inside this process: taken from the committed rocprofv3 runs (measured on c2 only)
        if tpath is not None and workload_name(args) == "c2":   # (measured on c2 only)
            tj = json.load(open(tpath))
            traffic, traffic_src = round(tj["traffic_bytes_per_launch"]), "profiles/%s (%s)" % (os.path.basename(tpath), tj["method"])
        # MFMA-busy counters of the same GEMM launches (SQ_VALU_MFMA_BUSY_CYCLES, separate rocprofv3 --pmc pass over the eager
        # step: tools/profile_mfma.sh -> profiles/r0N_mfma_busy_<config>.json); like `traffic`, not collectable in-process
        mfma_busy = None
        for tag in ("r05", "r04"):
            cand = os.path.join(ROOT, "profiles", "%s_mfma_busy_%s.json" % (tag, workload_name(args)))
            if os.path.exists(cand):
                mj = json.load(open(cand))
                gc = mj.get("classes", {}).get("gemm")
                if gc:
                    mfma_busy = {"gemm_class_mfma_util_pct": gc["mfma_util_pct"],
                                 "gemm_class_busy_frac_of_nominal_peak": gc["mfma_busy_frac_of_nominal_peak"],
                                 "all_kernels_mfma_util_pct": mj.get("all_kernels_mfma_util_pct"),
                                 "source": "profiles/%s (SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs); busy cycles / "
                                           "(1024 SIMDs x traced duration x 2.4 GHz): a profiled eager pass)" % os.path.basename(cand)}
                break
        if ms > 0:
            ach = flops / (ms * 1e-3) / 1e12
            roof = {"bound": "mfma",
                    "kernel": "the GEMM launches of a step: gemm_ws_kernel / gemm_ws2_kernel (128x128, 128x96 tiles), "
                              "gemm_w3_kernel (256x192), gemm_big_group_kernel (grouped weight gradients, 256x128), "
                              "gemm_kernel (ragged shapes); NT / NN / TN, bf16 MFMA 16x16x32 (the dense GEMMs fused with their "
                              "LayerNorm, gemm_ln_kernel, and the QKV projections fused with their attention, gemm_qkv_attn_kernel, are listed "
                              "under fused_dense_ln / fused_qkv_attn)",
                    "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "traffic_unit": "bytes/launch",
                    "traffic_source": traffic_src, "mfma_busy": mfma_busy, "algorithmic_bytes_per_launch": round(abytes / launches),
                    "algorithmic_flop_per_launch": round(flops / launches),
                    "launches_per_step": launches // nprof, "avg_launch_us": round(1e3 * ms / launches, 2),
                    "gemm_ms_per_step": round(ms / nprof, 3),
                    # the dense GEMMs whose LayerNorm runs inside the same launch (gemm_ln_kernel: the 128x96 / 128x128 tile body
                    # + a stripe hand-off + the row phase) are timed in a bracket of their own -- their duration contains the
                    # HBM-bound LayerNorm phase -- and are NOT part of achieved / frac above
                    "fused_dense_ln": None if not fused else {
                        "launches_per_step": fused["launches"] // nprof, "avg_launch_us": round(1e3 * fused["ms"] / fused["launches"], 2),
                        "gemm_flop_per_launch": round(fused["flops"] / fused["launches"]),
                        "ms_per_step": round(fused["ms"] / nprof, 3),
                        "gemm_tflops_incl_layernorm_phase": round(fused["flops"] / (fused["ms"] * 1e-3) / 1e12, 2)},
                    # the QKV projections whose self-attention runs inside the same launch (gemm_qkv_attn_kernel: the 256x192
                    # tile body, then the whole-head attention of the tile's two samples x one head from LDS); GEMM FLOPs only
                    "fused_qkv_attn": None if not fused_qa else {
                        "launches_per_step": fused_qa["launches"] // nprof,
                        "avg_launch_us": round(1e3 * fused_qa["ms"] / fused_qa["launches"], 2),
                        "gemm_flop_per_launch": round(fused_qa["flops"] / fused_qa["launches"]),
                        "ms_per_step": round(fused_qa["ms"] / nprof, 3),
                        "gemm_tflops_incl_attention_phase": round(fused_qa["flops"] / (fused_qa["ms"] * 1e-3) / 1e12, 2)},
                    "whole_step_tflops": round(samples_per_s / world * fl_sample / 1e12, 2),
                    "whole_step_frac": round(samples_per_s / world * fl_sample / 1e12 / PEAK_BF16_TFLOPS, 4)}

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, fl_sample)

    if use_dist:
        dist.barrier()
    if rank == 0:
        out = {
            "metric": "MNER samples/sec (fwd+bwd) at seq=%d, %d regions, bs=%d per GPU" % (args.seq, args.regions, args.batch),
            "value": round(samples_per_s, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            # the run's own noise bar: `repeats` blocks of `steps` steps each, value / ms_per_step from the MEDIAN block
            "repeats": repeats, "ms_per_step_min": round(1e3 * min(blocks) / args.steps, 3),
            "ms_per_step_max": round(1e3 * max(blocks) / args.steps, 3),
            "ms_per_step_blocks": ms_blocks,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.precision == "bf16" else "fp16 forward operands + bf16 backward (16-bit MFMA, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "%s: bert(H%d,L%d,h%d,I%d)+%dx2048 regions, seq_len %d, per-GPU batch %d, "
                                   "%d cross layer(s)%s, gated head, %d labels, train mode p=0.1, token-CE loss"
                                   % (workload_name(args), args.hidden, args.layers, args.hidden // 64, 4 * args.hidden,
                                      args.regions, args.seq, args.batch, args.cross_layers,
                                      " with fp8 QK^T/PV" if args.fp8_cross else "", args.labels),
                       "global_batch": args.batch * world, "seq_len": args.seq, "regions": args.regions,
                       "parallelism": "dp%d" % world, "flops_per_sample_fwd_bwd": fl_sample, "launch": mode,
                       "precision": args.precision, "accumulate": acc_k,
                       "shadow_policy": arena.shadow_policy,
                       "gradient_exchange": None if reducer is None else
                       "%s buckets x %d, %s on the wire (%d MB per rank and step)%s"
                       % ("bf16" if reducer.comm_bf16 else "f32", len(reducer.buckets), reducer.backend,
                          reducer.wire_bytes() >> 20, (" DIAG=" + args.dp_diag) if args.dp_diag else "") +
                       ("" if reducer.sparse_word is None else "; word-embedding gradient as all-gathered token rows")},
            "shadow_cast_us": None if shadow_cast_us is None else round(shadow_cast_us, 1),
            # the same step without the capture harness (eager launches from Python: what a plain import swap of the
            # reference's modules gets), and the per-call copy of a new batch into the captured step's static input buffers
            # (inside the timed region: every timed step is fed another batch)
            "eager_ms_per_step": None if eager_ms is None else round(eager_ms, 3),
            "eager_samples_per_s": None if eager_ms is None else round(args.batch * world / (eager_ms * 1e-3), 2),
            "refresh_us": None if refresh_us is None else round(refresh_us, 1),
            # loss = model(...); loss.backward() unchanged, the module wrapped once in icka_amd.graph.GraphedModule
            "wrapped_module_ms_per_step": None if wrapped_ms is None else round(wrapped_ms, 3),
            # PCIe-inclusive: the same captured step fed from pinned HOST tensors (H2D copies on the step's stream, serial with it)
            "host_inputs_ms_per_step": None if host_ms is None else round(host_ms, 3),
            "host_inputs_samples_per_s": None if host_ms is None else round(args.batch / (host_ms * 1e-3), 2),
            "host_inputs_prefetched_ms_per_step": None if host_pf_ms is None else round(host_pf_ms, 3),
            "host_input_bytes_per_step": host_bytes or None,
            "inputs": "%d different synthetic batches per rank, resident in HBM, rotated: every timed step copies the next one "
                      "into the captured step's static input buffers" % POOL,
            "loss": round(final_loss, 5),
            "roofline": roof, "cpu_baseline": cpu,
        }
        if stated is not None:
            out["config_as_stated"] = stated
        if opt_ms is not None:
            out["with_optimizer_ms_per_step"] = round(opt_ms, 3)
            out["with_optimizer"] = {"update": "icka_amd.optim.ArenaAdamW: global-norm clip at 1.0 + AdamW (two weight-decay groups, "
                                               "lr 3e-5) over %d nn.Parameters as 4 launches on the flat arena buffers; the update "
                                               "kernel also writes the bf16 weight shadow" % len(params),
                                     "steps": opt_steps, "shadow_casts_per_step": 0,
                                     "samples_per_s": round(args.batch * world / (opt_ms * 1e-3), 2),
                                     "torch_optim_ms_per_step": None if opt_torch_ms is None else round(opt_torch_ms, 3),
                                     "torch_optim": "clip_grad_norm_(1.0) + torch.optim.AdamW, same groups (one shadow cast per step)"}
        if cpu is not None:
            out["gpu_over_cpu"] = round(samples_per_s / cpu["value"], 1)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
