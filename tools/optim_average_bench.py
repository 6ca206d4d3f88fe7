#!/usr/bin/env python3
"""What the averaged weights of ArenaAdamW(average=...) cost at the c2 model's arena (bert-base, 36 regions), in bf16 and
mixed16, in ONE process:

  * the launches alone, over the whole arena, device events around 100 launches per block, alternating blocks:
    icka_optim_average (12 B per parameter: read p, read avg, write avg), icka_optim_swap (16 B + the 16-bit shadows) and
    icka_optim_adamw_dev (28 B + the shadows) -- with the bytes each moves and the rate that gives;
  * the TrainStep replay (seq 128, batch 32, train mode, k = 1) with and without average="ema", alternating blocks.

Prints medians and block spreads (max - min).  No time is asserted anywhere.
usage: python tools/optim_average_bench.py [--micro 100] [--blocks 5] [--out profiles/optim_average.txt]"""
import argparse
import copy
import os
import platform
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import icka_amd  # noqa: E402
from icka_amd import kernels as K  # noqa: E402
from icka_amd import synth  # noqa: E402
from icka_amd.config import BertConfig  # noqa: E402
from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF  # noqa: E402
from icka_amd.optim import ArenaAdamW  # noqa: E402

NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def summary(xs):
    return statistics.median(xs), max(xs) - min(xs)


def launches_alone(base, pool, blocks, precision, lines):
    model = icka_amd.set_precision(copy.deepcopy(base), precision).cuda().train()
    (model(*pool[0][:6], labels=pool[0][6])).backward()
    torch.cuda.synchronize()
    A = model._icka_arena
    opt = ArenaAdamW(model, lr=0.0, weight_decay=0.0, capturable=True, average="ema")     # rate 0: the weights stay where they are
    opt.prepare_capture()
    K.optim_sqnorm(A.gflat, opt._norm_table, opt._partials)
    K.optim_prepare(opt._partials, opt._norm_table.shape[0], 0.0, opt._state)
    n_avg = int(opt._avg_table[:, 1].sum().item())
    n_upd = int(opt._table3[:, 1].sum().item())
    sh_bytes = 2 * (A.shadow is not None) + 2 * (A.shadow16 is not None)
    legs = [
        ("icka_optim_average   ", lambda _: K.optim_average(A.flat, opt._avg, opt._avg_table, 0.999), 12 * n_avg, opt._avg_table.shape[0]),
        ("icka_optim_swap      ", lambda _: K.optim_swap(A.flat, opt._avg, A.shadow, A.shadow16, opt._avg_table),
         (16 + sh_bytes) * n_avg, opt._avg_table.shape[0]),
        ("icka_optim_adamw_dev ", lambda _: K.optim_adamw_dev(A.flat, A.gflat, opt._m, opt._v, A.shadow, A.shadow16, opt._table3,
                                                              opt._state), (28 + sh_bytes) * n_upd, opt._table3.shape[0]),
    ]
    for _, f, _, _ in legs:
        timed(f, 20)
    times = [[] for _ in legs]
    for _ in range(blocks):
        for i, (_, f, _, _) in enumerate(legs):
            times[i].append(1e3 * timed(f, 100))            # (100 launches: the swap runs an even number of times)
    lines.append("%s: arena of %d f32 elements (%d in the update's table, %d in the average's); shadows: %d B per element"
                 % (precision, A.total, n_upd, n_avg, sh_bytes))
    for (name, _, nbytes, chunks), t in zip(legs, times):
        med, spread = summary(t)
        lines.append("  %s %5d chunks  median %8.2f us (spread %6.2f)  %7.1f MB moved  -> %6.0f GB/s"
                     % (name, chunks, med, spread, nbytes / 1e6, nbytes / (med * 1e-6) / 1e9))
    m_avg, m_upd = summary(times[0])[0], summary(times[2])[0]
    lines.append("  the averaging launch takes %.2f of the AdamW launch's time and moves %.2f of its bytes"
                 % (m_avg / m_upd, legs[0][2] / legs[2][2]))
    print("\n".join(lines[-5:]), flush=True)


def replay(base, pool, blocks, micro_n, precision, lines):
    def build(average):
        model = icka_amd.set_precision(copy.deepcopy(base), precision).cuda().train()

        def micro(ids, seg, mask, added, vmean, vatt, labels):
            loss = model(ids, seg, mask, added, vmean, vatt, labels=labels)
            loss.backward()
            return loss

        micro(*pool[0])
        model.zero_grad()
        model._icka_arena.shadow_policy = "tracked"
        opt = ArenaAdamW(model, lr=3e-5, weight_decay=0.01, max_grad_norm=1.0, capturable=True,
                         schedule=("linear", 100, 1000000), average=average)
        ts = icka_amd.TrainStep(model, micro, opt, inputs=pool[0], accumulate=1)
        return (lambda i: ts(*pool[i % len(pool)])), ts

    a, obj_a = build(None)
    b, obj_b = build("ema")
    for f in (a, b):
        timed(f, 8)
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(timed(a, micro_n))
        tb.append(timed(b, micro_n))
    (ma, sa), (mb, sb) = summary(ta), summary(tb)
    lines.append("%s: TrainStep replay, k = 1, seq 128, batch 32, train mode, %d blocks of %d steps, alternating: without averaging "
                 "median %.4f ms (spread %.4f) | average='ema' median %.4f ms (spread %.4f) | difference %+.4f ms = %+.2f %%"
                 % (precision, blocks, micro_n, ma, sa, mb, sb, mb - ma, 100.0 * (mb - ma) / ma))
    print(lines[-1], flush=True)
    obj_a.close(), obj_b.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--micro", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "optim_average.txt"))
    args = ap.parse_args()
    torch.manual_seed(synth.REFERENCE_SEED)
    cfg = BertConfig(30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    base = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36)
    synth.fill_module_(base)
    pool = []
    for i in range(4):
        b = synth.synthetic_batch(32, 128, 36, seed=500 + i)
        pool.append(tuple(b[k].cuda() for k in NAMES))
    lines = ["tools/optim_average_bench.py: the c2 model's arena (bert-base, 36 regions), %s, %s, torch %s, HIP %s; device events, "
             "medians over %d alternating blocks"
             % ("%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]),
                platform.platform(), torch.__version__, torch.version.hip, args.blocks)]
    for precision in ("bf16", "mixed16"):
        launches_alone(base, pool, args.blocks, precision, lines)
    for precision in ("bf16", "mixed16"):
        replay(base, pool, args.blocks, args.micro, precision, lines)
    lines.append("Not fused: icka_optim_adamw_dev holds the new p in registers when it stores it; an average kept by that launch would "
                 "read and write avg only (8 B per parameter) and save the separate launch's 4 B re-read of p and its launch.  That "
                 "would change an existing entry point and is left for a later change.  What averaging adds to a replayed step is "
                 "the averaging launch, the one-thread prepare launch and their two kernel boundaries.")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
