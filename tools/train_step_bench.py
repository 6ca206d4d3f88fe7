#!/usr/bin/env python3
"""The optimisation loop of the reference (My_cross_attention.py:797-844) at the c2 shape (bert-base, seq 128, 36 regions, batch
32, bf16, train mode), timed two ways in ONE process, in alternating blocks:

  (a) today's loop: GraphedStep per micro-batch + host-mode ArenaAdamW.step() + LambdaLR.step() + zero_grad() every k-th;
  (b) TrainStep: the whole accumulation cycle, capturable ArenaAdamW update included, replayed from captured graphs.

for k = 1 and k = 5, device events around >= 200 micro-batches per block, 5 blocks per leg; and the update alone: ONE
icka_optim_adamw_dev launch against the two per-group icka_optim_adamw launches, over the c2 arena.  Prints medians and block
spreads (max - min) and says plainly whether (b) is above (a) by more than the larger of the two spreads.
usage: python tools/train_step_bench.py [--micro 200] [--blocks 5] [--out profiles/train_step.txt]"""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import icka_amd  # noqa: E402
from icka_amd import kernels as K  # noqa: E402
from icka_amd import synth  # noqa: E402
from icka_amd.config import BertConfig  # noqa: E402
from icka_amd.graph import GraphedStep  # noqa: E402
from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF  # noqa: E402
from icka_amd.optim import ArenaAdamW  # noqa: E402

NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")
TOTAL_UPDATES = 1000000      # the schedule never reaches rate 0 during the measurement


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


def verdict(name_a, a, name_b, b, unit):
    (ma, sa), (mb, sb) = summary(a), summary(b)
    slack = max(sa, sb)
    word = "NOT above" if mb <= ma + slack else "ABOVE (slower)"
    return ("%s median %.4f %s (spread %.4f) | %s median %.4f %s (spread %.4f) | difference %+.4f %s = %+.2f %% -> (b) is %s (a) by "
            "more than the larger spread (%.4f)" % (name_a, ma, unit, sa, name_b, mb, unit, sb, mb - ma, unit,
                                                    100.0 * (mb - ma) / ma, word, slack))


def build(base, pool, k, capturable):
    model = copy.deepcopy(base).cuda().train()

    def micro(ids, seg, mask, added, vmean, vatt, labels):
        loss = model(ids, seg, mask, added, vmean, vatt, labels=labels) / k
        loss.backward()
        return loss

    micro(*pool[0])                                  # builds the arena
    model.zero_grad()
    model._icka_arena.shadow_policy = "tracked"
    kw = dict(lr=3e-5, weight_decay=0.01, max_grad_norm=1.0)
    if capturable:
        opt = ArenaAdamW(model, capturable=True, schedule=("linear", 100, TOTAL_UPDATES), **kw)
        ts = icka_amd.TrainStep(model, micro, opt, inputs=pool[0], accumulate=k)
        return (lambda i: ts(*pool[i % len(pool)])), ts
    opt = ArenaAdamW(model, **kw)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda s: float(s) / 100 if s < 100 else max(0.0, float(TOTAL_UPDATES - s) / (TOTAL_UPDATES - 100)))
    gs = GraphedStep(model, micro, inputs=pool[0])

    def call(i):
        gs(*pool[i % len(pool)])
        if (i + 1) % k == 0:
            opt.step()
            sched.step()
            model.zero_grad()

    return call, gs


def update_alone(base, pool, blocks, lines):
    """adamw_dev (one launch, values from the device block) against the two per-group icka_optim_adamw launches."""
    model = copy.deepcopy(base).cuda().train()
    (model(*pool[0][:6], labels=pool[0][6])).backward()
    torch.cuda.synchronize()
    A = model._icka_arena
    host = ArenaAdamW(model, lr=0.0, weight_decay=0.0)          # rate 0: repeated updates leave the weights where they are
    dev = ArenaAdamW(model, lr=0.0, weight_decay=0.0, capturable=True)
    host._bind(), host._build(A)
    dev.prepare_capture()
    K.optim_sqnorm(A.gflat, dev._norm_table, dev._partials)
    K.optim_prepare(dev._partials, dev._norm_table.shape[0], 0.0, dev._state)
    lib, sh, sh16 = K._lib.load(), A.shadow.data_ptr(), None

    def two(_):
        for group, table in zip(host.param_groups, host._tables):
            K.check(lib.icka_optim_adamw(A.flat.data_ptr(), A.gflat.data_ptr(), host._m.data_ptr(), host._v.data_ptr(), sh, sh16,
                                         table.data_ptr(), table.shape[0], None, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, K._stream()),
                    "icka_optim_adamw")

    def one(_):
        K.optim_adamw_dev(A.flat, A.gflat, dev._m, dev._v, A.shadow, None, dev._table3, dev._state)

    for f in (two, one):
        timed(f, 20)
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(1e3 * timed(two, 100))
        tb.append(1e3 * timed(one, 100))
    lines.append("update alone, %d parameters, %d chunks: " % (A.total, dev._table3.shape[0])
                 + verdict("(a) two icka_optim_adamw", ta, "(b) one icka_optim_adamw_dev", tb, "us"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--micro", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "train_step.txt"))
    args = ap.parse_args()
    torch.manual_seed(synth.REFERENCE_SEED)
    cfg = BertConfig(30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    base = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36)
    synth.fill_module_(base)
    icka_amd.set_precision(base, "bf16")
    pool = []
    for i in range(4):
        b = synth.synthetic_batch(32, 128, 36, seed=500 + i)
        pool.append(tuple(b[k].cuda() for k in NAMES))
    lines = ["tools/train_step_bench.py: c2 shape (bert-base, seq 128, 36 regions, batch 32, bf16, train mode), %s, %d blocks of %d "
             "micro-batches per leg, alternating, device events; ms per micro-batch incl. the update every k-th"
             % (torch.cuda.get_device_name(0), args.blocks, args.micro)]
    for k in (1, 5):
        n = (args.micro + k - 1) // k * k               # whole cycles
        a, obj_a = build(base, pool, k, False)
        b, obj_b = build(base, pool, k, True)
        for f in (a, b):
            timed(f, 4 * k)
        ta, tb = [], []
        for _ in range(args.blocks):
            ta.append(timed(a, n))
            tb.append(timed(b, n))
        lines.append("k = %d: " % k + verdict("(a) GraphedStep + host ArenaAdamW + LambdaLR + zero_grad", ta, "(b) TrainStep", tb, "ms"))
        lines.append("        blocks (a) %s | (b) %s" % (" ".join("%.4f" % x for x in ta), " ".join("%.4f" % x for x in tb)))
        print(lines[-2] + "\n" + lines[-1], flush=True)
        obj_a.close(), obj_b.close()
        del a, b, obj_a, obj_b
        torch.cuda.empty_cache()
    update_alone(base, pool, args.blocks, lines)
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
