#!/usr/bin/env python3
"""What the reference's full training objective costs the c2 step (aux_losses=True: the contrastive heads, the pooler, the
contrastive + relevance losses, the negative-sample swap): gate_cl, bert-base, B = 32, S = 128, 49 regions, negative_rate 16,
temp 0.179 / temp_lamb 0.7 / lamb 0.62 (My_cross_attention.py:479-497), bf16, train mode, the step replayed as one hipGraph
(graph.GraphedStep).  Both models in one process on one box, interleaved blocks, median of 5 blocks each.  Reported, not
gated.  The kernel names come from a separate run under rocprofv3 --kernel-trace --stats (--steps 3 --blocks 1).

    python tools/objective_bench.py [--steps 30] [--blocks 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import icka_amd  # noqa: E402
from icka_amd import synth  # noqa: E402
from icka_amd.graph import GraphedStep  # noqa: E402

NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")


def build(aux):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=49, variant="gate_cl", aux_losses=aux)
    synth.fill_module_(m)
    icka_amd.set_precision(m, "bf16")
    return m.cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    b = synth.synthetic_batch(32, 128, 49, seed=1234)
    t = tuple(b[k].cuda() for k in NAMES)
    steps = {}
    for aux in (False, True):
        model = build(aux)

        def micro(*x, model=model, aux=aux):
            if aux:
                loss = model(*x[:6], 0.179, 0.7, 0.62, x[6], 16)
            else:
                loss = model(*x[:6], labels=x[6])
            loss.backward()
            return loss
        gs = GraphedStep(model, micro, inputs=t)
        steps[aux] = (model, gs)
    ms = {False: [], True: []}
    for _ in range(args.blocks):
        for aux in (False, True):
            model, gs = steps[aux]
            for _ in range(3):
                model.zero_grad()
                gs(*t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model.zero_grad()
                gs(*t)
            torch.cuda.synchronize()
            ms[aux].append(1e3 * (time.perf_counter() - t0) / args.steps)
    base, full = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps({"what": "c2 gate_cl training step (bf16, train mode, hipGraph replay), B=32 S=128 R=49, negative_rate 16",
                      "ms_aux_losses_false": round(base, 4), "ms_aux_losses_true": round(full, 4),
                      "extra_ms": round(full - base, 4), "extra_pct": round(100.0 * (full - base) / base, 2),
                      "blocks_false": [round(x, 4) for x in ms[False]], "blocks_true": [round(x, 4) for x in ms[True]],
                      "steps_per_block": args.steps}), flush=True)
    for aux in (False, True):
        steps[aux][1].close()


if __name__ == "__main__":
    main()
