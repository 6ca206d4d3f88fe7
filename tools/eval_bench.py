#!/usr/bin/env python3
"""Cost of the reference's dev and test passes (My_cross_attention.py:846-875 dev at ``eval_batch_size``, default 1 (:547);
:1022, :1047-1050 test at batch 4) on one MI355X, eagerly and replayed through ``GraphedModule(..., decode=True)``.

Models: the ``_gate_1`` tagger (bert-base trunk) and the published model (bert-large / roberta-large geometry, 24 + 24 layers
by default), eval mode under no_grad, synthetic Twitter-2015-shaped batches (seq 128, 49 regions, 13 labels, icka_amd.synth).
Each call returns python lists (test) or (lists, loss) (dev), so both runs end in one host sync per call, as in the reference.
Reported: ms per call and samples/s, median of ``--blocks`` blocks of ``--calls`` calls, with the min / max block.
Not the headline metric (bench.py).   usage: python tools/eval_bench.py [--eval-batch 1] [--layers 24] [--blocks 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icka_amd import BertConfig, synth  # noqa: E402
from icka_amd.graph import GraphedModule  # noqa: E402

NAMES = ("input_ids", "segment_ids", "input_mask", "ori_input_ids", "ori_input_mask", "ori_segment_ids",
         "added_attention_mask", "clip_features", "visual_embeds_mean", "visual_embeds_att", "offsets", "output_mask")


def build(which, layers):
    if which == "gate_1":
        from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
        cfg = BertConfig(30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
        return MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=13)
    from icka_amd.cross_modal import MTCCMBertForMMTokenClassificationCRF, PromptRobertaModel
    cfg = BertConfig(30522, hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096)
    cfg_r = BertConfig(50265, hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096,
                       max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5)
    return MTCCMBertForMMTokenClassificationCRF(cfg, None, PromptRobertaModel(cfg_r), layer_num1=1, num_labels=13)


def time_calls(fn, calls, blocks):
    """ms per call of each block (every call ends in its own host sync: the lists)."""
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-batch", type=int, default=1)
    ap.add_argument("--test-batch", type=int, default=4)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--models", default="gate_1,published")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    box = "%s (%s)" % (torch.cuda.get_device_name(dev), getattr(torch.cuda.get_device_properties(dev), "gcnArchName", "?"))
    for which in args.models.split(","):
        torch.manual_seed(synth.REFERENCE_SEED)
        model = build(which, args.layers).to(dev).train()
        tb = synth.synthetic_prompt_batch(4, 128, num_labels=13)
        tg = {k: v.to(dev) for k, v in tb.items()}
        targs = tuple(tg[k] for k in NAMES)
        gm = GraphedModule(model, targs, {"labels": tg["labels"], "mode": "train"}, decode=True, max_captures=8)
        model.eval()
        for mode, bs in (("dev", args.eval_batch), ("test", args.test_batch)):
            b = synth.synthetic_prompt_batch(bs, 128, num_labels=13, seed=synth.REFERENCE_SEED + bs)
            g = {k: v.to(dev) for k, v in b.items()}
            a = tuple(g[k] for k in NAMES)
            kw = {"labels": g["labels"], "mode": "dev"} if mode == "dev" else {"mode": "test"}
            res = {}
            with torch.no_grad():
                eager_out = model(*a, **kw)
                graph_out = gm(*a, **kw)              # (captures this signature)
                same = (eager_out[0] == graph_out[0]) if mode == "dev" else (eager_out == graph_out)
                for name, fn in (("eager", lambda: model(*a, **kw)), ("replayed", lambda: gm(*a, **kw))):
                    for _ in range(3):
                        fn()
                    res[name] = time_calls(fn, args.calls, args.blocks)
            line = {"model": which, "pass": mode, "batch": bs, "box": box, "same_tags": bool(same),
                    "eager_calls_of_wrapper": gm.stats["eager_calls"]}
            for name, blocks in res.items():
                med = statistics.median(blocks)
                line[name] = {"ms_per_call": round(med, 3), "ms_min": round(min(blocks), 3), "ms_max": round(max(blocks), 3),
                              "samples_per_s": round(bs * 1e3 / med, 1)}
            line["speedup"] = round(line["eager"]["ms_per_call"] / line["replayed"]["ms_per_call"], 2)
            print(json.dumps(line), flush=True)
        gm.close()
        del gm, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
