#!/usr/bin/env python3
"""One dev (or test) epoch of the reference's evaluation loop (My_cross_attention.py:853-917, :1052-1089) on one MI355X, two
legs on the same build, model and batches:

  baseline  what a user runs without the device scorer: ``GraphedModule(decode=True)`` -> python lists, ``loss.item()``, the
            ``.to('cpu')`` copies of the labels and the input mask (:880-881), the per-token Python loop of :882-903
            (``metrics.filter_batch``; it reads a HOST copy of the output mask -- the reference iterates the device tensor,
            one sync per token, which would only make this leg slower) and ``metrics.evaluate_lists`` at the end of the epoch;
  device    ``GraphedModule(decode="device")`` -> ``ChunkEvaluator.update`` + ``add_loss`` per batch, ONE ``compute()``.

Synthetic Twitter-shaped batches (icka_amd.synth: seq 128, 49 regions, the reference's 14-name label list = 15 tag ids);
``_gate_1`` at eval batch 1 (dev) and batch 4 (test), the published model (24 + 24 layers) at batch 1.  Both legs print
their counts, and the scorer is checked both ways on the same predictions (``same_predictions_check``).  Reported: ms per batch of an epoch of ``--batches`` batches, median of ``--blocks`` epochs with min / max,
the legs alternating.  usage: python tools/dev_loop_bench.py [--models gate_1,published] [--batches 20] [--blocks 5]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icka_amd import metrics as M  # noqa: E402
from icka_amd import synth  # noqa: E402
from icka_amd.graph import GraphedModule  # noqa: E402

NAMES = ("input_ids", "segment_ids", "input_mask", "ori_input_ids", "ori_input_mask", "ori_segment_ids",
         "added_attention_mask", "clip_features", "visual_embeds_mean", "visual_embeds_att", "offsets", "output_mask")
LMAP = M.label_list_map(M.REFERENCE_LABEL_LIST)
NL = len(LMAP)


def build(which, layers):
    from icka_amd import BertConfig
    if which == "gate_1":
        from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
        cfg = BertConfig(30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
        return MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=NL)
    from icka_amd.cross_modal import MTCCMBertForMMTokenClassificationCRF, PromptRobertaModel
    cfg = BertConfig(30522, hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096)
    cfg_r = BertConfig(50265, hidden_size=1024, num_hidden_layers=layers, num_attention_heads=16, intermediate_size=4096,
                       max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5)
    return MTCCMBertForMMTokenClassificationCRF(cfg, None, PromptRobertaModel(cfg_r), layer_num1=1, num_labels=NL)


def baseline_epoch(gm, batches, mode):
    y_pred, y_true, total, index = [], [], 0.0, 0
    for g in batches:
        a = tuple(g[k] for k in NAMES)
        if mode == "dev":
            tags, loss = gm(*a, labels=g["labels"], mode="dev")
            total += loss.item()
            index += 1
        else:
            tags = gm(*a, mode="test")
        label_ids = g["labels"].to("cpu").numpy()
        g["ori_input_mask"].to("cpu").numpy()
        mask = g["output_mask"].to("cpu").numpy()
        p, t = M.filter_batch(tags, label_ids, mask, LMAP)
        y_pred += p
        y_true += t
    sc = M.evaluate_lists(y_pred, y_true, LMAP)
    sc.mean_loss = total / index if index else None
    return sc


def device_epoch(gm, ev, batches, mode):
    ev.reset()
    for g in batches:
        a = tuple(g[k] for k in NAMES)
        if mode == "dev":
            tags, loss = gm(*a, labels=g["labels"], mode="dev")
            ev.add_loss(loss)
        else:
            tags = gm(*a, mode="test")
        ev.update(tags, g["labels"], g["output_mask"])
    return ev.compute()


def same_predictions_check(gm, ev, batches, mode):
    """The scorer on the SAME predictions both ways: one epoch of the device wrapper whose DeviceTags go to the evaluator and,
    read back, through the baseline's host loop.  (Two separate epochs of these models need not agree to the last bit: their
    losses move by an ulp between runs, and a near-tie can flip a tag.)"""
    ev.reset()
    y_pred, y_true, total, index = [], [], 0.0, 0
    for g in batches:
        a = tuple(g[k] for k in NAMES)
        if mode == "dev":
            tags, loss = gm(*a, labels=g["labels"], mode="dev")
            ev.add_loss(loss)
            total += loss.item()
            index += 1
        else:
            tags = gm(*a, mode="test")
        ev.update(tags, g["labels"], g["output_mask"])
        p, t = M.filter_batch(tags.tolist(), g["labels"].cpu().numpy(), g["output_mask"].cpu().numpy(), LMAP)
        y_pred += p
        y_true += t
    d, h = ev.compute(), M.evaluate_lists(y_pred, y_true, LMAP)
    return (d.counts == h.counts and d.per_class_counts == h.per_class_counts and tuple(d) == tuple(h)
            and d.mean_loss == (total / index if index else None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gate_1,published")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--legs", default="baseline,device")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    box = "%s (%s)" % (torch.cuda.get_device_name(dev), getattr(torch.cuda.get_device_properties(dev), "gcnArchName", "?"))
    legs = args.legs.split(",")
    for which in args.models.split(","):
        torch.manual_seed(synth.REFERENCE_SEED)
        model = build(which, args.layers).to(dev).train()
        tb = {k: v.to(dev) for k, v in synth.synthetic_prompt_batch(4, 128, num_labels=NL).items()}
        targs, tkw = tuple(tb[k] for k in NAMES), {"labels": tb["labels"], "mode": "train"}
        twin = copy.deepcopy(model)                           # one wrapper per module: the legs share nothing but the weights' values
        gms = {"baseline": GraphedModule(model, targs, tkw, decode=True, max_captures=8) if "baseline" in legs else None,
               "device": GraphedModule(twin, targs, tkw, decode="device", max_captures=8) if "device" in legs else None}
        model.eval()
        twin.eval()
        ev = M.ChunkEvaluator(LMAP, device=dev)
        for mode, bs in (("dev", 1), ("test", 4)) if which == "gate_1" else (("dev", 1),):
            batches = [{k: v.to(dev) for k, v in synth.synthetic_prompt_batch(bs, 128, num_labels=NL,
                                                                              seed=synth.REFERENCE_SEED + 100 * bs + i).items()}
                       for i in range(args.batches)]
            run = {"baseline": lambda: baseline_epoch(gms["baseline"], batches, mode),
                   "device": lambda: device_epoch(gms["device"], ev, batches, mode)}
            times, scores, seen = {n: [] for n in legs}, {}, {n: [] for n in legs}
            with torch.no_grad():
                for n in legs:
                    run[n]()                                  # captures this signature, warms up
                    run[n]()
                for _ in range(args.blocks):
                    for n in legs:                            # alternating
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        scores[n] = run[n]()
                        torch.cuda.synchronize()
                        times[n].append((time.perf_counter() - t0) * 1e3 / args.batches)
                        seen[n].append((scores[n].counts, scores[n].mean_loss))
            line = {"model": which, "pass": mode, "batch": bs, "batches_per_epoch": args.batches, "box": box}
            for n in legs:
                line[n] = {"ms_per_batch": round(statistics.median(times[n]), 3), "ms_min": round(min(times[n]), 3),
                           "ms_max": round(max(times[n]), 3), "counts": scores[n].counts, "f1": scores[n].f1,
                           "mean_loss": scores[n].mean_loss,
                           "same_in_every_block": all(x == seen[n][0] for x in seen[n]), "eager_calls_of_wrapper": gms[n].stats["eager_calls"]}
            if "device" in legs:
                with torch.no_grad():
                    line["scorer_equal_on_same_predictions"] = same_predictions_check(gms["device"], ev, batches, mode)
            if len(legs) == 2:
                b, d = scores["baseline"], scores["device"]
                line["legs_same_counts"] = b.counts == d.counts and b.per_class_counts == d.per_class_counts and b.mean_loss == d.mean_loss
                line["device_max_below_baseline_min"] = line["device"]["ms_max"] < line["baseline"]["ms_min"]
                line["device_median_not_above_baseline_max"] = line["device"]["ms_per_batch"] <= line["baseline"]["ms_max"]
            print(json.dumps(line), flush=True)
        for gm in gms.values():
            if gm is not None:
                gm.close()
        del gms, model, twin
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
