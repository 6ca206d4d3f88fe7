#!/usr/bin/env python3
"""What the attention-map recorder (icka_amd.attention_maps) costs, and how exact its maps are.  Writes profiles/attention_maps.txt.

Errors (the inputs of tests/test_attention_maps_gpu.py: the helpers of tests/attention_maps_oracle.py):
  * icka_attn_probs against the float64 softmax of the same bf16 values: maximum absolute error per shape and flag value;
  * the recorder on the fixture's ``cl`` model against the reference's own probabilities, bf16 and mixed16.
Timing at the c2 shape (MTCCMBertForMMTokenClassificationCRF cl, bert-base, B 32, S 128, 36 regions), eager calls, one process,
legs interleaved, median of ``--blocks`` blocks of ``--steps`` calls, spread = (max - min) / median over the blocks:
  * the eval forward (no_grad) without a recorder; with heads="mean" and heads="all", every module selected; with the
    cross-attention only;
  * the eager train step (forward + backward) with the recorder inactive, this tree against ``--parent DIR`` (a checkout of the
    parent commit with its library built): one fresh process per block and tree, alternating.  Without --parent the leg is
    left out and the file says so.
Reported, not gated.

    python tools/attention_maps_bench.py [--steps 20] [--blocks 5] [--parent DIR] [--out profiles/attention_maps.txt]"""
import argparse
import contextlib
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, S, R, C, VOCAB = 32, 128, 36, 13, 30522
CROSS = "txt2img_attention.layer.0.attention.self"


def build_c2():
    from icka_amd import synth
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(VOCAB, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=C, regions=R, variant="cl")
    synth.fill_module_(m)
    b = synth.synthetic_batch(B, S, R, num_labels=C, vocab_size=VOCAB, seed=5, layout="BRC")
    g = {k: v.cuda() for k, v in b.items()}
    args = (g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
            g["visual_embeds_att"])
    return m.cuda(), args, g["labels"]


def med_spread(ms):
    med = statistics.median(ms)
    return med, 100.0 * (max(ms) - min(ms)) / med


# ---- one block of eager train steps in THIS process (run once per block and tree by step_leg)
def step_block(steps):
    model, args, labels = build_c2()
    model.train()
    for _ in range(3):
        model.zero_grad()
        model(*args, labels=labels).backward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.zero_grad()
        model(*args, labels=labels).backward()
    torch.cuda.synchronize()
    print("STEP_MS %.4f" % ((time.perf_counter() - t0) / steps * 1e3), flush=True)


def step_leg(parent, steps, blocks):
    res = {"this": [], "parent": []}
    for _ in range(blocks):
        for tree, root in (("parent", parent), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-block", "--root", root, "--steps", str(steps)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("step block in %s failed (%d):\n%s" % (root, out.returncode, out.stderr[-2000:]))
            res[tree].append(float([ln for ln in out.stdout.splitlines() if ln.startswith("STEP_MS")][-1].split()[1]))
    return res


# ---- errors
def error_lines():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icka_amd
    import attention_maps_oracle as T
    lines = ["# icka_attn_probs vs float64 softmax of the same bf16 values: max abs error (B, heads, Sq, Skv)"]
    worst = 0.0
    for shape in T.KERNEL_SHAPES:
        qb, kb, add, H = T.kernel_case(*shape)
        ref = T.kernel_ref(qb, kb, add, *shape, H)
        errs = []
        for mean in (False, True):
            P, _b, _a = T.kernel_launch(qb, kb, add, *shape, H, mean)
            errs.append((P.double().cpu() - (ref.mean(dim=1) if mean else ref)).abs().max().item())
        worst = max(worst, *errs)
        lines.append("%-20s all %.3e   head_mean %.3e" % (shape, errs[0], errs[1]))
    lines.append("kernel-level maximum %.3e" % worst)
    lines.append("# recorder on the fixture's cl model vs the reference's probabilities: max abs error over the recorded modules")
    for prec in ("bf16", "mixed16"):
        model, batch, exp, names = T.build_model(prec)
        model.eval()
        for heads in ("all", "mean"):
            with torch.no_grad(), icka_amd.attention_maps(model, heads=heads) as rec:
                T.call_model(model, batch)
            e = max(float((rec[n][0].cpu() - torch.from_numpy(exp[heads + "/" + n].copy())).abs().max()) for n in names)
            lines.append("model-level %-8s heads=%-5s %.3e" % (prec, heads, e))
    return lines


# ---- eval-forward legs
def forward_legs(steps, blocks):
    import icka_amd
    model, args, _labels = build_c2()
    model.eval()
    legs = [("no recorder", None), ('heads="mean", every module', dict(heads="mean")), ('heads="all", every module', dict(heads="all")),
            ('heads="mean", cross-attention only', dict(heads="mean", select=[CROSS]))]
    res = {name: [] for name, _kw in legs}

    def run(kw, n):
        for _ in range(n):
            # a recorder per call: what a caller who reads the maps of each batch does (the maps of a call are freed with it)
            with (icka_amd.attention_maps(model, **kw) if kw is not None else contextlib.nullcontext()), torch.no_grad():
                model(*args)
        torch.cuda.synchronize()

    for _name, kw in legs:
        run(kw, 3)
    for _ in range(blocks):
        for name, kw in legs:
            t0 = time.perf_counter()
            run(kw, steps)
            res[name].append((time.perf_counter() - t0) / steps * 1e3)
    lines = ["# eval forward, eager, no_grad, c2 shape (B %d, S %d, %d regions, bert-base): ms/call  spread  vs no recorder" % (B, S, R)]
    base = statistics.median(res["no recorder"])
    for name, _kw in legs:
        med, sp = med_spread(res[name])
        lines.append("%-38s %8.3f  %5.1f%%  %+7.3f ms" % (name, med, sp, med - base))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with icka_amd/libicka_hip.so built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps.txt"))
    ap.add_argument("--step-block", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.step_block:
        step_block(a.steps)
        return
    lines = ["# tools/attention_maps_bench.py --steps %d --blocks %d  (%s)" % (a.steps, a.blocks, torch.cuda.get_device_name(0))]
    lines += error_lines()
    lines += forward_legs(a.steps, a.blocks)
    if a.parent:
        res = step_leg(os.path.abspath(a.parent), a.steps, a.blocks)
        lines.append("# eager train step (forward + backward), recorder inactive, one process per block and tree: ms/step  spread")
        for tree in ("parent", "this"):
            med, sp = med_spread(res[tree])
            lines.append("%-38s %8.3f  %5.1f%%" % (tree + " tree", med, sp))
        lines.append("this / parent = %.4f" % (statistics.median(res["this"]) / statistics.median(res["parent"])))
    else:
        lines.append("# eager train step against the parent commit: not measured (no --parent checkout given)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
