#!/usr/bin/env python3
"""What adversarial training on the word embeddings costs at the c2 shape (B 32, S 128, H 768; bert-base, 36 regions), in ONE
process:

  * the kernels alone, device events around 100 launches per block, alternating blocks: icka_adv_ascend (all three launches;
    with the projection active and inactive), icka_adv_init_uniform + icka_adv_bump, and icka_embed_fwd_adv beside
    icka_embed_fwd -- with the ascent's rate against its 3 * B * S * H * 4-byte minimum (read g, read delta, write delta) and
    against the achievable HBM bandwidth of an MI355X;
  * the TrainStep replay (bf16, train mode, k = 1): plain step against the FGM step, alternating blocks.

Prints medians and block spreads (max - min).  No time is asserted anywhere.
usage: python tools/adv_bench.py [--micro 50] [--blocks 5] [--out profiles/adversarial.txt]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o adv -- python tools/adv_bench.py --ascents 200
           (the per-launch times of the ascent: N steps with the projection active, nothing else, no file written)"""
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
B, S, H = 32, 128, 768
HBM_ACHIEVABLE = 6.3e12        # bytes / s a streaming kernel reaches on an MI355X (8 TB/s peak)


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


def kernels_alone(base, pool, blocks, lines):
    dev = "cuda"
    mask = pool[0][2]
    g = torch.Generator().manual_seed(3)
    grad = (torch.randn(B, S, H, generator=g) * 0.01).to(dev)
    delta0 = (torch.randn(B, S, H, generator=g) * 0.01).to(dev)
    delta = delta0.clone()
    norms = torch.zeros(B, 2, device=dev)
    ws = torch.zeros(K.adv_workspace_floats(B, S, H), device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    emb = icka_amd.set_precision(copy.deepcopy(base), "bf16").cuda().bert.embeddings
    ids, seg = pool[0][0], pool[0][1]
    y = torch.empty(B * S, H, dtype=torch.bfloat16, device=dev)
    yf = torch.empty(B * S, H, dtype=torch.float32, device=dev)
    xhat, rstd = torch.empty_like(y), torch.empty(B * S, device=dev)
    tables = (emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight, emb.LayerNorm.weight,
              emb.LayerNorm.bias)

    def init(_):
        K.adv_init_uniform(delta, mask, epsilon=1.0, seed=0, counter=counter)
        K.adv_bump(counter)

    legs = [
        # alpha 1e-6 keeps every sample inside the ball of radius 1e3: the third launch reads its partials and returns
        ("icka_adv_ascend, projection inactive ", lambda _: K.adv_ascend(delta, grad, mask, norms, ws, alpha=1e-6, epsilon=1e3)),
        # alpha 10 against a ball of radius 1: every sample is projected, the third launch sweeps delta once more
        ("icka_adv_ascend, projection active   ", lambda _: K.adv_ascend(delta, grad, mask, norms, ws, alpha=10.0, epsilon=1.0)),
        ("icka_adv_init_uniform + icka_adv_bump", init),
        ("icka_embed_fwd                       ", lambda _: K.embed_fwd(ids, seg, *tables, y, y_f32=yf, xhat=xhat, rstd=rstd,
                                                                        p_drop=0.1, seed=7)),
        ("icka_embed_fwd_adv                   ", lambda _: K.embed_fwd_adv(ids, seg, *tables, delta, y, y_f32=yf, xhat=xhat,
                                                                            rstd=rstd, p_drop=0.1, seed=7)),
    ]
    for _, f in legs:
        timed(f, 20)
    times = [[] for _ in legs]
    for _ in range(blocks):
        for i, (_, f) in enumerate(legs):
            times[i].append(1e3 * timed(f, 100))
    valid = int((mask != 0).sum().item())
    lines.append("kernels alone, B %d x S %d x H %d (%d of %d positions valid), 100 launches per block:" % (B, S, H, valid, B * S))
    minimum = 3 * B * S * H * 4
    for (name, _), t in zip(legs, times):
        med, spread = summary(t)
        extra = ""
        if name.startswith("icka_adv_ascend"):
            rate = minimum / (med * 1e-6)
            extra = "  %5.0f GB/s against the %.1f MB minimum = %4.1f %% of the achievable %.1f TB/s" % (
                rate / 1e9, minimum / 1e6, 100.0 * rate / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12)
        lines.append("  %s median %8.2f us (spread %6.2f)%s" % (name, med, spread, extra))
    print("\n".join(lines[-6:]), flush=True)


def ascents_only(n):
    g = torch.Generator().manual_seed(3)
    grad = (torch.randn(B, S, H, generator=g) * 0.01).cuda()
    delta = (torch.randn(B, S, H, generator=g) * 0.01).cuda()
    mask = synth.synthetic_batch(B, S, 36, seed=500)["input_mask"].cuda()
    norms = torch.zeros(B, 2, device="cuda")
    ws = torch.zeros(K.adv_workspace_floats(B, S, H), device="cuda")
    for _ in range(n):
        K.adv_ascend(delta, grad, mask, norms, ws, alpha=10.0, epsilon=1.0)
    torch.cuda.synchronize()


def replay(base, pool, blocks, micro_n, lines):
    def build(fgm):
        model = icka_amd.set_precision(copy.deepcopy(base), "bf16").cuda().train()
        adv = icka_amd.Adversary(model, epsilon=1.0, recipe="fgm") if fgm else None

        def micro(ids, seg, mask, added, vmean, vatt, labels):
            if adv is not None:
                return adv.run(lambda: model(ids, seg, mask, added, vmean, vatt, labels=labels), input_mask=mask)
            loss = model(ids, seg, mask, added, vmean, vatt, labels=labels)
            loss.backward()
            return loss

        micro(*pool[0])
        model.zero_grad()
        model._icka_arena.shadow_policy = "tracked"
        opt = ArenaAdamW(model, lr=3e-5, weight_decay=0.01, max_grad_norm=1.0, capturable=True, schedule=("linear", 100, 1000000))
        ts = icka_amd.TrainStep(model, micro, opt, inputs=pool[0], accumulate=1)
        return (lambda i: ts(*pool[i % len(pool)])), ts

    a, obj_a = build(False)
    b, obj_b = build(True)
    for f in (a, b):
        timed(f, 8)
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(timed(a, micro_n))
        tb.append(timed(b, micro_n))
    (ma, sa), (mb, sb) = summary(ta), summary(tb)
    lines.append("TrainStep replay, bf16, k = 1, seq 128, batch 32, train mode, %d blocks of %d steps, alternating: plain step median "
                 "%.4f ms (spread %.4f) | FGM step median %.4f ms (spread %.4f) | ratio %.3f (two forward + backward passes, one "
                 "ascent, one update: expected at most 2 plus the box spread)" % (blocks, micro_n, ma, sa, mb, sb, mb / ma))
    print(lines[-1], flush=True)
    obj_a.close(), obj_b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--micro", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "adversarial.txt"))
    ap.add_argument("--ascents", type=int, default=0, help="run this many ascent steps and exit (for a kernel trace)")
    args = ap.parse_args()
    if args.ascents:
        return ascents_only(args.ascents)
    torch.manual_seed(synth.REFERENCE_SEED)
    cfg = BertConfig(30522, hidden_size=H, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    base = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36)
    synth.fill_module_(base)
    pool = []
    for i in range(4):
        b = synth.synthetic_batch(B, S, 36, seed=500 + i)
        pool.append(tuple(b[k].cuda() for k in NAMES))
    lines = ["tools/adv_bench.py: the c2 shape (bert-base, 36 regions), %s, %s, torch %s, HIP %s; device events, medians over %d "
             "alternating blocks"
             % ("%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]),
                platform.platform(), torch.__version__, torch.version.hip, args.blocks)]
    kernels_alone(base, pool, args.blocks, lines)
    replay(base, pool, args.blocks, args.micro, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
