#!/usr/bin/env python3
"""Packed token-budget batches (icka_amd.set_packed) against the padded batch at the c2 model: MTCCMBertForMMTokenClassificationCRF
(cl, bert-base, S = 128, 36 regions), bf16, train mode, forward + backward replayed under GraphedModule.  Padded legs draw B
samples with lengths ~ U[lo, hi]; packed legs take the batches TokenBudgetBatchSampler makes from the same length
distribution (max_tokens rows), each brought to a fixed max_batch with empty samples so one capture serves every batch.
Both legs in one process on one box, interleaved blocks, median of ``--blocks`` blocks of ``--steps`` steps each; the spread
is (max - min) / median over the blocks.  Reported, not gated.

    python tools/packed_bench.py [--steps 30] [--blocks 5] [--out FILE]"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from icka_amd import GraphedModule, TokenBudgetBatchSampler, set_packed, synth  # noqa: E402

S, R, C, VOCAB = 128, 36, 13, 30522


def build():
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(VOCAB, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=C, regions=R, variant="cl")
    synth.fill_module_(m)
    return m.cuda().train()


def batch_of(lengths, B, g):
    """[B, S] batch whose first len(lengths) samples have these lengths; the rest are empty samples (mask all zero)."""
    n = len(lengths)
    lens = torch.zeros(B, dtype=torch.long)
    lens[:n] = torch.tensor(lengths)
    mask = (torch.arange(S)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, VOCAB, (B, S), generator=g) * mask
    labels = torch.randint(1, C, (B, S), generator=g) * mask
    vis = torch.randn(B, R, 2048, generator=g)
    added = torch.cat([torch.ones(B, R, dtype=torch.long), mask], dim=1)
    args = (ids, torch.zeros_like(ids), mask, added, vis.mean(dim=1), vis)
    return tuple(a.cuda() for a in args), labels.cuda(), n, int(lens.sum())


def legs(lo, hi, B_pad, max_tokens, max_batch, nb, seed):
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(lo, hi + 1, (nb * 4 * max_batch,), generator=g).tolist()
    padded = [batch_of(pool[i * B_pad:(i + 1) * B_pad], B_pad, g) for i in range(nb)]
    sampler = TokenBudgetBatchSampler(pool, max_tokens, max_batch)
    packed = []
    for idx in sampler:
        if len(packed) == nb:
            break
        packed.append(batch_of([pool[i] for i in idx], max_batch, g))
    return padded, packed


def time_leg(gm, batches, steps):
    t0 = time.perf_counter()
    samples = tokens = 0
    for i in range(steps):
        args, labels, n, ntok = batches[i % len(batches)]
        loss = gm(*args, labels=labels)
        loss.backward()
        samples += n
        tokens += ntok
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt / steps, samples / dt, tokens / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    base = build()
    lines = ["# tools/packed_bench.py --steps %d --blocks %d  (%s)" % (a.steps, a.blocks, torch.cuda.get_device_name(0)),
             "# leg                           ms/step  spread  samples/s  tokens/s  (median of %d blocks)" % a.blocks]
    cases = [("c2 U[32,128]", 32, 128, 32, 4096, 64), ("c2 U[8,64]", 8, 64, 32, 4096, 128),
             ("c5 U[32,128]", 32, 128, 64, 8192, 128)]
    for name, lo, hi, B_pad, max_tokens, max_batch in cases:
        padded, packed = legs(lo, hi, B_pad, max_tokens, max_batch, 8, seed=lo * 1000 + hi)
        mp, mk = copy.deepcopy(base), set_packed(copy.deepcopy(base), max_tokens)
        gp = GraphedModule(mp, padded[0][0], {"labels": padded[0][1]})
        gk = GraphedModule(mk, packed[0][0], {"labels": packed[0][1]})
        res = {"padded": [], "packed": []}
        for _ in range(a.blocks):
            res["padded"].append(time_leg(gp, padded, a.steps))
            res["packed"].append(time_leg(gk, packed, a.steps))
        for leg, label in (("padded", "padded B=%d" % B_pad), ("packed", "packed T=%d (<=%d)" % (max_tokens, max_batch))):
            ms = [r[0] * 1e3 for r in res[leg]]
            med = statistics.median(ms)
            lines.append("%-14s %-19s %7.3f  %5.1f%%  %9.1f  %8.0f" % (name, label, med, 100 * (max(ms) - min(ms)) / med,
                                                                     statistics.median(r[1] for r in res[leg]),
                                                                     statistics.median(r[2] for r in res[leg])))
        sp = statistics.median(r[1] for r in res["packed"]) / statistics.median(r[1] for r in res["padded"])
        lines.append("%-14s packed / padded samples/s = %.3f  (captures: padded %d, packed %d)"
                     % (name, sp, gp.stats["captures"], gk.stats["captures"]))
        gp.close()
        gk.close()
        del mp, mk, gp, gk
        torch.cuda.empty_cache()
        print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
