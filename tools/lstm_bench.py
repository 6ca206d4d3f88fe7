#!/usr/bin/env python3
"""Recurrence kernels of the BiLSTM tail (icka_lstm_fwd / icka_lstm_bwd: one persistent launch over all S steps) on their
own: microseconds per launch and per time step, as the median of ``--blocks`` timed blocks of ``--reps`` launches with the
blocks' spread (max - min): a difference smaller than the spread is not a difference.
usage: python tools/lstm_bench.py [--B 32 --S 128 --H 768] [--lengths none|full|max=N|synth|synth-sorted] [--forms all]

--lengths  none          the fixed-length entries icka_lstm_fwd / icka_lstm_bwd (the default; what every earlier figure is)
           full          the variable-length entries with every length = S
           max=N         ... with the lengths of a batch whose longest sample has N tokens (N, then N/2 .. N evenly)
           synth         ... with the lengths icka_amd/synth.py draws for a batch (U[S/4, S]), in batch order
           synth-sorted  ... the same lengths sorted descending (the second 16-row tile then has a shorter longest row)
Every form walks all S steps whatever the lengths (profiles/NEGATIVE_RESULTS.md): the lengths change the results, and these
lines show that they do not change the time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icka_amd import _lib, kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--S", type=int, default=128)
ap.add_argument("--H", type=int, default=768)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--lengths", default="none")
ap.add_argument("--forms", default="all", help="all: both hand-offs with and without the batch split; default: flags = 0 only")
ap.add_argument("--tag", default="", help="printed in front of every line (which build this is)")
args = ap.parse_args()
B, S, H = args.B, args.S, args.H
lib = _lib.load()
dev = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
torch.manual_seed(0)
gx = torch.randn(B * S, 8 * H, device=dev) * 0.5
whh = (torch.randn(8 * H, H, device=dev) * H ** -0.5).to(BF16)
y = torch.zeros(B * S, 2 * H, dtype=BF16, device=dev)
c_all = torch.zeros(B * S, 2 * H, device=dev)
act = torch.zeros(B * S, 8 * H, dtype=BF16, device=dev)
hprev = torch.zeros(B * S, 2 * H, dtype=BF16, device=dev)
dy = (torch.randn(B * S, 2 * H, device=dev) * 0.1).to(BF16)
whh_t = torch.empty(2 * H, 4 * H, dtype=BF16, device=dev)
K.transpose_bf16(whh, whh_t, 2, 4 * H, H)
dgates = torch.zeros(B * S, 8 * H, dtype=BF16, device=dev)
dcc = torch.zeros(2 * B, H, device=dev)


def lengths(spec):
    """-> (list of B lengths or None, description)"""
    if spec == "none":
        return None, "fixed-length entry"
    if spec == "full":
        return [S] * B, "lens all %d" % S
    if spec.startswith("max="):
        n = int(spec[4:])
        if not 0 <= n <= S:
            raise SystemExit("--lengths max=N needs 0 <= N <= S")
        ls = [n] + [max(min(n, 1), n // 2 + (n - n // 2) * b // max(B - 1, 1)) for b in range(1, B)]
        return ls, "lens max %d mean %.1f" % (max(ls), sum(ls) / B)
    if spec in ("synth", "synth-sorted"):
        from icka_amd import synth
        ls = synth.synthetic_batch(B, S, 49, vocab_size=512, seed=3, layout="BCHW")["lengths"].tolist()
        if spec == "synth-sorted":
            ls = sorted(ls, reverse=True)
        tiles = [max(ls[i:i + 16]) for i in range(0, B, 16)]
        return ls, "lens %s max %d mean %.1f, maxima of the 16-row tiles %s" % (spec, max(ls), sum(ls) / B, tiles)
    raise SystemExit("--lengths: none, full, max=N, synth or synth-sorted")


def timed(fn):
    """-> (median, spread) of the blocks, microseconds per launch"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / args.reps)
    return statistics.median(out), max(out) - min(out)


ls, what = lengths(args.lengths)
kw = {} if ls is None else {"lens": torch.tensor(ls, dtype=torch.int32, device=dev)}
steps = S if ls is None else max(ls)         # the longest row
forms = ((1, 1), (1, 0), (0, 1), (0, 0)) if args.forms == "all" else ((1, 1),)
for mode, split in forms:
    flags = (0 if mode else _lib.LSTM_TICKETS) | (0 if split else _lib.LSTM_NO_BATCH_SPLIT)     # per-call flags (no setters)
    tf, sf = timed(lambda: K.lstm_fwd(gx, whh, y, c_all, act, hprev, B, S, H, flags=flags, **kw))
    ysum = y.float().abs().sum().item()
    tb, sb = timed(lambda: K.lstm_bwd(dy, whh_t, act, c_all, dgates, dcc, B, S, H, flags=flags, **kw))
    gsum = dgates.float().abs().sum().item()
    # arithmetic of the recurrence alone: per step and direction h_{t-1} [B, H] x W_hh^T [H, 4H] = 2 B H 4H FLOP (backward: the
    # transposed product, the same count); the floor of a step is the hand-off of h_t between the blocks of the persistent launch
    # (one flag-in-data word round trip through L2, ~1 us idle by the microarch guide's handoff table), not this arithmetic
    fl = 2.0 * 2 * B * H * 4 * H * S
    print("%sB %d S %d H %d handoff %s split %d %s | fwd %.1f us +- %.1f (%.2f us per step of S, %.1f TFLOP/s = %.4f of the bf16 peak) "
          "| bwd %.1f us +- %.1f (%.2f us per step of S, %.1f TFLOP/s) | longest %d | checksums %.6e %.6e"
          % (args.tag + " " if args.tag else "", B, S, H, mode, split, what, tf, sf, tf / S, fl / tf * 1e-6, fl / tf * 1e-6 / 2500.0,
             tb, sb, tb / S, fl / tb * 1e-6, steps, ysum, gsum), flush=True)
