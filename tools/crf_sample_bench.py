#!/usr/bin/env python3
"""What a launch of icka_crf_sample costs for num_samples = 1, 8, 64 and a launch of icka_chunk_counts for 8 path rows, next
to icka_crf_nbest (nbest 8), icka_crf_posterior (Viterbi paths, no chunks) and icka_chunk_eval at the same shape, in one
process on one device.  Writes profiles/crf_sample.txt.

Seeded ``randn * 2`` emissions at B 32, S 128, C 13 (the c2 batch) with ragged prefix masks, lengths uniform in [S / 4, S]
(icka_amd.synth's Twitter-2015-shaped batches); gold labels over the reference's 15 tag ids.  Device events around
``--launches`` back-to-back launches of one kernel (so a figure is the steady launch-to-launch time, the launch gap included),
legs interleaved, median over ``--blocks`` blocks, spread = (max - min) / median.  Reported, not gated.

    python tools/crf_sample_bench.py [--launches 200] [--blocks 7] [--out profiles/crf_sample.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
SHAPE = (32, 128, 13)
DRAWS = (1, 8, 64)
ROWS = 8


def legs_of(B, S, C):
    from icka_amd import kernels as K
    from icka_amd import metrics as M
    from icka_amd.crf import CRF, CrfPosterior, NBestPaths, SampledPaths
    g = torch.Generator().manual_seed(B * 1000 + S + C)
    e = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    lens = torch.randint(S // 4, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().cuda()
    torch.manual_seed(C)
    crf = CRF(C, batch_first=True).cuda()
    P = tuple(p.detach() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
    ev = M.ChunkEvaluator.for_label_list(M.REFERENCE_LABEL_LIST)
    ev._ensure(e.device)
    labels = torch.randint(0, min(C, len(ev.names)), (B, S), generator=g).cuda()

    nb = NBestPaths(B, S, ROWS, e.device)
    nbest = lambda: K.crf_nbest(e, mask, *P, ROWS, nb.lens, nb.n_paths, nb.scores, nb.tags)
    nbest()
    post = CrfPosterior(B, S, e.device, False)
    K.crf_score_decode(e, None, mask, *P, None, post.tags.lens, post.tags.tags_flat)
    posterior = lambda: K.crf_posterior(e, mask, *P, post.log_z, post.bad, lens=post.tags.lens, tags_flat=post.tags.tags_flat,
                                        seq_logp=post.seq_logp, token_conf=post.token_conf)
    chunk_eval = lambda: K.chunk_eval(labels, mask, ev._table, ev.counters, len(ev.types), lens=post.tags.lens,
                                      tags_flat=post.tags.tags_flat)
    counts = torch.empty(ROWS, B, 4, dtype=torch.int32, device=e.device)
    chunk_counts = lambda: K.chunk_counts(nb.lens, nb.tags, labels, mask, ev._table, counts, len(ev.types))

    def sample(k):
        out = SampledPaths(B, S, k, e.device)
        return lambda: K.crf_sample(e, mask, *P, k, 1234, None, out.lens, out.log_z, out.scores, out.tags)

    return ([("crf_sample, num_samples = %d" % k, sample(k)) for k in DRAWS]
            + [("crf_nbest, nbest = %d" % ROWS, nbest), ("crf_posterior (paths, no chunks)", posterior),
               ("chunk_counts, %d rows" % ROWS, chunk_counts), ("chunk_eval (one path per sample)", chunk_eval)])


def time_leg(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--commit", default=None, help="the commit the figures are taken at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_sample.txt"))
    a = ap.parse_args()
    B, S, C = SHAPE
    lines = ["# tools/crf_sample_bench.py --launches %d --blocks %d  (%s)" % (a.launches, a.blocks, torch.cuda.get_device_name(0)),
             "# commit: %s" % (a.commit or commit() or "not recorded"),
             "# us per launch (device events around back-to-back launches, launch gap included): median over the blocks, spread"]
    legs = legs_of(B, S, C)
    for _name, fn in legs:
        time_leg(fn, 20)                       # warm-up of every leg
    res = {name: [] for name, _fn in legs}
    for _ in range(a.blocks):
        for name, fn in legs:
            res[name].append(time_leg(fn, a.launches))
    lines.append("B %d, S %d, C %d, lengths uniform in [%d, %d]" % (B, S, C, S // 4, S))
    med = {name: statistics.median(v) for name, v in res.items()}
    for name, v in res.items():
        lines.append("  %-36s %8.2f us  %5.1f%%" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name]))
    s = {k: med["crf_sample, num_samples = %d" % k] for k in DRAWS}
    lines.append("  num_samples = 64 / num_samples = 1 = %.2f;  per draw at 64: %.2f us" % (s[64] / s[1], s[64] / 64))
    lines.append("  num_samples = 8 / crf_nbest (nbest 8) = %.2f" % (s[8] / med["crf_nbest, nbest = %d" % ROWS]))
    lines.append("  chunk_counts (%d rows) / chunk_eval = %.2f" % (ROWS, med["chunk_counts, %d rows" % ROWS] / med["chunk_eval (one path per sample)"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
