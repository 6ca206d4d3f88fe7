#!/usr/bin/env python3
"""What a launch of icka_crf_nbest costs for nbest = 1, 2, 4, 8, next to icka_crf_score_decode (decode only, no gold tags)
at the same shape, in one process on one device.  Writes profiles/crf_nbest.txt.

Seeded ``randn * 2`` emissions with a ragged prefix mask at B 32, S 128, C 13 (the c2 batch): device events around
``--launches`` back-to-back launches of one kernel (so a figure is the steady launch-to-launch time, the launch gap
included), legs interleaved, median over ``--blocks`` blocks, spread = (max - min) / median.  Reported, not gated: the file
records the ratio of nbest = 1 to the existing decoder and of nbest = 8 to nbest = 1 (a merge that works as a merge stays
below 8).

    python tools/crf_nbest_bench.py [--launches 200] [--blocks 7] [--out profiles/crf_nbest.txt]"""
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
RANKS = (1, 2, 4, 8)
DECODE = "crf_score_decode (decode only)"


def legs_of(B, S, C):
    from icka_amd import kernels as K
    from icka_amd.crf import CRF, DeviceTags, NBestPaths
    g = torch.Generator().manual_seed(B * 1000 + S + C)
    e = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().cuda()
    torch.manual_seed(C)
    crf = CRF(C, batch_first=True).cuda()
    P = tuple(p.detach() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
    tags = DeviceTags.empty(B, S, e.device)
    legs = [(DECODE, lambda: K.crf_score_decode(e, None, mask, *P, None, tags.lens, tags.tags_flat))]

    def nbest(k):
        out = NBestPaths(B, S, k, e.device)
        return lambda: K.crf_nbest(e, mask, *P, k, out.lens, out.n_paths, out.scores, out.tags)

    return legs + [("crf_nbest, nbest = %d" % k, nbest(k)) for k in RANKS]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_nbest.txt"))
    a = ap.parse_args()
    B, S, C = SHAPE
    lines = ["# tools/crf_nbest_bench.py --launches %d --blocks %d  (%s)" % (a.launches, a.blocks, torch.cuda.get_device_name(0)),
             "# commit: %s" % (a.commit or commit() or "not recorded"),
             "# us per launch (device events around back-to-back launches, launch gap included): median over the blocks, spread"]
    legs = legs_of(B, S, C)
    for _name, fn in legs:
        time_leg(fn, 20)                       # warm-up of every leg
    res = {name: [] for name, _fn in legs}
    for _ in range(a.blocks):
        for name, fn in legs:
            res[name].append(time_leg(fn, a.launches))
    lines.append("B %d, S %d, C %d" % (B, S, C))
    med = {name: statistics.median(v) for name, v in res.items()}
    for name, v in res.items():
        lines.append("  %-36s %8.2f us  %5.1f%%" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name]))
    one, eight = med["crf_nbest, nbest = 1"], med["crf_nbest, nbest = 8"]
    lines.append("  nbest = 1 / crf_score_decode = %.2f" % (one / med[DECODE]))
    lines.append("  nbest = 8 / nbest = 1 = %.2f  (%s)" % (eight / one, "below 8: the merge works as a merge" if eight <= 8 * one
                                                          else "ABOVE 8: the merge does not work as a merge"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
