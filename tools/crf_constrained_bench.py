#!/usr/bin/env python3
"""What a launch of icka_crf_constrained_llh / _grad / _decode costs next to icka_crf_llh, icka_crf_grad and
icka_crf_score_decode (decode only) at the same shape, in one process on one device.  Writes profiles/crf_constrained.txt.

Seeded ``randn * 2`` emissions with a ragged prefix mask at B 32, S 128, C 13 (the c2 batch); the allowed sets are partial
labels (about half the positions a singleton, the rest every tag).  Device events around ``--launches`` back-to-back launches
of one kernel (so a figure is the steady launch-to-launch time, the launch gap included), legs interleaved, median over
``--blocks`` blocks, spread = (max - min) / median.  Reported, not gated: the file records the ratio of every constrained entry
to its unconstrained neighbour.  Two lattices suggest a ratio near 2 for the same body; at C <= 16 the unconstrained llh / grad
run their scaled linear-domain register forms while the constrained ones run the log-domain register form, so the ratio also
holds that difference (``--wide`` adds C 17, where both sides run the log-domain LDS form).  The notes under the figures say so.

    python tools/crf_constrained_bench.py [--launches 200] [--blocks 7] [--wide] [--out profiles/crf_constrained.txt]"""
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
WIDE = (32, 128, 17)
PAIRS = (("crf_constrained_llh", "crf_llh"), ("crf_constrained_grad", "crf_grad"),
         ("crf_constrained_decode", "crf_score_decode (decode only)"))


NOTES = ["# Two lattices in one launch suggest a ratio near 2 where both sides run the same body.",
         "# C 13: the unconstrained llh / grad run the scaled linear-domain register form (no transcendental on the chain), the",
         "#   constrained ones the log-domain register form (16 exp and a log per step and lattice): 2 lattices x that difference.",
         "#   Decoding has no transcendental in either and scans one lattice: the ratio is near 1.",
         "# C 17 (--wide): every entry runs its log-domain LDS form.  grad and decode sit where two / one lattices put them; the",
         "#   llh ratio above 3 is not explained by the lattice count (the constrained body also does the bit scan for the next",
         "#   position and the -inf selects each step; not profiled further)."]


def legs_of(B, S, C):
    from icka_amd import kernels as K
    from icka_amd.crf import CRF, ConstrainedPaths, DeviceTags
    F32 = torch.float32
    g = torch.Generator().manual_seed(B * 1000 + S + C)
    e = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().cuda()
    gold = torch.randint(0, C, (B, S), generator=g)
    known = torch.rand(B, S, generator=g) < 0.5
    allowed = CRF.allowed_from_tags(torch.where(known, gold, torch.full_like(gold, -1)), C).cuda()
    gold = gold.cuda()
    torch.manual_seed(C)
    crf = CRF(C, batch_first=True).cuda()
    P = tuple(p.detach() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
    dev = e.device
    llh, gllh = torch.empty(3, B, dtype=F32, device=dev), torch.ones(B, dtype=F32, device=dev)
    de = torch.empty_like(e)
    G = (torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, C, device=dev))
    tags, paths = DeviceTags.empty(B, S, dev), ConstrainedPaths(B, S, dev)
    paths.infeasible.zero_()
    return [("crf_llh", lambda: K.crf_llh(e, gold, mask, *P, llh[0])),
            ("crf_constrained_llh", lambda: K.crf_constrained_llh(e, mask, allowed, *P, llh[0], llh[1], llh[2])),
            ("crf_grad", lambda: K.crf_grad(e, gold, mask, *P, gllh, de, *G)),
            ("crf_constrained_grad", lambda: K.crf_constrained_grad(e, mask, allowed, *P, gllh, de, *G)),
            ("crf_score_decode (decode only)", lambda: K.crf_score_decode(e, None, mask, *P, None, tags.lens, tags.tags_flat)),
            ("crf_constrained_decode", lambda: K.crf_constrained_decode(e, mask, allowed, *P, paths.tags.lens,
                                                                        paths.tags.tags_flat, paths.scores, paths.infeasible))]


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
    ap.add_argument("--wide", action="store_true", help="also time C = 17, where every entry runs its log-domain LDS form")
    ap.add_argument("--commit", default=None, help="the commit the figures are taken at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_constrained.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/crf_constrained_bench.py needs a ROCm device: a time taken elsewhere says nothing")
    lines = ["# tools/crf_constrained_bench.py --launches %d --blocks %d%s  (%s)"
             % (a.launches, a.blocks, " --wide" if a.wide else "", torch.cuda.get_device_name(0)),
             "# commit: %s" % (a.commit or commit() or "not recorded"),
             "# us per launch (device events around back-to-back launches, launch gap included): median over the blocks, spread"]
    for B, S, C in (SHAPE, WIDE) if a.wide else (SHAPE,):
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
        for mine, theirs in PAIRS:
            lines.append("  %s / %s = %.2f" % (mine, theirs, med[mine] / med[theirs]))
    lines += NOTES
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
