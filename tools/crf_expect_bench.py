#!/usr/bin/env python3
"""What a launch of icka_crf_expect / icka_crf_expect_grad costs next to icka_crf_llh and icka_crf_grad at the same shape, in
one process on one device.  Writes profiles/crf_expect.txt.

Seeded ``randn * 2`` emissions with a ragged prefix mask at B 32, S 128, C 13 (the c2 batch).  The expectation entries are
timed in the forms the module methods launch: the entropy's (relative mode, no second lattice), the KL's first call (relative
mode against a second lattice, both sides differentiated), the same with the first lattice detached (no covariance) and the
log Z-only call.  Device events around ``--launches`` back-to-back launches of one kernel (so a figure is the steady
launch-to-launch time, the launch gap included), legs interleaved, median over ``--blocks`` blocks, spread = (max - min) /
median.  Reported, not gated: no ratio is fixed in advance.

    python tools/crf_expect_bench.py [--launches 200] [--blocks 7] [--out profiles/crf_expect.txt]"""
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
RATIOS = (("crf_expect (entropy)", "crf_llh"), ("crf_expect_grad (entropy)", "crf_grad"),
          ("crf_expect_grad (KL, both sides)", "crf_grad"), ("crf_expect_grad (KL, first detached)", "crf_grad"))

NOTES = ["# crf_llh and crf_grad run their scaled linear-domain register form at C 13 (no transcendental on the chain); the",
         "#   expectation entries run the log-domain register form (16 exp and a log per step and sweep, as the constrained",
         "#   entries do): the 'log Z only' legs are that difference alone, one plain log-domain forward(-backward).",
         "# With a payoff the forward sweep carries a second quantity beside alpha (16 more lane reads and multiply-adds per",
         "#   step, a division, and the centring: one wave maximum and two wave sums per position); the gradient entry with the",
         "#   covariance does the same beside beta and keeps two [C,C] accumulator columns in the pair loop.  With the first",
         "#   lattice detached no covariance is computed: the 'log Z only' cost.",
         "# profiles/crf_constrained.txt: the constrained gradient (two lattices) costs 2.36 x crf_grad at this shape."]


def legs_of(B, S, C):
    from icka_amd import kernels as K
    from icka_amd.crf import CRF
    F32 = torch.float32
    g = torch.Generator().manual_seed(B * 1000 + S + C)
    e = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    e2 = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().cuda()
    gold = torch.randint(0, C, (B, S), generator=g).cuda()
    torch.manual_seed(C)
    crf, other = CRF(C, batch_first=True).cuda(), CRF(C, batch_first=True).cuda()
    P = tuple(p.detach() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
    Q = tuple(p.detach() for p in (other.start_transitions, other.end_transitions, other.transitions))
    dev = e.device
    out, ones = torch.empty(2, B, dtype=F32, device=dev), torch.ones(B, dtype=F32, device=dev)
    de, de2 = torch.empty_like(e), torch.empty_like(e)
    G = (torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, C, device=dev))
    G2 = (torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, C, device=dev))
    kl = dict(second=e2, second_start=Q[0], second_end=Q[1], second_trans=Q[2], relative=True)
    dkl = dict(kl, d_second=de2, d_second_start=G2[0], d_second_end=G2[1], d_second_trans=G2[2])
    return [("crf_llh", lambda: K.crf_llh(e, gold, mask, *P, out[0])),
            ("crf_expect (log Z only)", lambda: K.crf_expect(e, mask, *P, out[0], None, relative=True)),
            ("crf_expect (entropy)", lambda: K.crf_expect(e, mask, *P, out[0], out[1], relative=True)),
            ("crf_expect (KL)", lambda: K.crf_expect(e, mask, *P, out[0], out[1], **kl)),
            ("crf_grad", lambda: K.crf_grad(e, gold, mask, *P, ones, de, *G)),
            ("crf_expect_grad (log Z only)", lambda: K.crf_expect_grad(e, mask, *P, ones, None, de, *G, relative=True)),
            ("crf_expect_grad (entropy)", lambda: K.crf_expect_grad(e, mask, *P, ones, ones, de, *G, relative=True)),
            ("crf_expect_grad (KL, both sides)", lambda: K.crf_expect_grad(e, mask, *P, ones, ones, de, *G, **dkl)),
            ("crf_expect_grad (KL, first detached)",
             lambda: K.crf_expect_grad(e, mask, *P, ones, ones, None, None, None, None, **dkl))]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_expect.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/crf_expect_bench.py needs a ROCm device: a time taken elsewhere says nothing")
    lines = ["# tools/crf_expect_bench.py --launches %d --blocks %d  (%s)" % (a.launches, a.blocks, torch.cuda.get_device_name(0)),
             "# commit: %s" % (a.commit or commit() or "not recorded"),
             "# us per launch (device events around back-to-back launches, launch gap included): median over the blocks, spread"]
    B, S, C = SHAPE
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
        lines.append("  %-38s %8.2f us  %5.1f%%" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name]))
    for mine, theirs in RATIOS:
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
