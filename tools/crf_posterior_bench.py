#!/usr/bin/env python3
"""What a launch of icka_crf_posterior costs, next to the CRF kernels it shares its recursions with.  Writes
profiles/crf_posterior.txt.

Per shape, in one process, on seeded ``randn * 2`` emissions with a ragged prefix mask and the Viterbi paths of
icka_crf_score_decode: device events around ``--launches`` back-to-back launches of one kernel (so a figure is the steady
launch-to-launch time, the launch gap included), legs interleaved, median over ``--blocks`` blocks, spread = (max - min) / median.
Legs: icka_crf_posterior without / with the [B,S,C] marginals and without / with a label table (the chunk outputs), and at the
same shapes icka_crf_grad and icka_crf_score_decode (unchanged kernels).  Reported, not gated.

    python tools/crf_posterior_bench.py [--launches 200] [--blocks 7] [--out profiles/crf_posterior.txt]"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
F32 = torch.float32
SHAPES = [(32, 128, 13), (4, 128, 15), (32, 128, 40)]      # c2 batch; the test pass's batch; a wide tag set (LDS log-domain body)


def legs_of(B, S, C):
    from icka_amd import kernels as K, metrics
    from icka_amd.crf import CRF, CrfPosterior
    g = torch.Generator().manual_seed(B * 1000 + S + C)
    e = (torch.randn(B, S, C, generator=g) * 2.0).cuda()
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().cuda()
    torch.manual_seed(C)
    crf = CRF(C, batch_first=True).cuda()
    P = tuple(p.detach() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
    names = ["O"] + [("B-" if j % 2 else "I-") + ("PER", "LOC", "ORG", "MISC")[(j - 1) // 2 % 4] for j in range(1, C)]
    table = torch.tensor(metrics.label_table(names, "O", ())[0], dtype=torch.int32).cuda()
    post = CrfPosterior(B, S, e.device, True)
    K.crf_score_decode(e, None, mask, *P, None, post.tags.lens, post.tags.tags_flat)
    marg = torch.empty(B, S, C, dtype=F32, device="cuda")
    tags = torch.randint(0, C, (B, S), generator=g).cuda()
    gllh = torch.ones(B, device="cuda")
    de = torch.empty_like(e)
    dP = tuple(torch.zeros_like(p) for p in P)
    llh = torch.empty(B, device="cuda")

    def posterior(with_marg, with_table):
        kw = dict(label_table=table, ent=post.ent, ent_conf=post.ent_conf, n_ent=post.n_ent) if with_table else {}
        return lambda: K.crf_posterior(e, mask, *P, post.log_z, post.bad, lens=post.tags.lens, tags_flat=post.tags.tags_flat,
                                       seq_logp=post.seq_logp, token_conf=post.token_conf, marginals=marg if with_marg else None, **kw)

    return [("posterior", posterior(False, False)), ("posterior + marginals", posterior(True, False)),
            ("posterior + chunks", posterior(False, True)), ("posterior + marginals + chunks", posterior(True, True)),
            ("crf_grad", lambda: K.crf_grad(e, tags, mask, *P, gllh, de, *dP)),
            ("crf_score_decode (decode only)", lambda: K.crf_score_decode(e, None, mask, *P, None, post.tags.lens, post.tags.tags_flat)),
            ("crf_score_decode (llh + decode)", lambda: K.crf_score_decode(e, tags, mask, *P, llh, post.tags.lens, post.tags.tags_flat))]


def time_leg(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_posterior.txt"))
    a = ap.parse_args()
    lines = ["# tools/crf_posterior_bench.py --launches %d --blocks %d  (%s)" % (a.launches, a.blocks, torch.cuda.get_device_name(0)),
             "# us per launch (device events around back-to-back launches, launch gap included): median over the blocks, spread"]
    for B, S, C in SHAPES:
        legs = legs_of(B, S, C)
        for _name, fn in legs:
            time_leg(fn, 20)                       # warm-up of every leg
        res = {name: [] for name, _fn in legs}
        for _ in range(a.blocks):
            for name, fn in legs:
                res[name].append(time_leg(fn, a.launches))
        lines.append("B %d, S %d, C %d (%s body)" % (B, S, C, "scaled register" if C <= 16 else "LDS log-domain"))
        med = {name: statistics.median(v) for name, v in res.items()}
        for name, v in res.items():
            lines.append("  %-36s %8.2f us  %5.1f%%" % (name, med[name], 100.0 * (max(v) - min(v)) / med[name]))
        both = med["crf_grad"] + med["crf_score_decode (decode only)"]
        lines.append("  posterior + marginals + chunks / (crf_grad + decode) = %.2f" % (med["posterior + marginals + chunks"] / both))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
