"""GPU: the minimum-risk recipe on candidate paths -- CRF.path_llh against the candidates' own log-probabilities and float64,
its -inf / zero gradient at a missing rank, and the gradients of minimum_risk(path_llh, f1_cost(path_counts)) in the emissions
and the three CRF parameters against a float64 torch-autograd restatement on the CPU.

Bars (those of tests/test_crf_constrained_gpu.py, which path_llh's kernels are held to):
  a log Z or a path score    bar(x) = 2e-4 + 2e-5 |x|;  path_llh = log Z_A - log Z: bar(log Z_A) + bar(log Z)
  d_emissions                2e-3 absolute (there for upstream weights up to 1.5; here a sample's rows carry sum_r |d loss /
                             d logp_r| <= w_b <= 1.5 in all, which the test asserts)
  parameter gradients        1e-3 (max |G_A| + max |G|) + 4e-5, G_A and G the |weight|-summed path counts and expected counts"""
import math

import numpy as np
import pytest
import torch

import crf_check as CC
import crf_sample_check as SC
import path_counts_oracle as PC

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAMES = SC.BIO_NAMES


def _bar(x):
    return 2e-4 + 2e-5 * abs(x)


def _inputs(B, S, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    return {"e": torch.randn(B, S, C, generator=g) * 2.0, "mask": CC.make_masks(B, S, kind, g),
            "start": torch.randn(C, generator=g) * 0.5, "end": torch.randn(C, generator=g) * 0.5,
            "trans": torch.randn(C, C, generator=g) * 0.7, "labels": torch.randint(0, C, (B, S), generator=g)}


def _crf(inp):
    from icka_amd.crf import CRF
    crf = CRF(inp["e"].shape[2], batch_first=True).cuda()
    with torch.no_grad():
        for p, k in zip((crf.start_transitions, crf.end_transitions, crf.transitions), ("start", "end", "trans")):
            p.copy_(inp[k])
    return crf


def _exact_logp(inp, b, path):
    c = SC.chain(inp, b)
    score = sum(CC.path_terms(path, c.x, c.start, c.end, c.T))
    return score - float(c.log_z), score, float(c.log_z)


@pytest.mark.parametrize("kind", ["prefix", "holes"])
def test_path_llh_equals_the_candidates_log_probs(kind):
    B, S, C, R = 4, 9, len(NAMES), 4
    inp = _inputs(B, S, C, kind, 31 + len(kind))
    crf = _crf(inp)
    e, m = inp["e"].cuda(), inp["mask"].cuda()
    nb = crf.decode_nbest(e, m, nbest=R)
    sp = crf.sample(e, m, num_samples=R, seed=12)
    post = crf.posterior(e, nb.rank(0), m)
    for what, cand, lp in (("nbest", nb, nb.log_probs(post.log_z)), ("sampled", sp, sp.log_probs())):
        llh = crf.path_llh(e, cand, m)
        assert tuple(llh.shape) == (B, R) and llh.dtype == torch.float32
        h = cand.host()
        paths = SC.split_rows(h["lens"], h["tags"])
        worst = 0.0
        for b in range(B):
            for r in range(R):
                if what == "nbest" and r >= h["n_paths"][b]:
                    assert float(llh[b, r]) == -math.inf
                    continue
                exact, score, log_z = _exact_logp(inp, b, paths[r][b])
                bar = _bar(score) + _bar(log_z)
                worst = max(worst, abs(float(llh[b, r]) - exact) / bar)
                assert abs(float(llh[b, r]) - exact) <= bar, (what, b, r, float(llh[b, r]), exact)
                assert abs(float(llh[b, r]) - float(lp[b, r])) <= 2 * bar, (what, b, r, float(llh[b, r]), float(lp[b, r]))
        print("RISK path_llh %s %s: worst err / bar %.3f" % (kind, what, worst))
    one = crf.path_llh(e, nb.rank(1), m)
    assert tuple(one.shape) == (B, 1) and torch.equal(one[:, 0], crf.path_llh(e, nb, m)[:, 1])
    with pytest.raises(ValueError, match="paths"):
        crf.path_llh(e, [[0] * S] * B, m)


def test_missing_rank_is_minus_inf_with_zero_gradient():
    from icka_amd import metrics as M
    from icka_amd import minimum_risk
    names = ["O", "B-PER", "I-PER"]
    B, S, C, R = 5, 6, 3, 8
    inp = _inputs(B, S, C, "prefix", 3)
    inp["mask"] = (torch.arange(S)[None, :] < torch.tensor([6, 1, 3, 5, 2])[:, None]).long()
    crf = _crf(inp)
    m = inp["mask"].cuda()
    nb = crf.decode_nbest(inp["e"].cuda(), m, nbest=R)
    assert nb.n_paths.tolist()[1] == 3
    eg = inp["e"].cuda().requires_grad_(True)
    llh = crf.path_llh(eg, nb, m)
    assert bool(torch.isinf(llh[1, 3:]).all()) and bool(torch.isfinite(llh[1, :3]).all()) and bool(torch.isfinite(llh[0]).all())
    crf.zero_grad(set_to_none=True)
    llh[:, 5].sum().backward()                      # rank 5: sample 1 does not have it
    assert torch.equal(eg.grad[1].view(torch.int32), torch.zeros_like(eg.grad[1]).view(torch.int32))
    assert float(eg.grad[0].abs().sum()) > 0 and bool(torch.isfinite(eg.grad).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in crf.parameters())
    # the whole recipe stays finite, and the missing ranks carry no weight
    ev = M.ChunkEvaluator(names)
    cost = M.f1_cost(ev.path_counts(nb, inp["labels"].cuda(), m))
    eg2 = inp["e"].cuda().requires_grad_(True)
    risk = minimum_risk(crf.path_llh(eg2, nb, m), cost)
    risk.sum().backward()
    assert bool(torch.isfinite(risk).all()) and bool(torch.isfinite(eg2.grad).all())
    lp = crf.path_llh(inp["e"].cuda(), nb, m)[1, :3].double()
    q = torch.softmax(lp, 0)
    assert abs(float(risk[1]) - float((q * cost[1, :3].double()).sum())) < 1e-5


def _risk64(inp, paths, cost, w, scale):
    """sum_b w_b sum_r softmax_r(scale logp)_r cost_r in float64 with autograd -> (value, leaves e, start, end, trans)"""
    e = inp["e"].double().requires_grad_(True)
    st, en, tr = (inp[k].double().requires_grad_(True) for k in ("start", "end", "trans"))
    B, S, C = e.shape
    total = 0.0
    coef = []
    for b in range(B):
        pos = CC.PO.on_positions(inp["mask"][b], S)
        x = e[b][pos]
        al = st + x[0]
        for i in range(1, len(pos)):
            al = torch.logsumexp(al[:, None] + tr, 0) + x[i]
        log_z = torch.logsumexp(al + en, 0)
        lps = []
        for y in paths[b]:
            s = st[y[0]] + x[0, y[0]] + en[y[-1]]
            for i in range(1, len(y)):
                s = s + tr[y[i - 1], y[i]] + x[i, y[i]]
            lps.append(s - log_z)
        lp = torch.stack(lps) * scale
        q = torch.exp(lp - torch.logsumexp(lp, 0))
        risk = (q * cost[b]).sum()
        coef.append((scale * q * (cost[b] - risk)).detach() * w[b])        # d (w risk) / d logp_r
        total = total + w[b] * risk
    return total, (e, st, en, tr), coef


@pytest.mark.parametrize("kind,source", [("prefix", "nbest"), ("holes", "sampled")])
def test_risk_gradients_against_float64_autograd(kind, source):
    from icka_amd import metrics as M
    from icka_amd import minimum_risk
    B, S, C, R = 3, 6, len(NAMES), 4
    inp = _inputs(B, S, C, kind, 77)
    crf = _crf(inp)
    m = inp["mask"].cuda()
    eg = inp["e"].cuda().requires_grad_(True)
    cand = crf.decode_nbest(eg, m, nbest=R) if source == "nbest" else crf.sample(eg, m, num_samples=R, seed=4)
    # gold labels near the candidates, so that their costs differ: candidate 1 with a third of its tags redrawn, under an
    # output mask that keeps the whole path (the CRF mask may have holes: path index j is position j only before the first)
    h = cand.host()
    rows = SC.split_rows(h["lens"], h["tags"])
    g = torch.Generator().manual_seed(5)
    out_mask = (torch.arange(S)[None, :] < torch.tensor(h["lens"])[:, None]).long()
    gold = torch.zeros(B, S, dtype=torch.int64)
    for b in range(B):
        y = torch.tensor(rows[1][b])
        gold[b, :len(y)] = torch.where(torch.rand(len(y), generator=g) < 0.33, torch.randint(0, C, (len(y),), generator=g), y)
    inp = dict(inp, labels=gold, out_mask=out_mask)
    labels, om = gold.cuda(), out_mask.cuda()
    ev = M.ChunkEvaluator(NAMES)
    counts = ev.path_counts(cand, labels, om)
    cost = M.f1_cost(counts)
    w = torch.tensor([0.5, 1.0, 1.5])
    scale = 1.0
    crf.zero_grad(set_to_none=True)
    loss = (minimum_risk(crf.path_llh(eg, cand, m), cost, scale) * w.cuda()).sum()     # the three-line recipe
    loss.backward()

    paths = [[rows[r][b] for r in range(R)] for b in range(B)]
    want_counts = PC.host_counts(h["lens"], h["tags"], inp["labels"], inp["out_mask"], NAMES)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and int(want_counts[..., 3].sum()) == 0
    c64 = torch.tensor(want_counts, dtype=F64)
    n = c64[..., 1] + c64[..., 2]
    cost64 = torch.where(n > 0, 1 - 2 * c64[..., 0] / n.clamp(min=1), torch.zeros_like(n)).transpose(0, 1)
    assert torch.allclose(cost.cpu().double(), cost64, atol=1e-6) and float(cost64.max() - cost64.min()) > 0
    ref, leaves, coef = _risk64(inp, paths, cost64, w.double(), scale)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))
    absw = [float(c.abs().sum()) for c in coef]
    assert max(absw) <= float(w.max()) and max(absw) > 1e-3          # the weights are not all zero: the test says something
    err = (eg.grad.cpu().double() - leaves[0].grad).abs().amax((1, 2))
    for b in range(B):
        print("RISK %s sample %d: d_emissions err %.3e (bar 2e-3), total |weight| %.3f" % (source, b, float(err[b]), absw[b]))
        assert float(err[b]) < 2e-3, (b, float(err[b]))
    # |weight|-summed counts: of the candidate paths (G_A) and expected under the model (G)
    ga = [torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64), torch.zeros(C, C, dtype=F64)]
    gf = [torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64), torch.zeros(C, C, dtype=F64)]
    for b in range(B):
        c = SC.chain(inp, b)
        for r, y in enumerate(paths[b]):
            a = float(coef[b][r].abs())
            ga[0][y[0]] += a
            ga[1][y[-1]] += a
            for u, v in zip(y, y[1:]):
                ga[2][u, v] += a
        gf[0] += absw[b] * c.marg[0]
        gf[1] += absw[b] * c.marg[-1]
        gf[2] += absw[b] * c.pair.sum(0)
    for name, p, ref_leaf, a, f in zip(("start", "end", "trans"), (crf.start_transitions, crf.end_transitions, crf.transitions),
                                       leaves[1:], ga, gf):
        bar = 1e-3 * (float(a.abs().max()) + float(f.abs().max())) + 4e-5
        perr = float((p.grad.cpu().double() - ref_leaf.grad).abs().max())
        print("RISK %s: d_%s err %.3e (bar %.3e)" % (source, name, perr, bar))
        assert perr < bar, (name, perr, bar)
