"""CPU: the float64 oracle of the CRF expectations (tests/crf_expect_oracle.py) against an enumeration of all paths, the
identities of entropy and KL, and the float32 restatement of the centred recursions of csrc/crf_expect.hip against the oracle.

The last is the guard against the cancellation the kernel's form avoids: Cov(f, r) = mu (a + b - E[r]) subtracts quantities of
size L |r|.  Errors of the float32 restatement against float64 at [2,128,13], L = 100 and 128, on normal emissions x 2 (this
test's inputs; entropy = relative mode without a second lattice | KL = relative mode against a second lattice | given mode):

    expect (|value| up to 360)  9.1e-5 | 6.9e-5 | 3.1e-5 (|value| 1)   bar 1.8e-4
    d_emissions                 4.0e-5 | 3.9e-5 | 2.5e-5               bar 7.9e-5
    d_start                     5.1e-6 | 7.6e-6 | 1.1e-5               bar 2.1e-5
    d_end                       1.7e-5 | 1.1e-5 | 1.5e-5               bar 3.4e-5
    d_trans (cells up to 12)    2.1e-4 | 2.0e-4 | 8.5e-5               bar 4.1e-4
    second lattice's gradients  e 1.6e-5, start 5.7e-6, end 1.3e-5, trans 4.8e-5: held to the bars of the first's

and the bars are 2 x the largest of each row.  The uncentred recurrences give 1e-2 .. 1.5e-1 on d_emissions there."""
import functools
import math

import pytest
import torch

import crf_constrained_oracle as CO
import crf_expect_oracle as EO
import crf_posterior_oracle as PO

F64 = torch.float64
MASKS = ["none", "prefix", "holes", "first_off"]


@functools.lru_cache(maxsize=None)
def _case(B, S, C, mask_kind):
    seed = B * 1000 + S * 10 + C + 7 * MASKS.index(mask_kind)
    p = CO.inputs(B, S, C, seed)
    return p, CO.make_mask(mask_kind, B, S, seed + 1), EO.second_lattice(B, S, C, seed + 2)


def _rows(lat, b):
    return [None if lat[0] is None else lat[0][b].double()] + [None if t is None else t.double() for t in lat[1:]]


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("mask_kind", MASKS)
def test_the_oracle_equals_the_enumeration(mask_kind, relative):
    B, S, C = 4, 6, 3
    p32, mask, q32 = _case(B, S, C, mask_kind)
    p, q = EO.leaves(*p32), EO.leaves(*q32)
    lz, ex = EO.expect(p, q, relative, mask)
    w = torch.linspace(0.5, 1.5, B, dtype=F64)
    g = EO.grads((w * ex).sum(), p + q)
    ref = [EO.enumerate_sample(None if mask is None else mask[b], _rows(p32, b), _rows(q32, b), relative) for b in range(B)]
    sgn = -1.0 if relative else 1.0
    for b, r in enumerate(ref):
        assert abs(float(lz[b].detach()) - r["log_z"]) < 1e-9 and abs(float(ex[b].detach()) - r["expect"]) < 1e-9
        want = r["cov_e"] + (r["E_e"] if relative else 0.0)
        assert (g[0][b] - w[b] * want).abs().max().item() < 1e-9
        assert (g[4][b] - sgn * w[b] * r["E_e"]).abs().max().item() < 1e-9
    for n, name in enumerate(("start", "end", "trans")):
        want = sum(w[b] * (r["cov_" + name] + (r["E_" + name] if relative else 0.0)) for b, r in enumerate(ref))
        assert (g[1 + n] - want).abs().max().item() < 1e-9, name
        assert (g[5 + n] - sgn * sum(w[b] * r["E_" + name] for b, r in enumerate(ref))).abs().max().item() < 1e-9, name
    # entropy and KL of the enumeration
    H = EO.entropy(p, mask)
    KL = EO.kl(p, q, mask)
    for b in range(B):
        mr = None if mask is None else mask[b]
        assert abs(H[b].item() - EO.enumerate_sample(mr, _rows(p32, b), [None] * 4, True)["H"]) < 1e-9
        assert abs(KL[b].item() - EO.enumerate_sample(mr, _rows(p32, b), _rows(q32, b), True)["KL"]) < 1e-9


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("B,S,C", [(4, 6, 3), (3, 20, 5)])
def test_identities(B, S, C, mask_kind):
    p32, mask, q32 = _case(B, S, C, mask_kind)
    p, q = EO.leaves(*p32), EO.leaves(*q32)
    H = EO.entropy(p, mask)
    on = EO.on_mask(mask, B, S)
    for b in range(B):
        L = int(on[b].sum())
        assert -1e-9 <= H[b].item() <= L * math.log(C) + 1e-9
    assert EO.kl(p, p, mask).abs().max().item() < 1e-9
    assert EO.kl(p, q, mask).min().item() >= -1e-9
    # a one-hot payoff at (t, j) picks the token marginal of the posterior oracle
    samples = PO.batch(p32[0], mask, *p32[1:])
    for t, j in ((0, 0), (S - 1, C - 1), (S // 2, 1)):
        g = torch.zeros(B, S, C, dtype=F64)
        g[:, t, j] = 1.0
        ex = EO.expect(p, [g, None, None, None], False, mask)[1]
        for b, s in enumerate(samples):
            assert abs(ex[b].item() - float(s.marg[t, j])) < 1e-9 or (not bool(on[b, t]) and abs(ex[b].item()) < 1e-9)


BARS = {"expect": 1.8e-4, "d_e": 7.9e-5, "d_start": 2.1e-5, "d_end": 3.4e-5, "d_trans": 4.1e-4}


@pytest.mark.parametrize("mode", ["entropy", "kl", "given"])
def test_the_centred_recursions_hold_in_float32(mode):
    B, S, C = 2, 128, 13
    p32, _, q32 = _case(B, S, C, "none")
    mask = CO.make_mask("prefix", B, S, 5)
    mask[1] = 1                       # two long samples: L = 100 and 128
    mask[0, :100] = 1
    mask[0, 100:] = 0
    relative = mode != "given"
    second = [None] * 4 if mode == "entropy" else list(q32)
    p, q = EO.leaves(*p32), EO.leaves(*second)
    lz, ex = EO.expect(p, q, relative, mask)
    w = torch.tensor([0.75, 1.25], dtype=F64)
    v = torch.tensor([-0.5, 1.5], dtype=F64)
    g = EO.grads((v * lz + w * ex).sum(), p + q)
    mine = [EO.centred_f32(p32[0][b], mask[b], *p32[1:], [None if second[0] is None else second[0][b]] + second[1:], relative,
                           v[b], w[b]) for b in range(B)]
    lz, ex = lz.detach(), ex.detach()
    err = {"expect": max(abs(m["expect"] - float(ex[b])) for b, m in enumerate(mine)),
           "log_z": max(abs(m["log_z"] - float(lz[b])) / abs(float(lz[b])) for b, m in enumerate(mine)),
           "d_e": max((m["d_e"].double() - g[0][b]).abs().max().item() for b, m in enumerate(mine))}
    for n, name in enumerate(("start", "end", "trans")):
        err["d_" + name] = (sum(m["d_" + name].double() for m in mine) - g[1 + n]).abs().max().item()
        if q[1 + n] is not None:
            err["d2_" + name] = (sum(m["d2_" + name].double() for m in mine) - g[5 + n]).abs().max().item()
    if q[0] is not None:
        err["d2_e"] = max((m["d2_e"].double() - g[4][b]).abs().max().item() for b, m in enumerate(mine))
    print(mode, "max |expect| %.1f" % ex.abs().max().item(), "max |d_trans| %.1f" % g[3].abs().max().item(),
          {k: "%.2e" % e for k, e in err.items()})
    assert err["log_z"] < 2e-5
    for k, bar in BARS.items():
        assert err[k] < bar, (k, err[k], bar)
    for k in ("d2_e", "d2_start", "d2_end", "d2_trans"):      # plain marginals times g_expect: the d_e / d_trans bars
        if k in err:
            assert err[k] < BARS[k.replace("d2", "d")], (k, err[k])
