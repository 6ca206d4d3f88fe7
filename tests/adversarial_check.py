"""Helpers of the element-wise tests of the adversarial-training kernels (csrc/adversarial.hip: icka_adv_ascend,
icka_adv_init_uniform; csrc/layernorm.hip: icka_embed_fwd_adv / _h); no test functions.  For every kernel a function that takes
the very values the kernel reads and returns {output: (float64 reference, bound)}, in the style of tests/embed_check.py and on
the buffers and the comparison of tests/kernel_check.py; plus the case list and input builder that tests/test_adversarial_cpu.py
(an f32 emulation, seeded faults) and tests/test_adversarial_elements_gpu.py (the device) share.  Nothing here is a fitted
constant.

Where the bounds come from (u = U_ACC = 2^-23 per f32 operation, as tests/kernel_check.py charges it)
-----------------------------------------------------------------------------------------------------
* A sum of squares of a sample follows the reduction tree the header states: a lane adds its at most 2 * ceil(H / 512) * 8
  squares in sequence, then 6 levels inside the wave, 2 across the block's waves, 1 + 6 across the slabs: ``tree_depth``
  additions lie on the longest path from a square to the result, one more rounding for the square itself.  All terms are
  non-negative, so the sum is off by at most (depth + 1) u of ITSELF; the square root halves a relative error and rounds once:
      r_norm = ((depth + 1) / 2 + 1) u               relative error of a norm computed from exact elements.
* n_g: n_g r_norm.  sc = alpha / n_g: relative r_norm + u.  u_el = delta + sc g (two roundings, or one as an fma):
      e_u = |sc g| (r_norm + 2 u) + u (|delta| + |sc g|).
* n_u is taken from the ROUNDED u the kernel holds: | ||u~|| - ||u|| | <= ||e_u||_2, then the tree: e_nu = ||e_u||_2 + n_u r_norm.
* Projection (n_u > epsilon): factor epsilon / n_u~ with relative error e_nu / n_u + u, one product:
      e_delta = f e_u + |delta| (e_nu / n_u + 2 u).
  Where |n_u - epsilon| <= e_nu the kernel may decide either way; the two outcomes differ by |u| |1 - epsilon / n_u| <=
  |u| e_nu / min(n_u, epsilon), which is added there (FGM from delta = 0 always lands there: ||u|| = epsilon up to roundoff).
* norms[b] = (n_g, n_u or epsilon): e_ng resp. e_nu + u epsilon, stored in f32.
* A sample that does not step keeps delta BITWISE at its valid positions (``untouched``); every non-valid position is an exact
  zero (``zero``), for every sample.
* Forward: s = ((word + delta) + pos) + type -- ``kernel_check.ln_fwd_bounds`` with t_abs = |w| + |delta| + |p| + |ty|; its
  e_s = 3 u t_abs pays the three additions.  The rest is ``embed_check.fwd_refs``.
"""
import math

import torch

import adversarial_oracle as ao
import kernel_check as kc
from kernel_check import BF16, F16, F32, U_ACC, assert_within, report, stored  # noqa: F401

F64 = torch.float64

# (B, S, H) of the issue; lengths are chosen by ``ascend_inputs``
ASCEND_SHAPES = [(1, 1, 8), (3, 5, 72), (4, 37, 520), (5, 7, 2048), (2, 128, 768)]


def tree_depth(S, H):
    """additions on the longest path of one sample's sum of squares (include/icka_hip.h, REDUCTION TREE)"""
    return 2 * math.ceil(H / 512) * 8 + 6 + 2 + (1 if S > 64 * ao.SLAB_ROWS else 0) + 6


def r_norm(S, H):
    return ((tree_depth(S, H) + 1) / 2.0 + 1.0) * U_ACC


def lengths_of(B, S):
    """valid lengths per sample: S, 1, 0, then in between -- 0, 1 and S all occur as soon as B >= 3"""
    base = [S, min(1, S), 0, max(1, S // 2), max(1, S - 1)]
    return [base[i % len(base)] for i in range(B)]


def ascend_inputs(B, S, H, seed=0, zero_sample=None, inf_sample=None):
    """CPU tensors of a case: delta f32 of per-sample norm about 0.2 or less at the valid positions (inside the ball of the
    tests' epsilon = 0.7) and junk (1e3-sized values and a NaN) at the non-valid ones, grad f32 (non-zero at the non-valid
    positions too), mask int64 with the valid positions FIRST except in sample 0 of B >= 2 cases with S >= 3,
    whose valid positions are scattered.  zero_sample / inf_sample: sample indices whose gradient is all zero / holds an inf."""
    g = torch.Generator().manual_seed(1234 + 7 * B + 13 * S + H + seed)
    lens = lengths_of(B, S)
    mask = torch.zeros(B, S, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    if B >= 2 and S >= 3:
        mask[0] = 1
        mask[0, 1] = 0          # a hole: validity is the mask's, not a length
        mask[0, S - 1] = 3      # any non-zero value counts
    delta = torch.randn(B, S, H, generator=g) * (0.2 / math.sqrt(S * H))       # per-sample norm <= about 0.2
    grad = torch.randn(B, S, H, generator=g) * 0.3
    v = mask != 0
    junk = torch.randn(B, S, H, generator=g) * 1e3
    junk[..., 0] = float("nan")
    delta = torch.where(v[:, :, None], delta, junk)
    if zero_sample is not None:
        grad[zero_sample] = torch.where(v[zero_sample][:, None], torch.zeros(S, H), grad[zero_sample])
    if inf_sample is not None and bool(v[inf_sample].any()):
        t = int(torch.nonzero(v[inf_sample])[0, 0])
        grad[inf_sample, t, H // 2] = float("inf")
    return delta, grad, mask


def ascend_refs(delta, grad, mask, alpha, epsilon):
    """{"delta": (ref, bound), "norms": (ref, bound)} + "untouched" [B] (samples whose valid positions keep their bits), "zero"
    [B, S] (positions that are exact zeros), "stepped" [B] -- module docstring.  alpha / epsilon: the f32 values the kernel gets."""
    B, S, H = delta.shape
    o = ao.ascend64(delta, grad, mask, alpha, epsilon)
    v = ao.valid_of(mask)
    stepped, shrunk, n_u, u = o["stepped"], o["shrunk"], o["n_u"], o["u"]
    rn = r_norm(S, H)
    n_g = o["norms"][:, 0]
    ng1 = torch.where(stepped, n_g, torch.ones_like(n_g))
    scg = torch.where(stepped[:, None, None], (alpha / ng1)[:, None, None] * grad.to(F64), torch.zeros(B, S, H, dtype=F64))
    scg = torch.where(v[:, :, None], scg, torch.zeros_like(scg))
    d = torch.where(v[:, :, None], delta.to(F64), torch.zeros(B, S, H, dtype=F64))
    e_u = scg.abs() * (rn + 2 * U_ACC) + U_ACC * (d.abs() + scg.abs())
    e_u = torch.where(stepped[:, None, None], e_u, torch.zeros_like(e_u))
    e_nu = torch.sqrt((e_u * e_u).sum((1, 2))) + n_u * rn
    nu1 = n_u.clamp_min(1e-300)
    f = torch.where(shrunk, epsilon / nu1, torch.ones_like(n_u))
    e_d = torch.where(shrunk[:, None, None], f[:, None, None] * e_u + o["delta"].abs() * (e_nu / nu1 + 2 * U_ACC)[:, None, None], e_u)
    either = stepped & ((n_u - epsilon).abs() <= e_nu)
    e_d = e_d + torch.where(either[:, None, None], u.abs() * (e_nu / torch.minimum(nu1, torch.full_like(nu1, epsilon)))[:, None, None],
                            torch.zeros_like(e_d))
    e_ng = n_g * rn
    e_n = torch.stack([torch.where(stepped, e_ng, torch.zeros_like(e_ng)), e_nu + U_ACC * epsilon], 1)
    return {"delta": (o["delta"], stored(e_d, o["delta"], F32)), "norms": (o["norms"], stored(e_n, o["norms"], F32)),
            "untouched": ~stepped, "zero": ~v, "stepped": stepped}


def compare_ascend(out_delta, out_norms, delta_in, refs, what, verbose=False):
    """every output of one ascent against ``refs``: bounds where the sample stepped, bits where it did not, exact zeros at the
    non-valid positions, norms (n_g of a sample that did not step: 0 exactly, or not finite)"""
    od, on = out_delta.detach().cpu(), out_norms.detach().cpu()
    ref, bound = refs["delta"]
    zero = refs["zero"]
    assert not bool(od[zero].view(torch.int32).ne(0).any()), "%s: a non-valid position is not an exact zero" % what
    st = refs["stepped"]
    if bool(st.any()):
        assert_within(od[st], ref[st], bound[st], "%s delta" % what, verbose=verbose)
    for b in torch.nonzero(~st)[:, 0].tolist():
        keep = ~zero[b]
        same = od[b][keep].view(torch.int32) == delta_in[b][keep].view(torch.int32)
        assert bool(same.all()), "%s: sample %d did not step, its valid positions must keep their bits" % (what, b)
    nref, nb = refs["norms"]
    assert_within(on[:, 1], nref[:, 1], nb[:, 1], "%s norms[:, 1]" % what, verbose=verbose)
    if bool(st.any()):
        assert_within(on[st, 0], nref[st, 0], nb[st, 0], "%s norms[:, 0]" % what, verbose=verbose)
    for b in torch.nonzero(~st)[:, 0].tolist():
        x = float(on[b, 0])
        assert x == 0.0 or not math.isfinite(x), "%s: n_g of sample %d that did not step is %r" % (what, b, x)


# ------------------------------------------------------------------------------------------------ an f32 emulation
def emulate_ascend(delta, grad, mask, alpha, epsilon, fault=None):
    """The kernel's formula in torch f32 (sums in torch's order: inside the bounds like any order).  fault: None, or one of
    "norm_over_pad" (the gradient norm runs over every position), "no_projection", "pad_row_left" (one non-valid row keeps
    what it held), "unnormalised" (alpha g instead of alpha g / n_g), "drop_slab" (the last slab of 8 rows is left out of
    the gradient norm).  -> (delta f32, norms f32 [B, 2])"""
    B, S, H = delta.shape
    v = mask != 0
    a, e = torch.tensor(alpha, dtype=F32), torch.tensor(epsilon, dtype=F32)
    vg = torch.ones_like(v) if fault == "norm_over_pad" else v.clone()
    if fault == "drop_slab":
        vg[:, (S - 1) // ao.SLAB_ROWS * ao.SLAB_ROWS:] = False
    g2 = torch.where(vg[:, :, None], grad * grad, torch.zeros_like(grad))
    n_g = torch.sqrt(g2.sum((1, 2)))
    stepped = torch.isfinite(n_g) & (n_g > 0)
    sc = torch.where(stepped, a / torch.where(stepped, n_g, torch.ones_like(n_g)), torch.zeros_like(n_g))
    if fault == "unnormalised":
        sc = torch.where(stepped, a.expand_as(sc), torch.zeros_like(sc))
    gz = torch.where(stepped[:, None, None], grad, torch.zeros_like(grad))
    u = torch.where(stepped[:, None, None], delta + sc[:, None, None] * gz, delta)
    u = torch.where(v[:, :, None], u, torch.zeros_like(u))
    n_u = torch.sqrt((u * u).sum((1, 2)))
    shrink = stepped & (n_u > e)
    if fault == "no_projection":
        shrink = torch.zeros_like(shrink)
    f = torch.where(shrink, e / torch.where(shrink, n_u, torch.ones_like(n_u)), torch.ones_like(n_u))
    out = torch.where(shrink[:, None, None], u * f[:, None, None], u)
    if fault == "pad_row_left":
        bt = torch.nonzero(~v)
        assert bt.numel(), "the case has no non-valid position"
        out[bt[0, 0], bt[0, 1]] = delta[bt[0, 0], bt[0, 1]]
    return out, torch.stack([n_g, torch.where(shrink, e.expand_as(n_u), n_u)], 1)


FAULTS = ("norm_over_pad", "no_projection", "pad_row_left", "unnormalised", "drop_slab")


# ------------------------------------------------------------------------------------------------ forward
def fwd_adv_refs(lay, word, pos, typ, delta, gamma, beta, eps, m, twin=None):
    """(y, twin, xhat, rstd) of icka_embed_fwd_adv -- ``embed_check.fwd_refs`` with the perturbation added to the word row first
    (module docstring).  ``lay``: ``embed_check.embed_layout``; ``delta`` f32 [M, H]."""
    w = word.double()[lay["wi"]]
    dl = delta.double().reshape(w.shape)
    p, t = pos.double()[lay["pi"]], typ.double()[lay["ti"]]
    r = kc.ln_fwd_bounds(w.abs() + dl.abs() + p.abs() + t.abs(), ((w + dl) + p) + t, gamma, beta, eps)
    y, e_y = r["y_raw"]
    yd = y * m.double()
    e = m.double() * e_y + U_ACC * yd.abs()
    out = {"y": (yd, stored(e, yd, BF16)), "xhat": r["xhat"], "rstd": r["rstd"]}
    if twin is not None:
        out["twin"] = (yd, stored(e, yd, twin))
    return out
