"""Helpers of the CRF-expectation tests (no test functions): a float64 statement of the definitions of ``icka_crf_expect`` /
``icka_crf_expect_grad`` (include/icka_hip.h) that leans on autograd alone, an enumeration of all paths for tiny cases, and a
float32 restatement of the centred recursions the kernel uses.

A lattice is ``(e [B,S,C], start [C], end [C], trans [C,C])``; the chain runs over the on-positions (position 0 and every
t >= 1 with mask != 0).  ``log_z`` is a differentiable forward recursion; ``E_p[r] = d/d lambda log Z(s_p + lambda r)`` at
``lambda = 0`` is taken by autograd with ``create_graph=True``, and every gradient is autograd of that: no recurrence of the
kernel is restated on this side."""
import itertools
import math

import torch

import crf_posterior_oracle as PO

F64 = torch.float64


def on_mask(mask, B, S):
    on = torch.ones(B, S, dtype=torch.bool) if mask is None else (mask != 0)
    on = on.clone()
    on[:, 0] = True
    return on


def log_z(e, start, end, trans, mask=None):
    """log Z [B] of float64 tensors, differentiable: the forward recursion over the on-positions.  The parameters may carry
    a leading batch dimension (start, end [B,C], trans [B,C,C])."""
    B, S, C = e.shape
    on = on_mask(mask, B, S)
    st, en = (start if start.dim() == 2 else start[None, :]), (end if end.dim() == 2 else end[None, :])
    tr = trans if trans.dim() == 3 else trans[None]
    alpha = st + e[:, 0]
    for t in range(1, S):
        nxt = torch.logsumexp(alpha[:, :, None] + tr, 1) + e[:, t]
        alpha = torch.where(on[:, t, None], nxt, alpha)
    return torch.logsumexp(alpha + en, 1)


def payoff(p, second, relative):
    """the payoff lattice from p = (e, start, end, trans) and the second lattice (a part may be None = zeros)"""
    second = [torch.zeros_like(a) if g is None else g for a, g in zip(p, second)]
    return [a - g for a, g in zip(p, second)] if relative else second


def expect(p, second, relative, mask=None):
    """(log Z_p, E_p[r]) [B] each, both differentiable in every leaf of ``p`` and ``second``."""
    r = payoff(p, second, relative)
    lam = torch.zeros(p[0].shape[0], dtype=F64, requires_grad=True)
    e, st, en, tr = p
    lz = log_z(e + lam[:, None, None] * r[0], st[None] + lam[:, None] * r[1][None], en[None] + lam[:, None] * r[2][None],
               tr[None] + lam[:, None, None] * r[3][None], mask)     # a per-sample lambda on the shared parameters
    ex, = torch.autograd.grad(lz.sum(), lam, create_graph=True)
    return lz, ex


def entropy(p, mask=None):
    lz, ex = expect(p, [None] * 4, True, mask)
    return lz - ex


def kl(p, q, mask=None):
    lz, ex = expect(p, q, True, mask)
    return ex - lz + log_z(*q, mask)


def leaves(*tensors):
    """float64 leaves that require grad (None stays None)"""
    return [None if t is None else t.detach().to(F64).clone().requires_grad_(True) for t in tensors]


def grads(value, wrt):
    """d value / d each tensor of ``wrt`` (None for a None entry; zeros where the value does not depend on it)"""
    have = [t for t in wrt if t is not None]
    got = iter(torch.autograd.grad(value, have, allow_unused=True))
    out = []
    for t in wrt:
        if t is None:
            out.append(None)
        else:
            g = next(got)
            out.append(torch.zeros_like(t) if g is None else g.detach())
    return out


# ------------------------------------------------------------------------------------------------------- enumeration
def enumerate_sample(mask_row, p, second, relative):
    """All C^L paths of ONE sample (p, second: lattices whose e is [S, C]; a None part of second = zeros) -> dict with ``log_z``,
    ``expect`` = E_p[r], ``H`` = -sum p log p, ``KL`` = sum p log(p / q) with q the second lattice, the expected features
    ``E_e`` [S,C], ``E_start``, ``E_end`` [C], ``E_trans`` [C,C] and their covariances with r ``cov_*``, cell by cell."""
    e = p[0]
    S, C = e.shape
    pos = PO.on_positions(mask_row, S)
    L = len(pos)
    sec = [torch.zeros_like(a) if g is None else g for a, g in zip(p, second)]

    def score(lat, y):
        s = float(lat[1][y[0]]) + float(lat[0][pos[0], y[0]])
        for i in range(1, L):
            s += float(lat[3][y[i - 1], y[i]]) + float(lat[0][pos[i], y[i]])
        return s + float(lat[2][y[-1]])

    paths = list(itertools.product(range(C), repeat=L))
    sp = [score(p, y) for y in paths]
    sq = [score(sec, y) for y in paths]
    lse = lambda v: float(torch.logsumexp(torch.tensor(v, dtype=F64), 0))
    lzp, lzq = lse(sp), lse(sq)
    out = {"log_z": lzp, "expect": 0.0, "H": 0.0, "KL": 0.0}
    names = {"e": (S, C), "start": (C,), "end": (C,), "trans": (C, C)}
    E = {n: torch.zeros(*shape, dtype=F64) for n, shape in names.items()}
    Er = {n: torch.zeros(*shape, dtype=F64) for n, shape in names.items()}
    for y, a, b in zip(paths, sp, sq):
        pr = math.exp(a - lzp)
        r = (a - b) if relative else b
        out["expect"] += pr * r
        out["H"] -= pr * (a - lzp)
        out["KL"] += pr * ((a - lzp) - (b - lzq))
        for acc, w in ((E, pr), (Er, pr * r)):
            for i, t in enumerate(pos):
                acc["e"][t, y[i]] += w
            acc["start"][y[0]] += w
            acc["end"][y[-1]] += w
            for i in range(1, L):
                acc["trans"][y[i - 1], y[i]] += w
    for n in names:
        out["E_" + n] = E[n]
        out["cov_" + n] = Er[n] - E[n] * out["expect"]
    return out


# --------------------------------------------------------------------------------- the kernel's recursions in float32
def centred_f32(e, mask_row, start, end, trans, second, relative, g_logz, g_expect, dtype=torch.float32):
    """ONE sample through the recursions of csrc/crf_expect.hip, in ``dtype`` torch ops: alpha and beta in the log domain, the
    prefix and suffix payoffs a and b carried minus a wave-uniform offset (the filtering mean forward, the mu-weighted mean of
    a + b backward), the pair cells centred with the stored offset.  ``second``: four parts, None = zeros.  Returns a dict:
    ``log_z``, ``expect``, ``d_e`` [S,C], ``d_start``, ``d_end``, ``d_trans`` and the second lattice's ``d2_*``."""
    S, C = e.shape
    pos = PO.on_positions(mask_row, S)
    L = len(pos)
    c = lambda t: None if t is None else t.to(dtype)
    e, start, end, trans = c(e), c(start), c(end), c(trans)
    g, gs, ge, gt = [c(t) for t in second]
    pay = (lambda x, y: x - y) if relative else (lambda x, y: y)
    z1, z2 = torch.zeros(C, dtype=dtype), torch.zeros(C, C, dtype=dtype)
    R = pay(trans, z2 if gt is None else gt)
    p_st, p_en = pay(start, z1 if gs is None else gs), pay(end, z1 if ge is None else ge)
    x = [e[t] for t in pos]
    rn = [pay(e[t], z1 if g is None else g[t]) for t in pos]
    rn[0] = p_st + rn[0]
    rn[L - 1] = rn[L - 1] + p_en
    al, at, ms = [start + x[0]], [], []
    a0 = rn[0]
    m0 = (torch.softmax(al[0], 0) * a0).sum()
    at.append(a0 - m0)
    ms.append(m0)
    csum = m0
    for i in range(1, L):
        v = al[i - 1][:, None] + trans
        m = v.max(0).values
        w = torch.exp(v - m[None, :])
        s = w.sum(0)
        al.append(m + torch.log(s) + x[i])
        a = rn[i] + (w * (at[i - 1][:, None] + R)).sum(0) / s
        mi = (torch.softmax(al[i], 0) * a).sum()
        at.append(a - mi)
        ms.append(mi)
        csum = csum + mi
    v = al[L - 1] + end
    lz = torch.logsumexp(v, 0)
    mu = torch.exp(v - lz)
    out = {"log_z": float(lz), "expect": float(csum + (mu * at[L - 1]).sum() / mu.sum())}
    glz, gex = dtype_scalar(g_logz, dtype), dtype_scalar(g_expect, dtype)
    c_mu = glz + (gex if relative else 0.0)
    c_g = -gex if relative else gex
    d_e, d2_e = torch.zeros(S, C, dtype=dtype), torch.zeros(S, C, dtype=dtype)
    X, V = torch.zeros(C, C, dtype=dtype), torch.zeros(C, C, dtype=dtype)
    beta, braw = end.clone(), torch.zeros(C, dtype=dtype)
    for i in range(L - 1, -1, -1):
        lzi = torch.logsumexp(al[i] + beta, 0)      # log Z as this position sees it: the rounding common to its alphas drops out
        mu = torch.softmax(al[i] + beta, 0)
        sab = at[i] + braw
        mean = (mu * sab).sum()
        bt = braw - mean
        cov = mu * (sab - mean)
        d_e[pos[i]] = gex * cov + c_mu * mu
        d2_e[pos[i]] = c_g * mu
        if i == L - 1:
            muL, covL = mu, cov
        if i == 0:
            mu0, cov0 = mu, cov
            break
        u = x[i] + beta
        rb = rn[i] + bt
        xi = torch.exp(al[i - 1][:, None] + trans + (u - lzi)[None, :])
        X += xi
        V += xi * (at[i - 1][:, None] + R + (rb - ms[i])[None, :])
        vv = trans + u[None, :]
        mx = vv.max(1).values
        w = torch.exp(vv - mx[:, None])
        s = w.sum(1)
        beta = mx + torch.log(s)
        braw = (w * (R + rb[None, :])).sum(1) / s
    out.update({"d_e": d_e, "d_start": gex * cov0 + c_mu * mu0, "d_end": gex * covL + c_mu * muL, "d_trans": gex * V + c_mu * X,
                "d2_e": d2_e, "d2_start": c_g * mu0, "d2_end": c_g * muL, "d2_trans": c_g * X})
    return out


def dtype_scalar(v, dtype):
    return float(torch.tensor(float(v)).to(dtype))


# ---------------------------------------------------------------------------------------------------- test inputs
def second_lattice(B, S, C, seed, scale=1.0):
    """(e2, start2, end2, trans2) f32 normal draws: a payoff, or the scores of a second CRF"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, C, generator=g) * scale, torch.randn(C, generator=g) * 0.5 * scale,
            torch.randn(C, generator=g) * 0.5 * scale, torch.randn(C, C, generator=g) * 0.5 * scale)
