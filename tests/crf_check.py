"""Helpers of the element-wise CRF kernel tests (no test functions): a float64 reference of what csrc/crf.hip computes for ANY
mask, a Viterbi reference with an explicit tie rule, a restatement of the host and device dispatch, error bounds derived from
the number formats (conventions of tests/kernel_check.py; no fitted constant) and the case list.

Semantics (pytorch-crf 0.7.2 as restated in oracle/crf_oracle.py; include/icka_hip.h).  Per sample the ON positions are
position 0 and every t >= 1 with mask[t] != 0; the recursions advance on them only.  Three rules matter only when the mask
has holes: the gold transition into an on position t comes from the label at the LITERAL previous position t - 1 (on or not);
the end transition is taken at the label at INDEX sum(mask) - 1 (the raw sum: a mask with mask[0] == 0 counts one less than
there are on positions); Viterbi back-pointers are recorded at EVERY step, from the score state that step sees, and the
back-trace starts at index sum(mask) - 1 and walks the first sum(mask) - 1 of them.  Labels are clamped into [0, C - 1]
before anything reads them (``tag_at``).

Rows whose mask is ALL ZERO are left out of every case here: the oracle's ``seq_ends = -1`` wraps to the last position there,
while the kernels' ``last = 0`` is a rule of their own (path length 1, end transition at position 0) that no reference states.

Forms.  With C <= 16 and S <= 512 ("small") the likelihood and gradient kernels first try the SCALED linear-domain recursion
if S * C <= 4096 and fall back, per sample and on the device, to the LOG-domain recursion when a normaliser or zend leaves
(1e-30, 1e30) or log Z / a marginal is not finite.  ``forms`` restates that with an f32 emulation of the scaled recursion
(tests/test_crf_scaled_cpu.py); where an emulated normaliser is within a factor 2^10 of a threshold either form may run and
the larger bound applies.  Everything else (S * C > 4096, C > 16, S > 512) is log-domain.

Bounds.  u = U_ACC = 2^-23 per f32 operation.  Two REQUIREMENTS on the device functions, the allowance kernel_check already
grants attention's exp2 / log:
    EXP_REL(x) = 2^-22 + u |x|          relative error of __expf(x): the function and its argument scaling
    LOG_ABS(s) = 2^-22 (1 + |log s|)    absolute error of __logf(s)
All bounds are first order in u, WORST CASE, and grow with the number of on positions L: at L = 315 .. 512 the scaled-form
bound of a marginal is about 3e-3 relative while an f32 emulation errs by about 2e-6 (ratio 0.001).  That is why every edge
also runs at a short chain (S <= 8), where the bound is a few 1e-5 relative and within an order of magnitude of what the
kernels err by (measured ratios 0.04 .. 0.3: the table in tests/kernel_check.py); the long cases are there for the indexing
at the path boundaries.  What the bounds catch is shown by the seeded faults of tests/test_crf_check_cpu.py.  See ``lin_errors``, ``log_errors``, ``bounds`` and ``viterbi_tol`` for the derivations.
"""
import functools
import math

import numpy as np
import torch

import crf_posterior_oracle as PO
import test_crf_scaled_cpu as EM
from kernel_check import F32, TINY, U_ACC, stored
from oracle import crf_oracle as O

F64 = torch.float64
CM, MAXW, CRF_LIN_SC, CRF_MAX_SC = 16, 8, 4096, 12288          # csrc/crf.hip
NORM_LO, NORM_HI = 1e-30, 1e30                                 # crf_forward_lin's safe range of a normaliser
MARGIN = 2.0 ** 10                                             # closer than this to a threshold: either form
LOG_FLUSH = (-126 + 10) * math.log(2.0)                        # exp arguments below this may underflow f32 (same margin)
E_SHAPE = -1                                                   # ICKA_E_SHAPE

KERNELS = ("crf_llh_kernel", "crf_grad_kernel", "crf_decode_kernel", "crf_score_decode_kernel", "crf_llh_small_kernel",
           "crf_grad_small_kernel", "crf_decode_small_kernel", "crf_score_decode_small_kernel")
ENTRIES = ("llh", "grad", "decode", "score_decode")


def exp_rel(x):
    return 2.0 ** -22 + U_ACC * x.abs()


def log_abs(log_s):
    return 2.0 ** -22 * (1.0 + log_s.abs())


# --------------------------------------------------------------------------------------------------------- dispatch
def small(S, C):
    return C <= CM and S <= 64 * MAXW


def refused(entry, S, C):
    """icka_crf_grad / _decode / _score_decode return ICKA_E_SHAPE at S * C > 12288; icka_crf_llh keeps nothing per position."""
    return entry != "llh" and S * C > CRF_MAX_SC


def kernel_of(entry, S, C):
    return "crf_%s%s_kernel" % (entry, "_small" if small(S, C) else "")


def staged(S, C):
    """crf_viterbi_small keeps the emissions in LDS up to S * C = 4096 and reads them from memory beyond."""
    return small(S, C) and S * C <= CRF_LIN_SC


def forms(inp):
    """-> [(form of the likelihood kernels, form of the gradient kernel, why)] per sample, each "lin", "log" or "either".

    The give-up rule of crf_forward_lin restated: the scaled result is kept iff every normaliser (the sum of the alpha state
    before each on step t >= 1) and zend lie in (1e-30, 1e30) and log Z is finite; the gradient kernel also gives up when a
    marginal is not finite.  The emulation is f32 but not bit-exact, so a normaliser within 2^10 of a threshold, or a bhat
    within 2^10 of the f32 overflow, leaves the form open."""
    B, S, C = inp["e"].shape
    if not small(S, C):
        return [("log", "log", "kernel")] * B
    if S * C > CRF_LIN_SC:
        return [("log", "log", "size")] * B
    out = []
    for b in range(B):
        r = EM.scaled_full(inp["e"][b].numpy(), inp["tags"][b].numpy(), None if inp["mask"] is None else inp["mask"][b].numpy(),
                           inp["start"].numpy(), inp["end"].numpy(), inp["trans"].numpy())
        n = r["norms"].astype(np.float64)
        sure_out = bool(np.any(~np.isfinite(n)) or np.any(n < NORM_LO / MARGIN) or np.any(n > NORM_HI * MARGIN)
                        or (not np.isfinite(r["logz"]) and np.all(n > NORM_LO * MARGIN)))
        sure_in = bool(np.all(np.isfinite(n)) and np.all(n > NORM_LO * MARGIN) and np.all(n < NORM_HI / MARGIN)
                       and np.isfinite(r["logz"]))
        fl = "log" if sure_out else ("lin" if sure_in else "either")
        fg = fl
        if fl == "lin" and not (r["bh_max"] < 2.0 ** 118):
            fg = "log" if not r["ok"] and r["bh_max"] > 2.0 ** 138 else "either"
        out.append((fl, fg, "give-up" if fl == "log" else ""))
    return out


# -------------------------------------------------------------------------------------------------------- reference
def clamp_tags(tags, C):
    return tags.clamp(0, C - 1)


def _mask_bool(mask, B, S):
    return torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0


def reference(inp):
    """float64: llh [B] from oracle.crf_oracle.crf_llh (labels clamped first), and d_emissions / d_start / d_end / d_trans =
    the gradient of sum_b gllh[b] llh[b] by autograd through it.  Any mask except an all-zero row (see the module docstring)."""
    B, S, C = inp["e"].shape
    m = _mask_bool(inp["mask"], B, S)
    if bool((m.sum(1) == 0).any()):
        raise ValueError("a row whose mask is all zero has no reference")
    e = inp["e"].double().requires_grad_(True)
    st, en, tr = (inp[k].double().requires_grad_(True) for k in ("start", "end", "trans"))
    llh = O.crf_llh(e, clamp_tags(inp["tags"], C), None if inp["mask"] is None else m, st, en, tr)
    (llh * inp["gllh"].double()).sum().backward()
    dtr = tr.grad if tr.grad is not None else torch.zeros(C, C, dtype=F64)          # S = 1: no transition is read
    return {"llh": llh.detach(), "de": e.grad, "dstart": st.grad, "dend": en.grad, "dtrans": dtr}


class Chain(object):
    """Forward-backward of ONE sample over its on positions, float64, plain: ``pos``, ``alpha`` / ``beta`` / ``x`` [L, C],
    ``log_z``, ``marg`` [L, C], ``pair`` [L - 1, C, C] (pair[k][i, j] = P(tag i at pos[k], tag j at pos[k + 1])), and the
    kernels' own index rules ``last`` (= sum(mask) - 1) and the gold path's terms."""

    def __init__(self, e, mask_row, tags, start, end, trans):
        S, C = e.shape
        self.S, self.C = S, C
        self.pos = PO.on_positions(mask_row, S)
        L = self.L = len(self.pos)
        raw = S if mask_row is None else int((mask_row != 0).sum())
        self.last = raw - 1 if raw > 0 else 0
        self.y = clamp_tags(tags, C).tolist()
        self.x = x = e.double()[self.pos]
        self.start, self.end, self.T = start.double(), end.double(), trans.double()
        T = self.T
        al = [self.start + x[0]]
        for k in range(1, L):
            al.append(torch.logsumexp(al[k - 1][:, None] + T, 0) + x[k])
        be = [None] * L
        be[L - 1] = self.end
        for k in range(L - 1, 0, -1):
            be[k - 1] = torch.logsumexp(T + (x[k] + be[k])[None, :], 1)
        self.alpha, self.beta = torch.stack(al), torch.stack(be)
        self.log_z = torch.logsumexp(al[L - 1] + self.end, 0)
        self.marg = torch.exp(self.alpha + self.beta - self.log_z)
        if L > 1:
            self.pair = torch.exp(self.alpha[:-1, :, None] + T[None] + (x[1:] + self.beta[1:])[:, None, :] - self.log_z)
        else:
            self.pair = torch.zeros(0, C, C, dtype=F64)
        # the gold path by the kernels' rules: its terms (for the roundoff of their f32 sum) and its counts
        y = self.y
        self.gold_terms = [float(self.start[y[0]]), float(x[0][y[0]])]
        self.gold_T = torch.zeros(C, C, dtype=F64)
        for k in range(1, L):
            t = self.pos[k]
            self.gold_terms += [float(T[y[t - 1], y[t]]), float(x[k][y[t]])]
            self.gold_T[y[t - 1], y[t]] += 1
        self.gold_terms.append(float(self.end[y[self.last]]))
        self.num = sum(self.gold_terms)


def chains(inp):
    B, S, C = inp["e"].shape
    return [Chain(inp["e"][b], None if inp["mask"] is None else inp["mask"][b], inp["tags"][b], inp["start"], inp["end"],
                  inp["trans"]) for b in range(B)]


def reference_from_chains(inp, ch):
    """The same five quantities without autograd: 1[y] - marginal at on positions (the token marginals), gold counts minus
    pair marginals, times gllh.  tests/test_crf_check_cpu.py asserts that this, ``reference`` and crf_posterior_oracle.Sample agree."""
    B, S, C = inp["e"].shape
    g = inp["gllh"].double()
    out = {"llh": torch.zeros(B, dtype=F64), "de": torch.zeros(B, S, C, dtype=F64), "dstart": torch.zeros(C, dtype=F64),
           "dend": torch.zeros(C, dtype=F64), "dtrans": torch.zeros(C, C, dtype=F64)}
    for b, c in enumerate(ch):
        out["llh"][b] = c.num - c.log_z
        for k, t in enumerate(c.pos):
            out["de"][b, t] = -g[b] * c.marg[k]
            out["de"][b, t, c.y[t]] += g[b]
        out["dstart"] += -g[b] * c.marg[0]
        out["dstart"][c.y[0]] += g[b]
        out["dend"] += -g[b] * c.marg[-1]
        out["dend"][c.y[c.last]] += g[b]
        out["dtrans"] += g[b] * (c.gold_T - c.pair.sum(0))
    return out


# ----------------------------------------------------------------------------------------------------------- bounds
def lin_errors(c, norms_log):
    """Scaled form -> (e_marg [L, C], e_pair [C, C], e_logz): absolute errors of the marginals, of sum_k pair[k] and of log Z.

    Every quantity of the scaled recursion is a sum of products of non-negative numbers, so relative errors ADD along a
    product and never grow in a sum.  With E = exp(trans - max trans), x_t = exp(e_t - max_j e_t), c_t the normaliser:
      r_E   = EXP_REL + u |trans - max|   (the subtraction is one more rounding of the argument), worst entry of E;
      r_x,t = likewise for row t of the emissions; r_S, r_End for exp(start - max), exp(end - max).
      forward on step   a_t = dot(a_{t-1}, E) * (x_t * (1 / c_t)),  c_t = sum16(a_{t-1}):
                        (C + 2) u the dot product (16 fmas in four chains and three adds: never more than C + 2 roundings of
                        live terms), 4 u the row sum, 3 u the reciprocal and the two products:  F_t = (C + 9) u + r_E + r_x,t
      backward on step  u_t = (x_t * (1 / c_t)) * bhat_t, bhat_{t-1} = dot(u_t, E row):  B_t = (C + 5) u + r_E + r_x,t
      Z = zend prod c_t carries every forward step, the start term r_S + r_x,0 + u and the end term r_End + 5 u (product and
      row sum); the c_t themselves CANCEL between the forward, the backward (which reuses the stored c_t) and log Z, whatever
      their rounded values are.
      marginal at the k-th on position = a_k bhat_k (alpha_k, beta_k and Z each with the steps they went through):
                        rho_k = F_all + F_(<= k) + B_(> k) + 2 (r_S + r_x,0 + u) + 2 (r_End + 5 u) + 2 u, taken as expm1(rho_k);
                        a pair marginal at step k needs no more (its own E, x and fma are part of F_k).
      log Z = mS + sum (max_j e_t + max trans) + sum log c_t + mEnd + log zend:  rho_Z, LOG_ABS of every logarithm, and
      (2 L + 8) u times the sum of the absolute terms (the running sum, the wave sum of the static part).
    Underflow: a factor below 2^-116 (2^10 above the smallest normal number; the same margin as for the thresholds) may be
    flushed to zero, and the paths through it are then lost.  The factors, from the float64 chain: at a node (t, j) x_t[j],
    a_t[j] = exp(alpha_t[j] - lse(alpha_{t-1}) - max trans - max_j e_t), bhat_t[j] = marginal / a_t[j], x_t[j] / c_t and
    u_t[j] = x_t[j] bhat_t[j] / c_t; on an edge (t; i, j) E[i][j], a_{t-1}[i] E[i][j] and E[i][j] u_t[j].  The lost paths
    weigh at most the marginal of that node, or the pair marginal of that edge; twice their sum K (numerator and Z) is added
    to every marginal of the sample and to log Z.  With plain parameters nothing is that small and K = 0."""
    L, C, u = c.L, c.C, U_ACC
    dT = c.T - c.T.max()
    liveT = dT > LOG_FLUSH
    r_E = float(exp_rel(dT[liveT]).max() + u * dT[liveT].abs().max())
    dx = c.x - c.x.max(1, keepdim=True).values
    livex = dx > LOG_FLUSH
    adx = torch.where(livex, dx.abs(), torch.zeros_like(dx)).amax(1)
    r_x = 2.0 ** -22 + 2 * u * adx
    ds, dn = c.start - c.start.max(), c.end - c.end.max()
    if float(ds.min()) < LOG_FLUSH or float(dn.min()) < LOG_FLUSH:
        raise ValueError("start / end spreads that underflow f32 are not covered by the scaled-form bound")
    lse_al = torch.logsumexp(c.alpha, 1)
    mx = c.x.max(1).values
    log_a = c.alpha - mx[:, None] - torch.cat((c.start.max().reshape(1), lse_al[:-1] + c.T.max()))[:, None]
    log_c = torch.logsumexp(log_a, 1)                   # log_c[k]: the normaliser of on step k + 1
    log_bh = (c.alpha + c.beta - c.log_z) - log_a
    node = torch.minimum(torch.minimum(dx, log_a), log_bh)
    K = 0.0
    if L > 1:
        log_xs = dx[1:] - log_c[:-1, None]
        log_u = log_xs + log_bh[1:]
        node[1:] = torch.minimum(node[1:], torch.minimum(log_xs, log_u))
        edge = torch.minimum(dT[None] + torch.zeros(L - 1, 1, 1, dtype=F64),
                             torch.minimum(log_a[:-1, :, None] + dT[None], dT[None] + log_u[:, None, :]))
        K += 2.0 * float(c.pair[edge < LOG_FLUSH].sum())
    K += 2.0 * float(c.marg[node < LOG_FLUSH].sum())
    r_S = 2.0 ** -22 + 2 * u * float(ds.abs().max())
    r_End = 2.0 ** -22 + 2 * u * float(dn.abs().max())
    F = (C + 9) * u + r_E + r_x[1:]
    Bk = (C + 5) * u + r_E + r_x[1:]
    zero = torch.zeros(1, dtype=F64)
    Fcum = torch.cat((zero, torch.cumsum(F, 0)))                                     # steps 1 .. k
    Bcum = torch.cat((torch.flip(torch.cumsum(torch.flip(Bk, [0]), 0), [0]), zero))    # steps k + 1 .. L - 1
    ends = (r_S + float(r_x[0]) + u) + (r_End + 5 * u)
    rho = torch.expm1(Fcum[-1] + Fcum + Bcum + 2 * ends + 2 * u)
    e_marg = rho[:, None] * c.marg + K
    e_pair = (rho[1:, None, None] * c.pair).sum(0) + (L - 1) * K
    logs = torch.as_tensor(norms_log, dtype=F64)
    A = (abs(float(c.start.max())) + float(c.x.max(1).values.abs().sum()) + (L - 1) * abs(float(c.T.max()))
         + float(logs.abs().sum()) + abs(float(c.end.max())))
    e_logz = float(Fcum[-1]) + ends + float(log_abs(logs).sum()) + (2 * L + 8) * u * A + K
    return e_marg, e_pair, e_logz


def log_errors(c):
    """Log-domain form (crf_grad_small_log, crf_llh_small_log, and the LDS kernels for C > 16 or S > 512: the same arithmetic)
    -> (e_marg, e_pair, e_logz) as ``lin_errors``.

    The error of alpha / beta is ABSOLUTE and additive per step.  One step alpha_t[j] = lse_i(alpha_{t-1}[i] + T[i][j]) + e_t[j]:
      v_i = alpha_i + T_ij            u |v_i| each; a log-sum-exp moves by at most the w-weighted mean of what its arguments move
                                      (w = softmax(v): its gradient), so the inherited error and u |v_i| enter weighted by w --
                                      a forbidden (-1e4) argument has no weight and costs nothing;
      lse = m + log(sum exp(v - m))   LSE_C = [EXP_REL(0) + (2 C / e) u] + (C + 6) u + LOG_ABS(log C): the exp allowance, whose
                                      |v - m| part (argument rounding and scaling: 2 u |d| exp(-d) <= 2 u / e per term, at most
                                      C terms of a sum >= 1), the C-term sum (six more levels for a wave sum), the log of a
                                      sum <= C; then u |lse| for the add of m and u |alpha_t| for the add of e_t.
    beta likewise with u_t = e_t + beta_t (u |u_t|).  log Z is one more log-sum-exp of alpha_last + end.
      marginal = exp((alpha + beta) - log Z): its argument is off by d_alpha + d_beta + d_logZ + u (|alpha + beta| + |arg|), so
      its relative error is expm1 of that, times (1 + EXP_REL(arg)) plus EXP_REL(arg); a pair marginal
      exp(((alpha_{t-1}[i] + T) + u_t[j]) - log Z) likewise with three roundings."""
    L, C, u = c.L, c.C, U_ACC
    lseC = 2.0 ** -22 + (2 * C / math.e) * u + (C + 6) * u + 2.0 ** -22 * (1.0 + math.log(C))
    T, al, be, x = c.T, c.alpha, c.beta, c.x
    da = [u * al[0].abs()]
    for k in range(1, L):
        v = al[k - 1][:, None] + T
        w = torch.softmax(v, 0)
        lse = torch.logsumexp(v, 0)
        da.append((w * (da[-1][:, None] + u * v.abs())).sum(0) + lseC + u * lse.abs() + u * al[k].abs())
    v = al[L - 1] + c.end
    w = torch.softmax(v, 0)
    dz = float((w * (da[-1] + u * v.abs())).sum() + lseC + u * c.log_z.abs())

    def rel(darg, arg):
        er = exp_rel(arg)
        return torch.expm1(darg) * (1 + er) + er

    e_marg = torch.zeros(L, C, dtype=F64)
    e_pair = torch.zeros(C, C, dtype=F64)
    db = torch.zeros(C, dtype=F64)
    for k in range(L - 1, -1, -1):
        s = al[k] + be[k]
        arg = s - c.log_z
        e_marg[k] = rel(da[k] + db + dz + u * (s.abs() + arg.abs()), arg) * c.marg[k]
        if k == 0:
            break
        uu = x[k] + be[k]
        du = db + u * uu.abs()
        a1 = al[k - 1][:, None] + T
        a2 = a1 + uu[None, :]
        arg = a2 - c.log_z
        rp = rel(da[k - 1][:, None] + du[None, :] + dz + u * (a1.abs() + a2.abs() + arg.abs()), arg)
        e_pair += torch.where(c.pair[k - 1] > 0, rp * c.pair[k - 1], torch.zeros_like(rp))
        v = T + uu[None, :]
        w = torch.softmax(v, 1)
        db = (w * (du[None, :] + u * v.abs())).sum(1) + lseC + u * be[k - 1].abs()
    return e_marg, e_pair, dz


def bounds(inp, ch=None, ref=None, init=None, force=None):
    """-> {"llh" [B], "de" [B, S, C], "dstart" [C], "dend" [C], "dtrans" [C, C]}: the bound of every element, the form chosen per
    sample by ``forms`` ("either": the larger), and "forms".  ``init``: what d_start / d_end / d_trans held before the call;
    ``force`` ("lin" / "log"): the bound of that form for every sample instead (the CPU suite holds each emulation to its own).

      de      = g (1[y] - marg): |g| (e_marg + 2^-126: a marginal below the smallest normal number may be flushed before g
                multiplies it), one rounding of the difference and one of the product (``stored``); exact zero at off positions.
      d_start / d_end / d_trans: the sum over the samples of |g| times the per-term errors, plus (N + 4) u sum |terms| over the
                N terms that are added -- in a register per sample, then atomically per entry; the gold + 1 terms and the
                initial content included -- plus the rounding of the stored sum.
      llh     = num - log Z: (2 L + 2) u sum |gold terms| for the strided f32 sum of the 2 L + 1 gold terms, the log Z error,
                and u (|num| + |log Z|)."""
    B, S, C = inp["e"].shape
    u = U_ACC
    ch = chains(inp) if ch is None else ch
    ref = reference_from_chains(inp, ch) if ref is None else ref
    fm = forms(inp) if force is None else [(f, f, "forced") for f in ([force] * B if isinstance(force, str) else force)]
    g = inp["gllh"].double().abs()
    init = init or {}
    out = {"llh": torch.zeros(B, dtype=F64), "de": torch.zeros(B, S, C, dtype=F64), "forms": fm}
    acc = {k: torch.zeros_like(ref[k]) for k in ("dstart", "dend", "dtrans")}
    mag = {k: (init[k].double().abs() if k in init else torch.zeros_like(ref[k])) for k in acc}
    n_terms = {"dstart": 2 * B, "dend": 2 * B, "dtrans": sum(2 * (c.L - 1) for c in ch) + B}
    for b, c in enumerate(ch):
        per_l, per_g = [], []
        want = {fm[b][0], fm[b][1]}
        res = {}
        if want & {"lin", "either"}:
            r = EM.scaled_full(inp["e"][b].numpy(), inp["tags"][b].numpy(), None if inp["mask"] is None else inp["mask"][b].numpy(),
                               inp["start"].numpy(), inp["end"].numpy(), inp["trans"].numpy())
            res["lin"] = lin_errors(c, np.log(np.clip(r["norms"].astype(np.float64), 1e-300, None)))
        if want & {"log", "either"}:
            res["log"] = log_errors(c)
        pick = lambda f, i: res[f][i] if f != "either" else torch.maximum(torch.as_tensor(res["lin"][i]), torch.as_tensor(res["log"][i]))
        e_logz = float(pick(fm[b][0], 2))
        e_marg, e_pair = pick(fm[b][1], 0), pick(fm[b][1], 1)
        gold_abs = sum(abs(t) for t in c.gold_terms)
        e_llh = (2 * c.L + 2) * u * gold_abs + e_logz + u * (abs(c.num) + abs(float(c.log_z)))
        out["llh"][b] = stored(torch.tensor(e_llh, dtype=F64), ref["llh"][b], F32)
        for k, t in enumerate(c.pos):
            onehot = torch.zeros(C, dtype=F64)
            onehot[c.y[t]] = 1
            out["de"][b, t] = stored(g[b] * (e_marg[k] + TINY[F32] + u * (onehot - c.marg[k]).abs()), ref["de"][b, t], F32)
        oh0, ohl = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
        oh0[c.y[0]] = 1
        ohl[c.y[c.last]] = 1
        acc["dstart"] += g[b] * (e_marg[0] + TINY[F32])
        acc["dend"] += g[b] * (e_marg[-1] + TINY[F32])
        acc["dtrans"] += g[b] * (e_pair + (c.L - 1) * TINY[F32])
        mag["dstart"] = mag["dstart"] + g[b] * (c.marg[0] + oh0)
        mag["dend"] = mag["dend"] + g[b] * (c.marg[-1] + ohl)
        mag["dtrans"] = mag["dtrans"] + g[b] * (c.pair.sum(0) + c.gold_T)
    for k in acc:
        out[k] = acc[k] + (n_terms[k] + 4) * u * mag[k]
    return out


# ---------------------------------------------------------------------------------------------------------- Viterbi
def viterbi_ref(e, mask_row, start, end, trans):
    """The package's Viterbi by plain loops in float64, ties to the SMALLEST index (back-pointer and final tag).
    -> (path of max(sum(mask), 1) tags, its final score, states: the score vector after every step, fin: final scores + end,
    bp).  Back-pointers are recorded at every step t >= 1 from the state that step sees, whether t is on or not."""
    S, C = e.shape
    E, st, en, T = e.double().tolist(), start.double().tolist(), end.double().tolist(), trans.double().tolist()
    on, last = EM.mask_rules(None if mask_row is None else mask_row.numpy(), S)
    score = [st[j] + E[0][j] for j in range(C)]
    states, bp = [score], [None]
    for t in range(1, S):
        new, arg = [], []
        for j in range(C):
            best, am = -math.inf, 0
            for i in range(C):
                v = score[i] + T[i][j]
                if v > best:
                    best, am = v, i
            new.append(best + E[t][j])
            arg.append(am)
        bp.append(arg)
        if on[t]:
            score = new
        states.append(score)
    fin = [score[j] + en[j] for j in range(C)]
    bt = 0
    for j in range(1, C):
        if fin[j] > fin[bt]:
            bt = j
    path = [0] * (last + 1)
    path[last] = bt
    for t in range(last, 0, -1):
        bt = bp[t][bt]
        path[t - 1] = bt
    return path, fin[path[last]], states, fin, bp


def mask_is_prefix(mask_row, S):
    """the on positions are 0 .. sum(mask) - 1: the path is then the best chain over them"""
    if mask_row is None:
        return True
    m = (mask_row != 0).tolist()
    n = sum(m)
    return n >= 1 and all(m[:n])


def path_terms(path, e, start, end, trans):
    """terms of the float64 score of ``path`` as the chain over positions 0 .. len(path) - 1"""
    E, T = e.double(), trans.double()
    t = [float(start[path[0]]), float(E[0, path[0]])]
    for k in range(1, len(path)):
        t += [float(T[path[k - 1], path[k]]), float(E[k, path[k]])]
    return t + [float(end[path[-1]])]


def viterbi_tol(L, *term_lists):
    """2 (2 L + 2) u sum |terms|: an f32 running sum of the 2 L + 1 terms of a path errs by at most (2 L + 2) u times their absolute
    sum; the kernel's path beats the optimum in f32, so in float64 it loses at most the error of both (the larger absolute sum
    of the two is charged twice)."""
    return 2 * (2 * L + 2) * U_ACC * max(sum(abs(x) for x in t) for t in term_lists)


def check_path(path, best_score, e, mask_row, start, end, trans, exact, vref=None):
    """Assertions on one sample's Viterbi output -> worst err / tol (0 for exact cases).  ``exact`` (integer parameters: every
    f32 sum is exact): the path and the score equal the tie-rule reference.  Otherwise, for a prefix mask: the float64 score of
    the path is within ``viterbi_tol`` of the optimum and best_score within it of that score; for a mask with holes, where
    the package's path is not the optimum of any chain, every choice is checked where it was made: the final tag against the
    final scores and each back-pointer against the state it was taken from, each within the same tolerance."""
    S, C = e.shape
    ref_path, ref_score, states, fin, bp = viterbi_ref(e, mask_row, start, end, trans) if vref is None else vref
    assert len(path) == len(ref_path), ("path length", len(path), len(ref_path))
    assert all(0 <= p < C for p in path), path
    if exact:
        assert path == ref_path, (path, ref_path)
        assert best_score is None or best_score == ref_score, (best_score, ref_score)
        return 0.0
    L = len(PO.on_positions(mask_row, S))
    T = trans.double().tolist()
    if mask_is_prefix(mask_row, S):
        tp, to = path_terms(path, e, start, end, trans), path_terms(ref_path, e, start, end, trans)
        tol = viterbi_tol(L, tp, to)
        worst = (sum(to) - sum(tp)) / tol
        assert sum(tp) >= sum(to) - tol, ("path score", sum(tp), sum(to), tol)
        mine = sum(tp)
    else:
        absT = max(abs(v) for row in T for v in row)
        terms = [float(start.abs().max())] + [float(e[t].abs().max()) for t in PO.on_positions(mask_row, S)] + [absT] * (L - 1) \
            + [float(end.abs().max())]
        tol = viterbi_tol(L, terms)
        last = len(path) - 1
        worst = (max(fin) - fin[path[last]]) / tol
        for t in range(last, 0, -1):
            cand = [states[t - 1][i] + T[i][path[t]] for i in range(C)]
            worst = max(worst, (max(cand) - cand[path[t - 1]]) / tol)
        assert worst <= 1, ("a Viterbi choice is worse than the best by more than the tolerance", worst, tol)
        mine = fin[path[last]]
    if best_score is not None:
        worst = max(worst, abs(best_score - mine) / tol)
        assert abs(best_score - mine) <= tol, ("best_score", best_score, mine, tol)
    return worst


# ------------------------------------------------------------------------------------------------------------ cases
MASKS = ("none", "full", "prefix", "holes", "first_off")
PARAMS = ("plain", "forbid", "wide", "integer")

CASES = [
    (3, 1, 3, "none", "plain"), (3, 1, 3, "prefix", "integer"), (3, 1, 16, "full", "plain"), (3, 1, 17, "holes", "plain"),
    (3, 6, 3, "none", "plain"), (3, 6, 3, "full", "integer"), (3, 6, 3, "prefix", "plain"), (3, 6, 3, "holes", "plain"),
    (3, 6, 3, "first_off", "plain"), (3, 6, 3, "holes", "integer"), (3, 6, 3, "first_off", "integer"),
    (3, 6, 16, "holes", "plain"), (3, 6, 16, "first_off", "integer"), (3, 6, 16, "prefix", "plain"),
    (3, 6, 17, "holes", "plain"), (3, 6, 17, "first_off", "integer"), (3, 6, 17, "prefix", "plain"),
    (2, 5, 64, "holes", "plain"), (2, 5, 64, "first_off", "integer"),
    (3, 63, 13, "holes", "plain"), (3, 64, 13, "holes", "plain"), (3, 65, 13, "holes", "integer"),
    (2, 315, 13, "full", "plain"), (2, 316, 13, "holes", "integer"),
    (2, 512, 8, "holes", "plain"),
    (2, 256, 16, "none", "plain"), (2, 257, 16, "holes", "integer"),
    (2, 512, 16, "holes", "plain"), (2, 513, 16, "first_off", "integer"),
    (1, 192, 64, "full", "plain"),
    (3, 12, 13, "holes", "forbid"), (3, 12, 13, "prefix", "wide"), (3, 12, 40, "holes", "forbid"), (3, 12, 40, "prefix", "wide"),
    (3, 8, 13, "first_off", "forbid"), (3, 8, 13, "holes", "wide"),
]
REFUSED_CASE = (1, 193, 64, "none", "plain")        # S * C = 12352: icka_crf_llh works, the other three return ICKA_E_SHAPE
BRUTE = [c for c in CASES if c[1] == 6 and c[2] == 3]


def case_id(c):
    return "B%d_S%d_C%d_%s_%s" % c


def make_masks(B, S, kind, g):
    """int64 [B, S] or None.  prefix: rows of length S, random, 1 (B = 2: S and 1).  holes: position 0 on everywhere; row 0 random
    with position S - 1 on after a hole at S - 2; row 1 all off past position 0 (B >= 3); other rows random.  first_off: row 0
    has mask[0] == 0 and its last position (and random others) on; the other rows have random holes."""
    if kind == "none":
        return None
    if kind == "full":
        return torch.ones(B, S, dtype=torch.int64)
    if kind == "prefix":
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0] = S
        lens[B - 1] = 1 if B > 1 else S
        return (torch.arange(S)[None, :] < lens[:, None]).long()
    m = (torch.rand(B, S, generator=g) < 0.6).long()
    m[:, 0] = 1
    if kind == "holes":
        m[0, S - 1] = 1
        if S >= 3:
            m[0, S - 2] = 0
        if B >= 3:
            m[1, 1:] = 0
    else:
        if S < 2:
            raise ValueError("first_off needs S >= 2: an all-zero row has no reference")
        m[0, 0] = 0
        m[0, S - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of a case (CPU tensors, f32 / int64), seeded by the case.  Labels at off positions are 0 or C - 1, so that
    ``pad_labels`` can replace them by out-of-range values that clamp to the same.  gllh holds a negative value, powers of two
    and (B >= 3) a zero."""
    B, S, C, mk, pk = case
    g = torch.Generator().manual_seed(B * 100003 + S * 1009 + C * 17 + MASKS.index(mk) * 5 + PARAMS.index(pk))
    if pk == "integer":
        ri = lambda *s: torch.randint(-3, 4, s, generator=g).float()
        e, start, end, trans = ri(B, S, C), ri(C), ri(C), ri(C, C)
    else:
        e = torch.randn(B, S, C, generator=g) * {"plain": 1.0, "wide": 30.0, "forbid": 40.0}[pk]
        start, end = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
        trans = torch.randn(C, C, generator=g) * 0.7
        if pk == "forbid":          # every tag but 0 can be entered from tag 0 only
            trans[:, 1:] = -1e4
            trans[0, 1:] = 0.0
    mask = make_masks(B, S, mk, g)
    tags = torch.randint(0, C, (B, S), generator=g)
    if mask is not None:
        off = mask == 0
        off[:, 0] = False
        edge = ((torch.arange(S)[None, :] + torch.arange(B)[:, None]) % 2) * (C - 1)
        tags = torch.where(off, edge, tags)
    gllh = torch.tensor({1: [2.0], 2: [-0.75, 2.0], 3: [-0.75, 2.0, 0.0], 4: [-0.75, 2.0, 0.5, 0.0]}[B])
    init = {"dstart": torch.randn(C, generator=g), "dend": torch.randn(C, generator=g) + 3.0, "dtrans": torch.randn(C, C, generator=g) - 2.0}
    return {"e": e, "tags": tags, "mask": mask, "start": start, "end": end, "trans": trans, "gllh": gllh, "init": init}


def pad_labels(inp):
    """tags with the labels at off positions replaced by -100 (where they were 0) and C + 5 (where they were C - 1): the
    clamped values are the ones every rule read before, so llh and d_emissions must not change by a bit."""
    B, S, C = inp["e"].shape
    if inp["mask"] is None:
        return inp["tags"].clone()
    off = inp["mask"] == 0
    off[:, 0] = False
    t = inp["tags"]
    return torch.where(off & (t == 0), torch.full_like(t, -100), torch.where(off & (t == C - 1), torch.full_like(t, C + 5), t))


@functools.lru_cache(maxsize=None)
def expected(case):
    """Everything the tests compare with, computed once per case and left unchanged: chains, reference, bounds."""
    inp = make_case(case)
    ch = chains(inp)
    ref = reference(inp)
    bnd = bounds(inp, ch, ref, inp["init"])
    tot = {k: ref[k] + inp["init"][k].double() for k in ("dstart", "dend", "dtrans")}
    for k in tot:
        bnd[k] = stored(bnd[k], tot[k], F32)
    return {"inp": inp, "chains": ch, "ref": ref, "bounds": bnd, "total": tot}


@functools.lru_cache(maxsize=None)
def viterbi_of(case, b):
    inp = make_case(case)
    return viterbi_ref(inp["e"][b], None if inp["mask"] is None else inp["mask"][b], inp["start"], inp["end"], inp["trans"])


def coverage(cases=None):
    """-> (kernels reached, {small kernel: forms reached}) from the restated dispatch; ``assert_coverage`` demands all eight
    kernels and, for the three small likelihood / gradient kernels, the scaled form, the log form by size and by give-up."""
    cases = CASES if cases is None else cases
    kern, fr = set(), {"crf_llh_small_kernel": set(), "crf_grad_small_kernel": set(), "crf_score_decode_small_kernel": set()}
    for case in list(cases) + [REFUSED_CASE]:
        B, S, C = case[:3]
        for en in ENTRIES:
            if not refused(en, S, C):
                kern.add(kernel_of(en, S, C))
        if small(S, C) and case != REFUSED_CASE:
            for fl, fg, why in forms(make_case(case)):
                for k, f in (("crf_llh_small_kernel", fl), ("crf_score_decode_small_kernel", fl), ("crf_grad_small_kernel", fg)):
                    if f != "either":
                        fr[k].add("lin" if f == "lin" else "log by " + why)
    return kern, fr


def assert_coverage(cases=None):
    kern, fr = coverage(cases)
    assert kern == set(KERNELS), sorted(set(KERNELS) - kern)
    for k, got in fr.items():
        assert got >= {"lin", "log by size", "log by give-up"}, (k, sorted(got))
    return kern, fr
