"""Helpers of the element-wise tests of the fp32-exact kernels (csrc/exact.hip, icka_x_*; no test functions): for every
kernel a function that takes the exact f32 inputs and returns {output: (float64 reference, bound)}.  The buffers, the
comparison and the GEMM accumulation bound are those of tests/kernel_check.py; nothing here is a fitted constant.

Where the bounds come from
--------------------------
* One f32 operation (add, multiply, divide, sqrt; an fma is one, not two) is off by at most U = 2^-24 of its result.
* An f32 sum of n terms in ANY order (lanes with stride 64, DPP tree, LDS tree, row phases, atomics) is charged
  (n + 4) U_ACC sum|terms|, U_ACC = 2^-23, as tests/kernel_check.py does: n - 1 additions plus four spare roundings that
  pay for what produced each term (a product, a mask multiply) and the division by n.
* A device math function (expf, logf, erff, tanhf) is charged LIBM_REL = 2^-22 of its result: a REQUIREMENT on the device
  function (4 ulp), the figure the suite's token-CE bound already charges expf and logf.  It is propagated through what
  follows the call: in 1 - tanh^2, g (1 - g) and gelu' the charge is an ABSOLUTE term (LIBM_REL |tanh| etc.), because the
  subtraction that follows can cancel.
* Every result is stored in f32: ``stored(err, ref, F32)`` adds U (|ref| + err) and the 2^-126 a flushed subnormal costs.
* Dropout masks are inputs (kernels.dropout_mask / kernels.attn_dropout_mask, pinned to CPU restatements elsewhere): the
  functions take the multiplier tensor m (0 or 1 / (1 - p); ones without dropout).

Every function works on the device of its inputs, so tests/test_exact_check_cpu.py runs them on CPU emulations of the
kernels (and on seeded faults) at the very shapes tests/test_exact_elements_gpu.py runs on the device.
"""
import math

import torch

from kernel_check import (F32, Guarded, U_ACC, assert_within, gemm_acc_bound, guarded, guarded_input,  # noqa: F401
                          report, stored, with_beta)

U = 2.0 ** -24             # unit roundoff of one f32 operation (round to nearest)
LIBM_REL = 2.0 ** -22      # REQUIREMENT on expf / logf / erff / tanhf of the device: relative error of the result

NT, NN, TN, TT = 0, 1, 2, 3            # ICKA_GEMM_* (include/icka_hip.h)
F64 = torch.float64


def _d(t):
    return t.double()


def _st(ref, err):
    return ref, stored(err, ref, F32)


# ------------------------------------------------------------------------------------------------------------ GEMM
def gemm_refs(op, A, B, bias, alpha, beta, c_old):
    """icka_x_gemm: C = alpha op(A) op(B) + bias + beta C_old.  A is [.., M, K] (NT, NN) or [.., K, M] (TN, TT), B is [.., N, K]
    (NT, TT) or [.., K, N] (NN, TN); leading dimensions are the batch.  The products of f32 operands are exact inside the fma
    chain of the matrix instruction, so the error is that of a length-K f32 sum: ``gemm_acc_bound`` (the +4 pays the alpha
    multiply and the bias add); beta C_old enters through ``with_beta``.  With beta == 0 C_old is not read: the reference
    ignores it (the test fills it with NaN)."""
    a = _d(A) if op in (NT, NN) else _d(A).transpose(-1, -2)
    b = _d(B).transpose(-1, -2) if op in (NT, TT) else _d(B)
    K = a.shape[-1]
    ref = alpha * (a @ b)
    if bias is not None:
        ref = ref + _d(bias)
    err = gemm_acc_bound(a.abs() @ b.abs(), K, alpha, bias)
    if beta != 0:
        ref, err = with_beta(err, ref, beta, c_old)
    return {"C": _st(ref, err)}


# ------------------------------------------------------------------------------------------------------- LayerNorm
def ln_core(s, t_abs, n_pre, gamma, beta, eps):
    """The LayerNorm of a row s whose elements were formed by ``n_pre`` f32 operations on terms of absolute sum t_abs (the
    structure of kernel_check.ln_fwd_bounds, f32 storage throughout):
      e_s    = n_pre U t_abs
      e_mean = (H + 4) U_ACC mean(t_abs)                      f32 sum of length H, then / H
      e_c    = e_s + e_mean + U |c|,  c = s - mean
      e_var  = (H + 4) U_ACC var + mean(2 |c| e_c + e_c^2)   f32 sum of squares; (c + e)^2 - c^2 = 2 c e + e^2
      r_rstd = e_var / (2 (var + eps - e_var)) + 3 U          relative: |(v + e)^-1/2 - v^-1/2| <= v^-1/2 e / (2 (v - e)); the
                                                              add of eps, the sqrt and the division are one rounding each
      e_xhat = rstd e_c + |xhat| (r_rstd + U)
      e_y    = |gamma| e_xhat + U (|gamma xhat| + |y|)        product and add
    An all-zero row has every term zero: y == beta bitwise.  H = 1 gives c == 0 exactly."""
    H = s.shape[-1]
    s, t_abs, g, b = _d(s), _d(t_abs), _d(gamma), _d(beta)
    mean = s.mean(-1, keepdim=True)
    c = s - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = c * rstd
    e_s = n_pre * U * t_abs
    e_mean = (H + 4) * U_ACC * t_abs.mean(-1, keepdim=True)
    e_c = e_s + e_mean + U * c.abs()
    e_var = (H + 4) * U_ACC * var + (2 * c.abs() * e_c + e_c * e_c).mean(-1, keepdim=True)
    r_rstd = e_var / (2 * (var + eps - e_var).clamp_min(1e-300)) + 3 * U
    e_xhat = rstd * e_c + xhat.abs() * (r_rstd + U)
    y = g * xhat + b
    e_y = g.abs() * e_xhat + U * ((g * xhat).abs() + y.abs())
    return {"y": _st(y, e_y), "xhat": _st(xhat, e_xhat), "rstd": _st(rstd[..., 0], rstd[..., 0] * r_rstd[..., 0])}


def ln_fwd_refs(x, m, residual, gamma, beta, eps):
    """icka_x_ln_fwd: (y, xhat, rstd) of LN(x m + residual); two f32 operations form an element (one without residual)."""
    x, m = _d(x), _d(m)
    r = torch.zeros_like(x) if residual is None else _d(residual)
    return ln_core(x * m + r, x.abs() * m + r.abs(), 2, gamma, beta, eps)


def ln_bwd_refs(dy, xhat, rstd, gamma, m):
    """icka_x_ln_bwd from the SAVED xhat / rstd (exact as given), as kernel_check.ln_bwd_bounds:
      gd   = dy gamma                         U |gd|
      c1   = mean(gd), c2 = mean(gd xhat)     (H + 4) U_ACC mean|gd|, (H + 4) U_ACC mean|gd xhat|
      dpre = rstd (gd - c1 - xhat c2)         rstd (U |gd| + e_c1 + |xhat| e_c2) + 4 U rstd (|gd| + |c1| + |xhat c2|)
                                              (product xhat c2, two subtractions, the multiply by rstd)
      ddense = dpre m                         m e_dpre + U |ddense|"""
    H = dy.shape[-1]
    dy, xh, g, m = _d(dy), _d(xhat), _d(gamma), _d(m)
    r = _d(rstd)[:, None]
    gd = g * dy
    c1 = gd.mean(-1, keepdim=True)
    c2 = (gd * xh).mean(-1, keepdim=True)
    e_c1 = (H + 4) * U_ACC * gd.abs().mean(-1, keepdim=True)
    e_c2 = (H + 4) * U_ACC * (gd * xh).abs().mean(-1, keepdim=True)
    ds = r * (gd - c1 - xh * c2)
    e_ds = r * (U * gd.abs() + e_c1 + xh.abs() * e_c2) + 4 * U * r * (gd.abs() + c1.abs() + (xh * c2).abs())
    dd = ds * m
    return {"dpre": _st(ds, e_ds), "ddense": _st(dd, m * e_ds + U * dd.abs())}


def colsum_refs(a, b, accumulate, prefill):
    """icka_x_colsum: out[c] (+)= sum_r a[r, c] (b[r, c]): an f32 sum of M terms in any order (four row phases, then a tree):
    (M + 4) U_ACC sum|a b|; accumulating adds the prefill through ``with_beta``."""
    M = a.shape[0]
    t = _d(a) if b is None else _d(a) * _d(b)
    ref, err = t.sum(0), (M + 4) * U_ACC * t.abs().sum(0)
    if accumulate:
        ref, err = with_beta(err, ref, 1.0, prefill)
    return {"out": _st(ref, err)}


# ------------------------------------------------------------------------------------------------------ embeddings
def embed_rows(ids, tt, S):
    """-> (word row, position row, type row) index of every one of the B*S rows of icka_x_embed_fwd"""
    M = ids.numel()
    rows = torch.arange(M, device=ids.device)
    return ids.reshape(-1), rows % S, (torch.zeros_like(rows) if tt is None else tt.reshape(-1))


def embed_fwd_refs(ids, tt, word, pos, typ, gamma, beta, S, eps):
    """icka_x_embed_fwd: LN((word[id] + pos[row % S]) + type[tt]): two f32 additions form an element."""
    wi, pi, ti = embed_rows(ids, tt, S)
    w, p, t = _d(word)[wi], _d(pos)[pi], _d(typ)[ti]
    return ln_core(w + p + t, w.abs() + p.abs() + t.abs(), 2, gamma, beta, eps)


def scatter_refs(dpre, index, nrows, prefill, skip=None):
    """One table of a scatter: table[index[r]] += dpre[r] by f32 atomics in any order onto the prefilled table:
    (count + 4) U_ACC (sum|dpre rows| + |prefill|) per element, count = rows that land there.  ``skip``: rows of that index
    receive nothing (padding_idx).  A row with count 0 keeps its prefill bitwise (error 0 against a bound > 0; the test
    checks the padding row bitwise on top)."""
    g = _d(dpre)
    keep = torch.ones_like(index, dtype=torch.bool) if skip is None else index != skip
    H = g.shape[1]
    ref = torch.full((nrows, H), float(prefill), dtype=F64, device=g.device)
    ab = torch.full((nrows, H), abs(float(prefill)), dtype=F64, device=g.device)
    cnt = torch.zeros(nrows, dtype=F64, device=g.device)
    ref.index_add_(0, index[keep], g[keep])
    ab.index_add_(0, index[keep], g[keep].abs())
    cnt.index_add_(0, index[keep], torch.ones(int(keep.sum()), dtype=F64, device=g.device))
    return _st(ref, (cnt[:, None] + 4) * U_ACC * ab)


def embed_scatter_refs(dpre, ids, tt, S, sizes, padding_idx, prefill):
    """icka_x_embed_scatter: the three tables (sizes = rows of word, pos, type) receive sums of dpre rows."""
    wi, pi, ti = embed_rows(ids, tt, S)
    return {"dword": scatter_refs(dpre, wi, sizes[0], prefill, skip=padding_idx),
            "dpos": scatter_refs(dpre, pi, sizes[1], prefill), "dtyp": scatter_refs(dpre, ti, sizes[2], prefill)}


def prompt_rows(ids, src, B, S_in, S, P, pos_offset):
    """-> per output row of the prompt embedding (B*S rows): is_prompt, word id (0 where prompt), prompt row b*P + p (0 where
    word), position row sp + pos_offset"""
    dev = ids.device
    b = torch.arange(B, device=dev).repeat_interleave(S)
    sp = torch.arange(S, device=dev).repeat(B)
    sidx = src.long()[sp]
    isp = sidx < 0
    wid = ids.reshape(B, S_in)[b, sidx.clamp_min(0)]
    prow = b * P + (-1 - sidx).clamp_min(0)
    return isp, torch.where(isp, torch.zeros_like(wid), wid), torch.where(isp, prow, torch.zeros_like(prow)), sp + pos_offset


def prompt_fwd_refs(ids, src, prompt, word, pos, typ, gamma, beta, B, S_in, S, P, pos_offset, eps):
    """icka_x_embed_prompt_fwd: LN((x + pos[t + pos_offset]) + type[0]), x a word row or a prompt row."""
    isp, wid, prow, prw = prompt_rows(ids, src, B, S_in, S, P, pos_offset)
    x = torch.where(isp[:, None], _d(prompt).reshape(B * P, -1)[prow], _d(word)[wid])
    p, t = _d(pos)[prw], _d(typ)[0][None]
    return ln_core(x + p + t, x.abs() + p.abs() + t.abs(), 2, gamma, beta, eps)


def prompt_scatter_refs(dpre, ids, src, B, S_in, S, P, pos_offset, sizes, padding_idx, prefill):
    """icka_x_embed_prompt_scatter: word rows by atomics (prompt positions and the padding id excluded), position rows
    sp + pos_offset, type row 0 from every row; "dprompt": (row of dpre that each [b, p] must equal BITWISE, or -1)."""
    isp, wid, prow, prw = prompt_rows(ids, src, B, S_in, S, P, pos_offset)
    windex = torch.where(isp, torch.full_like(wid, -7), wid)          # -7: never a row, never the padding id
    keep = ~isp
    out = {"dword": scatter_refs(dpre[keep], windex[keep], sizes[0], prefill, skip=padding_idx),
           "dpos": scatter_refs(dpre, prw, sizes[1], prefill),
           "dtyp": scatter_refs(dpre, torch.zeros_like(prw), sizes[2], prefill)}
    source = torch.full((B * P,), -1, dtype=torch.long, device=ids.device)
    source[prow[isp]] = torch.nonzero(isp)[:, 0]
    out["dprompt_source"] = source
    return out


# --------------------------------------------------------------------------------------------------------- softmax
def softmax_fwd_refs(P0, mask, m, scale, rows_per_batch):
    """icka_x_softmax_fwd, P0 [rows, Skv] the scores, mask [B, Skv] additive, m [rows, Skv] the attention dropout multiplier.
      z_j  = P0_j scale + mask_j                U (|P0_j scale| + |z_j|)          = e_z
      a_j  = z_j - max                          softmax is shift-invariant, so which maximum the kernel found does not
                                                matter; the subtraction costs U |a_j|:   D_j = e_z + U |z_j - max z|
      n_j  = expf(a_j)                          relative rho_j = expm1(D_j) + LIBM_REL
      se   = sum_j n_j                          relative rho_se = sum_j p_j rho_j + (Skv + 4) U_ACC
      p_j  = n_j / se                           relative (1 + rho_j) (1 + U) / (1 - rho_se) - 1
      Pd_j = p_j m_j                            m_j e_p + U |Pd_j|
    A batch whose keys are all at -10000 has |z| near 1e4: e_z is then near 6e-4 and the bound says so."""
    Skv = P0.shape[-1]
    rows = P0.shape[0]
    mk = _d(mask)[torch.arange(rows, device=P0.device) // rows_per_batch]
    z = _d(P0) * scale + mk
    p = torch.softmax(z, -1)
    D = U * ((_d(P0) * scale).abs() + z.abs()) + U * (z - z.amax(-1, keepdim=True)).abs()
    rho = torch.expm1(D) + LIBM_REL
    rho_se = (p * rho).sum(-1, keepdim=True) + (Skv + 4) * U_ACC
    e_p = p * ((1 + rho) * (1 + U) / (1 - rho_se) - 1)
    pd = p * _d(m)
    return {"P": _st(p, e_p), "Pd": _st(pd, _d(m) * e_p + U * pd.abs())}


def softmax_bwd_refs(P, dPd, m, scale):
    """icka_x_softmax_bwd from the SAVED P (exact as given): dp = dPd m (U |dp|); dot = sum_j dp_j p_j, an f32 sum:
    e_dot = (Skv + 4) U_ACC sum|dp p|; dS = p (dp - dot) scale: |p scale| (U |dp| + e_dot + U |dp - dot|) + 2 U |dS|."""
    Skv = P.shape[-1]
    p, dp = _d(P), _d(dPd) * _d(m)
    dot = (dp * p).sum(-1, keepdim=True)
    e_dot = (Skv + 4) * U_ACC * (dp * p).abs().sum(-1, keepdim=True)
    dS = p * (dp - dot) * scale
    return {"dS": _st(dS, (p * scale).abs() * (U * dp.abs() + e_dot + U * (dp - dot).abs()) + 2 * U * dS.abs())}


# ------------------------------------------------------------------------------------------------------ elementwise
SQRT1_2, INV_SQRT_2PI = math.sqrt(0.5), 1.0 / math.sqrt(2.0 * math.pi)


def _erf_parts(x):
    """1 + erf(x / sqrt 2) in float64 without cancellation (erfc(-a)), and the error of the f32 evaluation 1 + erff(x c):
    the argument a = x c carries 2 U |a| (the f32 constant, the product), erf' = 2 / sqrt(pi) exp(-a^2); erff itself
    LIBM_REL |erf|; the addition U |1 + erf|."""
    a = _d(x) * SQRT1_2
    one_plus = torch.special.erfc(-a)
    e = 2.0 / math.sqrt(math.pi) * torch.exp(-a * a) * 2 * U * a.abs() + LIBM_REL * torch.erf(a).abs() + U * one_plus
    return one_plus, e


def sigmoid_err(z, e_z=0.0):
    """s = 1 / (1 + expf(-z)) for an argument with error e_z: expf relative expm1(e_z) + LIBM_REL, which moves s by
    s (1 - s) of it; the addition and the division one rounding each.  Below 2^-126 ``stored`` pays the flush (expf(100)
    overflows to inf and s becomes 0)."""
    s = torch.sigmoid(_d(z))
    return s, s * ((1 - s) * (math.expm1(e_z) if isinstance(e_z, float) else torch.expm1(e_z)) + (1 - s) * LIBM_REL + 2 * U)


def act_fwd_refs(mode, x, aux=None):
    """icka_x_act_fwd.  0: y = x 0.5 (1 + erff(x c)): |x / 2| e_(1+erf) + 2 U |y| (two products).  1: y = tanhf(x): LIBM_REL |y|.
    2: y2 = sigmoid(x) (``sigmoid_err``), y = y2 aux: |aux| e_s + U |y|."""
    x = _d(x)
    if mode == 0:
        op, e = _erf_parts(x)
        y = 0.5 * x * op
        return {"y": _st(y, (0.5 * x).abs() * e + 2 * U * y.abs())}
    if mode == 1:
        y = torch.tanh(x)
        return {"y": _st(y, LIBM_REL * y.abs())}
    s, e_s = sigmoid_err(x)
    y = s * _d(aux)
    return {"y2": _st(s, e_s), "y": _st(y, _d(aux).abs() * e_s + U * y.abs())}


def act_bwd_refs(mode, dy, saved, aux=None):
    """icka_x_act_bwd (saved and aux exact as given).
      0: gelu'(x) = 0.5 (1 + erf) + x k expf(q), q = -0.5 x x.  First term 0.5 e_(1+erf).  q costs 2 U |q|, so G = expf(q) is
         off by G (expm1(2 U |q|) + LIBM_REL) = e_G -- an ABSOLUTE term of gelu'; x k G: |x k| e_G + 3 U |x k G| (the constant,
         two products); the sum U |gelu'|.  dx = dy gelu': |dy| e + U |dx|.
      1: dx = dy (1 - y^2): |dy| (U y^2 + U |1 - y^2|) + U |dx|.
      2: dx = dy aux g (1 - g): |dy aux g| U |1 - g| + 3 U |dx|;  dx2 = dy g: U |dx2|."""
    dy, s = _d(dy), _d(saved)
    if mode == 0:
        op, e_op = _erf_parts(s)
        q = -0.5 * s * s
        G = torch.exp(q)
        e_G = G * (torch.expm1(2 * U * q.abs()) + LIBM_REL)
        t2 = s * INV_SQRT_2PI * G
        gp = 0.5 * op + t2
        e = 0.5 * e_op + (s * INV_SQRT_2PI).abs() * e_G + 3 * U * t2.abs() + U * gp.abs()
        dx = dy * gp
        return {"dx": _st(dx, dy.abs() * e + U * dx.abs())}
    if mode == 1:
        dx = dy * (1 - s * s)
        return {"dx": _st(dx, dy.abs() * (U * s * s + U * (1 - s * s).abs()) + U * dx.abs())}
    a = _d(aux)
    dx, dx2 = dy * a * s * (1 - s), dy * s
    return {"dx": _st(dx, (dy * a * s).abs() * U * (1 - s).abs() + 3 * U * dx.abs()), "dx2": _st(dx2, torch.zeros_like(dx2))}


def mul_refs(x, m):
    """icka_x_dropout (y = x m) and any single product: one rounding, which ``stored`` charges."""
    y = _d(x) * _d(m)
    return {"y": _st(y, torch.zeros_like(y))}


def add_refs(a, b):
    """icka_x_add: one rounding."""
    y = _d(a) + _d(b)
    return {"out": _st(y, torch.zeros_like(y))}


def scale_ratio_refs(x, num, den):
    """icka_x_scale_by_ratio: s = num / max(den, 1) (U |s|; NULL = 1), y = x s: U |y| before the store."""
    s = (1.0 if num is None else float(num)) / (1.0 if den is None else max(float(den), 1.0))
    y = _d(x) * s
    return {"y": _st(y, U * y.abs())}


# ----------------------------------------------------------------------------------------------------- sample gates
def _sample_gate(gate, mode):
    """g [B] and its error: mode 0 sigmoid(gate[b]); mode 1 1 / (1 + expf(gate[2b] - gate[2b+1])), whose argument
    d = gate[2b] - gate[2b+1] costs U |d|."""
    gate = _d(gate)
    if mode == 0:
        return sigmoid_err(gate.reshape(-1))
    d = gate.reshape(-1, 2)[:, 0] - gate.reshape(-1, 2)[:, 1]
    return sigmoid_err(-d, U * d.abs())


def sample_gate_fwd_refs(a, c, gate, mode, B, S):
    """icka_x_sample_gate_fwd: out = g a + (1 - g) c (c NULL: g a).  1 - g: e_g + U |1 - g|; two products and one add:
    |a| e_g + |c| (e_g + U |1 - g|) + 2 U (|g a| + |(1 - g) c|)."""
    g, e_g = _sample_gate(gate, mode)
    g, e_g = g.repeat_interleave(S)[:, None], e_g.repeat_interleave(S)[:, None]
    a = _d(a)
    if c is None:
        return {"out": _st(g * a, a.abs() * e_g + U * (g * a).abs())}
    c = _d(c)
    out = g * a + (1 - g) * c
    return {"out": _st(out, a.abs() * e_g + c.abs() * (e_g + U * (1 - g).abs()) + 2 * U * ((g * a).abs() + ((1 - g) * c).abs()))}


def sample_gate_bwd_refs(dout, a, c, gate, mode, B, S):
    """icka_x_sample_gate_bwd: da = g d: |d| e_g + U |da|; dc = (1 - g) d: |d| (e_g + U |1 - g|) + U |dc|;
    acc_b = sum over the S H elements of d (a - c): (n + 4) U_ACC sum|d (a - c)| (the subtraction and the product are two of
    the four spare roundings); t = acc g (1 - g): |g (1 - g)| e_acc + |acc| (|1 - g| e_g + |g| (e_g + U |1 - g|)) + 2 U |t|.
    dgate: mode 0 [B] = t; mode 1 [B, 2] = (-t, +t), the same error for both words."""
    g, e_g = _sample_gate(gate, mode)
    d, a = _d(dout), _d(a)
    H = a.shape[1]
    gr, er = g.repeat_interleave(S)[:, None], e_g.repeat_interleave(S)[:, None]
    out = {"da": _st(gr * d, d.abs() * er + U * (gr * d).abs())}
    diff = a if c is None else a - _d(c)
    if c is not None:
        out["dc"] = _st((1 - gr) * d, d.abs() * (er + U * (1 - gr).abs()) + U * ((1 - gr) * d).abs())
    terms = (d * diff).reshape(B, S * H)
    acc, e_acc = terms.sum(-1), (S * H + 4) * U_ACC * terms.abs().sum(-1)
    t = acc * g * (1 - g)
    e_t = (g * (1 - g)).abs() * e_acc + acc.abs() * ((1 - g).abs() * e_g + g.abs() * (e_g + U * (1 - g).abs())) + 2 * U * t.abs()
    if mode == 0:
        out["dgate"] = _st(t, e_t)
    else:
        out["dgate"] = _st(torch.stack([-t, t], -1), torch.stack([e_t, e_t], -1))
    return out


# -------------------------------------------------------------------------------------------------------- LSTM cell
def lstm_rows(B, S, k):
    """-> per direction (t, t_prev) of step k: the forward direction runs at t = k and reads t - 1, the reverse at
    t = S - 1 - k and reads t + 1."""
    return [(k, k - 1), (S - 1 - k, S - k)]


def lstm_fwd_refs(z, c_all, y, B, S, H, k):
    """icka_x_lstm_cell_fwd, step k.  z [B, S, 2, 4, H]: the pre-activations the test supplied; c_all / y [B, S, 2, H]: what the
    KERNEL stored (only the neighbouring step k - 1 is read, exact as given).  -> per direction d a dict of (reference, bound)
    for "act" [B, 4, H], "c" and "y" [B, H] at row t, and "hprev": the tensor hprev[:, t, d] must equal BITWISE.
      i, f, o = sigmoid(z)       ``sigmoid_err``;     g = tanhf(z): LIBM_REL |g|
      c = f c' + i g             |c'| e_f + |g| e_i + |i| e_g + e_i e_g + 2 U (|f c'| + |i g|)
      h = o tanhf(c)             tanh is 1-Lipschitz: e_tc = e_c + LIBM_REL |tanh c|;  |tc| e_o + |o| e_tc + e_o e_tc + U |h|"""
    out = []
    for d, (t, tp) in enumerate(lstm_rows(B, S, k)):
        zz = _d(z[:, t, d])
        i, e_i = sigmoid_err(zz[:, 0])
        f, e_f = sigmoid_err(zz[:, 1])
        o, e_o = sigmoid_err(zz[:, 3])
        g = torch.tanh(zz[:, 2])
        e_g = LIBM_REL * g.abs()
        cp = _d(c_all[:, tp, d]) if k else torch.zeros_like(g)
        c = f * cp + i * g
        e_c = cp.abs() * e_f + g.abs() * e_i + i.abs() * e_g + e_i * e_g + 2 * U * ((f * cp).abs() + (i * g).abs())
        tc = torch.tanh(c)
        e_tc = e_c + LIBM_REL * tc.abs()
        h = o * tc
        e_h = tc.abs() * e_o + o.abs() * e_tc + e_o * e_tc + U * h.abs()
        out.append({"act": _st(torch.stack([i, f, g, o], 1), torch.stack([e_i, e_f, e_g, e_o], 1)), "c": _st(c, e_c),
                    "y": _st(h, e_h), "hprev": y[:, tp, d] if k else torch.zeros_like(y[:, t, d])})
    return out


def lstm_bwd_refs(dy, dh_rec, dc_in, act, c_all, B, S, H, k, first):
    """icka_x_lstm_cell_bwd, step k.  dy / c_all [B, S, 2, H], act [B, S, 2, 4, H] (the saved activations), dh_rec / dc_in
    [2, B, H]: the carry the KERNEL left after step k + 1 -- all exact as given; with ``first`` dh_rec and dc_in are not read
    (the test fills them with NaN).  -> per direction {"dgates": [B, 4, H], "dc_carry": [B, H]} as (reference, bound).
      dh = dy + dh_rec                    U |dh|
      tc = tanhf(c)                       LIBM_REL |tc|;   s = 1 - tc^2: 2 |tc| e_tc + e_tc^2 + U tc^2 + U |s|  (ABSOLUTE)
      a  = dh o s                         |o s| e_dh + |dh o| e_s + 2 U |a|
      dc = carry + a                      e_a + U |dc|                       (carry exact)
      di = dc g i (1 - i), df = dc c' f (1 - f):   |factor| e_dc + 5 U |.|    (1 - x is relative U of itself; three products)
      dg = dc i (1 - g^2)                 |i (1 - g^2)| e_dc + |dc i| (U g^2 + U |1 - g^2|) + 2 U |dg|
      do = dh tc o (1 - o)                |tc o (1 - o)| e_dh + |dh o (1 - o)| e_tc + 5 U |do|
      dc_carry' = dc f                    |f| e_dc + U |dc f|"""
    out = []
    for d, (t, tp) in enumerate(lstm_rows(B, S, k)):
        i, f, g, o = (_d(act[:, t, d, q]) for q in range(4))
        c = _d(c_all[:, t, d])
        cp = _d(c_all[:, tp, d]) if k else torch.zeros_like(c)
        dh = _d(dy[:, t, d]) + (0.0 if first else _d(dh_rec[d]))
        e_dh = U * dh.abs()
        tc = torch.tanh(c)
        e_tc = LIBM_REL * tc.abs()
        s = 1 - tc * tc
        e_s = 2 * tc.abs() * e_tc + e_tc * e_tc + U * tc * tc + U * s.abs()
        a = dh * o * s
        e_a = (o * s).abs() * e_dh + (dh * o).abs() * e_s + 2 * U * a.abs()
        dc = a + (0.0 if first else _d(dc_in[d]))
        e_dc = e_a + U * dc.abs()
        fi, ff, fg = g * i * (1 - i), cp * f * (1 - f), i * (1 - g * g)
        di, df, dg = dc * fi, dc * ff, dc * fg
        do = dh * tc * o * (1 - o)
        e = [fi.abs() * e_dc + 5 * U * di.abs(), ff.abs() * e_dc + 5 * U * df.abs(),
             fg.abs() * e_dc + (dc * i).abs() * (U * g * g + U * (1 - g * g).abs()) + 2 * U * dg.abs(),
             (tc * o * (1 - o)).abs() * e_dh + (dh * o * (1 - o)).abs() * e_tc + 5 * U * do.abs()]
        out.append({"dgates": _st(torch.stack([di, df, dg, do], 1), torch.stack(e, 1)),
                    "dc_carry": _st(dc * f, f.abs() * e_dc + U * (dc * f).abs())})
    return out


# --------------------------------------------------------------------------------------------------------- token CE
def token_ce_refs(x, labels, mask, prefill=(0.5, 2.0)):
    """icka_x_token_ce (the bound of the bf16 test in tests/test_row_kernel_edges_gpu.py, carried over to f32 storage).  A row
    COUNTS if and only if mask != 0 and 0 <= label < C, compared in 64 bits; a row that does not count adds nothing to
    loss_sum / count and its gradient row is all zeros.
      exponent x_c - lse: D_c = U_ACC (2 |x_c| + 3 |lse| + 3 log C + C + 8)   (derived there)
      g = p - onehot:     p expm1(D_c) + LIBM_REL p + U_ACC |g|
      loss = lse - x_y:   D_y + U_ACC |loss|;  loss_sum: rows in any order, (M + 4) U_ACC sum|loss|, onto the prefill
      count:              exact"""
    M, C = x.shape
    x = _d(x)
    lab = labels.long()
    counts = (mask != 0) & (lab >= 0) & (lab < C)
    cf = counts.double()[:, None]
    onehot = torch.nn.functional.one_hot(torch.where(counts, lab, torch.zeros_like(lab)), C).double() * cf
    lse = torch.logsumexp(x, -1, keepdim=True)
    p = torch.exp(x - lse)
    ref = (p - onehot) * cf
    D = U_ACC * (2 * x.abs() + 3 * lse.abs() + 3 * math.log(C) + C + 8)
    e = (p * torch.expm1(D) + LIBM_REL * p + U_ACC * ref.abs()) * cf
    loss = (lse - (x * onehot).sum(-1, keepdim=True)) * cf
    e_loss = ((D * onehot).sum(-1, keepdim=True) + U_ACC * loss.abs()) * cf
    ref_sum, e_sum = with_beta(e_loss.sum() + (M + 4) * U_ACC * loss.abs().sum(), loss.sum(), 1.0,
                               torch.tensor(prefill[0], dtype=F64, device=x.device))
    return {"dlogits": _st(ref, e), "loss_sum": _st(ref_sum.reshape(1), e_sum.reshape(1)),
            "count": prefill[1] + float(counts.sum())}


# ------------------------------------------------------------------------------------------------------ the shapes
# (one list, used by the GPU test on the kernels and by the CPU test on the emulations and the seeded faults)
LN_M, ROW_H, P_DROP = (1, 5, 130), (1, 8, 63, 64, 65, 200), (0.0, 0.1)
EMBED = dict(B=3, S=5, vocab=11, types=2, max_pos=16, padding_idx=0)
PROMPT = dict(B=2, S_in=5, P=3, S=7, pos_offsets=(0, 4), src=(0, -1, 1, -3, 4, -2, 2), vocab=11, max_pos=16, padding_idx=0)
SOFTMAX = dict(B=2, heads=3, Sq=3, Skv=(1, 2, 63, 64, 65, 130), scales=(1.0, 0.125))
COLSUM_M, COLSUM_N = (1, 3, 4, 5, 130), (1, 63, 64, 65, 130)
FLAT_N = (1, 255, 257, 2 ** 21 + 3)
PLANTED = (0.0, -0.0, 30.0, -30.0, 100.0, -100.0)
ADD_MN = ((1, 1), (5, 13), (130, 65))
CONCAT = ((1, 1, 1), (5, 13, 64), (130, 65, 7))
REGIONS = ((1, 1, 1), (2, 49, 8), (3, 5, 65))
SAMPLE_GATE = ((1, 1, 1), (3, 5, 13), (2, 3, 5500))
LSTM = ((1, 1, 1), (2, 3, 5), (3, 4, 70))
GEMM_MN = ((1, 1), (127, 129), (128, 128), (129, 1), (1, 127))
GEMM_K = (1, 3, 15, 16, 17, 50)
GEMM_AB = ((1.0, 0.0), (0.5, 2.0))
CE_M, CE_C_LD = (1, 5, 130, 300), ((13, 13), (13, 16), (1, 4))
EPS_LN = 1e-12


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(F32)


def uniform(*shape, seed, lo=-6.0, hi=6.0, planted=()):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(F32)
    f = t.reshape(-1)
    if f.numel() > 37 * len(planted):          # (a tensor too small for all of them keeps its plain values)
        for j, v in enumerate(planted):
            f[j * 37] = v
    return t


def ln_inputs(M, H, mean100=False):
    """x, residual, gamma, beta, dy of a LayerNorm case and the index of its all-zero row (row 2; None if M < 3); with
    ``mean100`` rows of mean 100 and deviation 1 without residual."""
    x = rnd(M, H, seed=1) + (100.0 if mean100 else 0.0)
    r = torch.zeros(M, H) if mean100 else rnd(M, H, seed=2)
    z = 2 if M > 2 else None
    if z is not None:
        x[z] = 0.0
        r[z] = 0.0
    return x, r, rnd(H, seed=4) + 1.0, rnd(H, seed=5), rnd(M, H, seed=6), z


def softmax_mask(Skv, kind):
    """[2, Skv] additive mask: batch 0 open; batch 1 with its trailing third (at least one key) at -10000, or ("all") every key."""
    mk = torch.zeros(2, Skv)
    mk[1, (0 if kind == "all" else Skv - max(1, Skv // 3)):] = -10000.0
    return mk


def embed_ids(B, S, vocab):
    """ids [B, S] that include 0 (the padding id), vocab - 1, and id 3 in every sample"""
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, vocab, (B, S), generator=g)
    ids[:, 1 % S] = 3
    ids[0, 0] = 0
    ids[-1, S - 1] = 0
    ids[0, 2 % S] = vocab - 1
    return ids


def ce_inputs(M, C):
    """logits, labels, mask of a token-CE case: mask as in the bf16 test; on valid rows one label -100, one equal to C and one
    2^32 + 3 on the first valid rows (M = 1: only -100; M = 5: the first two, so that one valid row stays in range)."""
    x = rnd(M, C, seed=1, scale=3.0)
    labels = torch.randint(0, C, (M,), generator=torch.Generator().manual_seed(2))
    mask = (torch.arange(M) % 3 != 1).long()
    mask[0] = 1
    valid = torch.nonzero(mask)[:, 0]
    for row, v in zip(valid[:max(1, valid.numel() - 1)].tolist(), (-100, C, 2 ** 32 + 3)):
        labels[row] = v
    return x, labels, mask


# ------------------------------------------------------------------------------------------------------ comparison
def compare(outs, refs, what, verbose=False):
    """assert_within for every (reference, bound) pair of ``refs`` whose name is in ``outs``"""
    for name, rb in refs.items():
        if isinstance(rb, tuple) and name in outs and outs[name] is not None:
            assert_within(outs[name].reshape(rb[0].shape), rb[0], rb[1], "%s %s" % (what, name), verbose=verbose)


def same_bits(a, b, what):
    """bitwise equality of two f32 tensors (NaN payloads and the sign of zero included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    ne = a.view(torch.int32) != b.view(torch.int32)
    assert not bool(ne.any()), "%s: %d of %d elements differ bitwise" % (what, int(ne.sum()), ne.numel())


# ---------------------------------------------------------------------------------- dropout multipliers on the CPU
def cpu_dropout_mask(n, p, seed):
    """the flat-index multiplier of drop_mul: 1 / (1 - p) (in f32) where hash(idx) >= p 2^32, else 0; ones for p = 0"""
    import numpy as np
    from test_dropout_hash_cpu import icka_hash as _hash          # the numpy restatement of icka_hash (csrc/common.h)
    if p <= 0:
        return torch.ones(n)
    keep = _hash(seed & 0xffffffff, seed >> 32, np.arange(n, dtype=np.uint32)) >= np.uint32(int(p * 4294967296.0))
    return torch.from_numpy(keep).to(F32) * (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=F32)))


def cpu_attn_dropout_mask(rows, Skv, p, seed):
    """the pair form of drop_mul_key: element (row, key) takes the low (even key) or high (odd key) 16 bits of
    hash(row Skv + key / 2) against (p 2^32) >> 16"""
    import numpy as np
    from test_dropout_hash_cpu import icka_hash as _hash
    if p <= 0:
        return torch.ones(rows, Skv)
    r, k = np.meshgrid(np.arange(rows, dtype=np.uint32), np.arange(Skv, dtype=np.uint32), indexing="ij")
    with np.errstate(over="ignore"):
        h = _hash(seed & 0xffffffff, seed >> 32, (r * np.uint32(Skv) + (k >> np.uint32(1))).astype(np.uint32))
    t = np.uint32(int(p * 4294967296.0)) >> np.uint32(16)
    half = np.where(k & np.uint32(1), h >> np.uint32(16), h & np.uint32(0xffff))
    return torch.from_numpy(half >= t).to(F32) * (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=F32)))
