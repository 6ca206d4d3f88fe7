"""Helpers of the element-wise tests of the gated-head kernels (csrc/fusion.hip: icka_sample_gate_*, icka_crs_*,
icka_cls_head_*) and of the contrastive objective (csrc/objective.hip: icka_contrastive_*); no test functions.  For every
entry point a function that takes the rounded values the kernel reads and returns {output: (float64 reference, bound)}.
The buffers and the comparison are those of tests/kernel_check.py, the objective's oracle is tests/objective_oracle.py
(tests/test_head_check_cpu.py asserts that the references here equal it); nothing here is a fitted constant.

Where the bounds come from
--------------------------
* U = U_ACC = 2^-23 per f32 operation (as tests/kernel_check.py charges f32 accumulation).
* An f32 sum of n terms in ANY order -- per-thread chunk order, the DPP wave tree, the block sum through LDS, the float
  atomics of ``dgate`` and ``crs``, a value already in the accumulator -- is charged (n + 4) U sum|terms|; the four spare
  roundings pay for what produced each term (a subtraction, a product) and what follows the sum (a scale, a division).
* 16-bit stores: ``stored(err, ref, dtype)``.
* The ``__expf`` sigmoid of the per-sample gates: SIGMOID_ABS = 2^-12 absolute, the REQUIREMENT tests/kernel_check.py
  states for the device's sigmoid.  It is absolute, so for a saturated gate (logit +-30) the bound of dgate is
  2^-12 sum|dout (a - c)| although the true g (1 - g) is 1e-13: loose there by nine orders of magnitude, and stated
  here for that reason.  A wrong sign, a dropped chunk or g in place of 1 - g move dgate by far more at plain logits.
* expf / log1pf / expm1f of the contrastive kernels: LIBM_REL = 2^-22 of the result (tests/exact_check.py), again a
  requirement on the device function.

The contrastive bounds, in the order they propagate (``contrastive_refs``)
-------------------------------------------------------------------------
1. Delta_ij on s_ij = cos(t_i, v_j) / temp: the dot product (D + 4) U sum_d |t_id v_jd|, each norm relative
   r_n = (D + 4) U / 2 + U (the sum of squares, halved by the square root, plus the root's rounding), three roundings for
   the product of the norms and the two divisions; all divided by temp.
2. m (the row / column maximum) moves by at most dmax_i = max_j Delta_ij.  L = log1p(sigma), sigma the sum of
   exp(s_j - m) over all but one maximal entry: every argument moves by at most 2 dmax (the excluded entry is exactly 0 on
   both sides, whichever member of a tie is excluded), so sigma by a factor within exp(+-2 dmax); each term carries
   U |s_j - m| + LIBM_REL relative, the sum (B + 4) U sigma, log1p LIBM_REL L.
3. loss term (m - s_ii) + L: where the diagonal is the maximum by more than 2 dmax the first part is exactly 0 in the
   kernel too, otherwise it is charged dmax + Delta_ii.  stats[0] is the (2B + 4) U sum of the weighted terms over B.
4. backward: x = (s - m) - L gets Delta + dmax + e_L (nothing but e_L on a dominant diagonal), p = exp(x) or expm1(x)
   moves by exp(x) expm1(e_x) + LIBM_REL |p|; G by the weighted sum of the two; g_j = G coef / n_j; the accumulation
   sum_j g_j x_j by sum_j e_g |x_j| + (B + 4) U sum_j |g_j x_j|; the projection x (x . dx) / n^2 by the (D + 4) U dot
   product; the final division by n by r_n + U.

Known looseness.  Delta is a worst-case bound that grows with D / temp, and step 4 multiplies it by the softmax: taken
as a relative L2 norm the whole-gradient bound is looser than the 1e-4 bar of tests/test_objective_gpu.py at every case
here except D = 8 at temp = 1 with up to 65 rows (tests/test_head_check_cpu.py asserts it either way; on the device the
kernels use about 1/40 of it).  Element-wise it still sees what that norm cannot: a single wrong entry of ws, the
relevance half, exchanged temp_lamb weights, exp for expm1 on the diagonal.  The dgate bound of the per-sample gates
charges the absolute 2^-12 on sum|dout (a - c)|, which outgrows the cancelling sum as sqrt(S H): relative to dgate it is
3e-4 at 8 elements per sample, 7e-3 at 120 and 0.33 at 16632, more for saturated gates.  The cls_head_bwd bound of du
charges the bf16 inputs gate and cross as exact and dx with its (C + 4) U accumulation.
"""
import torch

import objective_oracle as OO
from exact_check import LIBM_REL, compare, same_bits                                             # noqa: F401
from kernel_check import BF16, F16, F32, LIP_SIGMOID, SIGMOID_ABS, U_ACC, report, stored          # noqa: F401

U = U_ACC
F64 = torch.float64
FP16_MAX = 65504.0


def _d(t):
    return t.double()


def f32r(x):
    """the f32 value a float argument of the C ABI arrives as"""
    return float(torch.tensor(float(x), dtype=F32))


# ------------------------------------------------------------------------------------------------------- dispatch
SPLIT = 8                    # blocks per sample of the per-sample gate and crs forward kernels (256 threads, one chunk each)
CLS_TB, CLS_MAXC = 16, 16    # tokens per cls_head_bwd block (one slab each); classes per slab bias part
CLS_FWD_GRID_CAP, CRS_DGRAD_GRID_CAP = 512, 2048
CLS_LDS_BYTES = 44 * 1024
STAGE_FLOATS = 6144
MAX_B, MAX_D = 256, 4096


def nb_of(B):
    """the NB instantiation of contrastive_fwd_kernel: (B + 31) >> 5 rounded up to a power of two"""
    nb = (B + 31) >> 5
    return 1 if nb == 1 else 2 if nb == 2 else 4 if nb <= 4 else 8


def kc_of(NB):
    """K-chunk length of the LDS staging: 184, 88, 40, 16"""
    return (STAGE_FLOATS // (32 * NB + 1)) & ~7


def cc_of(C):
    return 13 if C <= 13 else 16


def gate_trips(S, H):
    """grid-stride trips of a gate / crs forward block over the S H / 8 chunks of its sample"""
    return -(-(S * (H // 8)) // (SPLIT * 256))


def cls_fwd_grid(M):
    return min((M + 7) // 8, CLS_FWD_GRID_CAP)


def cls_fwd_trips(M):
    return -(-M // (8 * cls_fwd_grid(M)))


def cls_fwd_ok(H, C):
    return H % 8 == 0 and 2 * H // 8 <= 256 and 1 <= C <= CLS_MAXC and C * 2 * H * 2 <= CLS_LDS_BYTES


def crs_dgrad_trips(B, S, H):
    n = B * S * (H // 8)
    return -(-n // (256 * min((n + 255) // 256, CRS_DGRAD_GRID_CAP)))


def cls_slabs(M):
    return (M + CLS_TB - 1) // CLS_TB


def cls_slab_floats(H, C):
    return C * 2 * H + CLS_MAXC


def contrastive_ws_floats(B):
    return B * B + 6 * B


# ---------------------------------------------------------------------------------------------------- sample gates
def gate_value(gate, mode):
    """g [B] and its error: mode 0 sigmoid(gate[b]); mode 1 sigmoid(gate[b, 1] - gate[b, 0]), whose argument costs U |d|
    (a quarter of it reaches g)."""
    gate = _d(gate)
    if mode == 0:
        return torch.sigmoid(gate.reshape(-1)), torch.full_like(gate.reshape(-1), SIGMOID_ABS)
    d = gate.reshape(-1, 2)[:, 1] - gate.reshape(-1, 2)[:, 0]
    return torch.sigmoid(d), SIGMOID_ABS + LIP_SIGMOID * U * d.abs()


def sample_gate_fwd_refs(a, c, gate, mode, B, S):
    """icka_sample_gate_fwd: out = g a + (1 - g) c (c NULL: g a), stored in bf16.  The kernel forms 1 - g from its own g, so
    an error of g moves out by |a - c| e_g; 1 - g, two products and an add: 3 U (|g a| + |(1 - g) c|)."""
    g, e_g = gate_value(gate, mode)
    g, e_g = g.repeat_interleave(S)[:, None], e_g.repeat_interleave(S)[:, None]
    a = _d(a)
    if c is None:
        ref = g * a
        return {"out": (ref, stored(a.abs() * e_g + U * ref.abs(), ref, BF16))}
    c = _d(c)
    ref = g * a + (1 - g) * c
    return {"out": (ref, stored((a - c).abs() * e_g + 3 * U * ((g * a).abs() + ((1 - g) * c).abs()), ref, BF16))}


def sample_gate_fwd_h_refs(a16, gate, mode, B, S):
    """icka_sample_gate_fwd_h: x = g a in f32; out = bf16(x) and out16 = fp16(clamp(x, +-65504)), BOTH from x."""
    g, e_g = gate_value(gate, mode)
    g, e_g = g.repeat_interleave(S)[:, None], e_g.repeat_interleave(S)[:, None]
    a = _d(a16)
    ref = g * a
    e = a.abs() * e_g + U * ref.abs()
    ref16 = ref.clamp(-FP16_MAX, FP16_MAX)
    return {"out": (ref, stored(e, ref, BF16)), "out16": (ref16, stored(e, ref16, F16))}


def sample_gate_bwd_refs(dout, a, c, gate, mode, B, S, prefill, with_dc=True):
    """icka_sample_gate_bwd: da = g d: |d| e_g + U |da|; dc = (1 - g) d: |d| (e_g + U) + U |dc| (mode 0 with c and dc);
    dgate += t, t = g (1 - g) sum d (a - c) over the n = S H elements of the sample.  The sum, the products with g and 1 - g
    and the atomics onto the prefilled word are one f32 sum of n + 1 terms: (n + 5) U (|prefill| + g (1 - g) sum|d (a - c)|);
    g (1 - g) moves by e_g (|1 - 2 g| + e_g).  Mode 1: dgate[b] = (-t, +t) on top of the prefill."""
    g, e_g = gate_value(gate, mode)
    d, a = _d(dout), _d(a)
    H = a.shape[1]
    gr, er = g.repeat_interleave(S)[:, None], e_g.repeat_interleave(S)[:, None]
    out = {"da": (gr * d, stored(d.abs() * er + U * (gr * d).abs(), gr * d, BF16))}
    diff = a if c is None else a - _d(c)
    if c is not None and with_dc:
        dc = (1 - gr) * d
        out["dc"] = (dc, stored(d.abs() * (er + U) + U * dc.abs(), dc, BF16))
    terms = (d * diff).reshape(B, S * H)
    acc, aabs = terms.sum(-1), terms.abs().sum(-1)
    gg = g * (1 - g)
    t = acc * gg
    pre = _d(prefill)
    if mode == 0:
        ref = pre.reshape(-1) + t
        e = (S * H + 5) * U * (pre.reshape(-1).abs() + gg * aabs) + aabs * e_g * ((1 - 2 * g).abs() + e_g)
    else:
        ref = pre.reshape(B, 2) + torch.stack([-t, t], -1)
        e = (S * H + 5) * U * (pre.reshape(B, 2).abs() + (gg * aabs)[:, None]) + (aabs * e_g * ((1 - 2 * g).abs() + e_g))[:, None]
    out["dgate"] = (ref, stored(e, ref, F32))
    return out


# ------------------------------------------------------------------------------------------------- crs classifier
def _crs_x(seq, cross, B, S, H):
    return torch.cat([_d(seq).reshape(B, S, H), _d(cross).reshape(B, S, H)], -1).reshape(B, S * 2 * H)


def crs_fwd_refs(seq, cross, W, bias, prefill, B, S, H):
    """icka_crs_fwd: crs[b, j] += sum_{s,k} cat(seq, cross)[b, s, k] W[j, s 2H + k] + bias_j (once): an f32 sum of the
    2 S H products, the bias and the prefilled word: (2 S H + 6) U sum|terms|."""
    x, w = _crs_x(seq, cross, B, S, H), _d(W).reshape(2, S * 2 * H)
    ref = _d(prefill).reshape(B, 2) + x @ w.t()
    ab = _d(prefill).reshape(B, 2).abs() + x.abs() @ w.abs().t()
    if bias is not None:
        ref, ab = ref + _d(bias), ab + _d(bias).abs()
    return {"crs": (ref, stored((2 * S * H + 6) * U * ab, ref, F32))}


def crs_bwd_refs(dcrs, seq, cross, W, B, S, H, accumulate, dW0, db0, with_w=True):
    """icka_crs_bwd: dseq / dcross [B S, H] bf16 = d0 W[0] + d1 W[1] (two products, one add: 3 U sum|.|); dW [2, S 2H] and
    dbias [2] (+)= sums over the B samples: (B + 5) U (sum|terms| + |prefill|).  ``with_w=False`` leaves dW / dbias out."""
    dcrs, w = _d(dcrs).reshape(B, 2), _d(W).reshape(2, S * 2 * H)
    dx = (dcrs @ w).reshape(B, S, 2, H)
    e = (3 * U * (dcrs.abs() @ w.abs())).reshape(B, S, 2, H)
    out = {"dseq": (dx[:, :, 0].reshape(B * S, H), stored(e[:, :, 0].reshape(B * S, H), dx[:, :, 0].reshape(B * S, H), BF16)),
           "dcross": (dx[:, :, 1].reshape(B * S, H), stored(e[:, :, 1].reshape(B * S, H), dx[:, :, 1].reshape(B * S, H), BF16))}
    if not with_w:
        return out
    x = _crs_x(seq, cross, B, S, H)
    dW, aW = dcrs.t() @ x, dcrs.abs().t() @ x.abs()
    db, ab = dcrs.sum(0), dcrs.abs().sum(0)
    if accumulate:
        dW, aW = dW + _d(dW0).reshape(2, -1), aW + _d(dW0).reshape(2, -1).abs()
        db, ab = db + _d(db0).reshape(2), ab + _d(db0).reshape(2).abs()
    out["dW"] = (dW, stored((B + 5) * U * aW, dW, F32))
    out["dbias"] = (db, stored((B + 5) * U * ab, db, F32))
    return out


# ------------------------------------------------------------------------------------------------ classifier head
def cls_head_fwd_refs(seq, gated, W, bias):
    """icka_cls_head_fwd(_h): logits f32 [M, C] = [seq | gated] . W^T + bias.  Products of two bf16 (or two fp16) values are
    exact in f32; the 2H-long sum over lanes, the LDS transpose and the two shuffles, plus the bias: (2H + 4) U sum|terms|."""
    x, w = torch.cat([_d(seq), _d(gated)], 1), _d(W)
    ref, ab = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        ref, ab = ref + _d(bias), ab + _d(bias).abs()
    return {"logits": (ref, stored((x.shape[1] + 4) * U * ab, ref, F32))}


def cls_head_bwd_refs(dl, seq, gated, gate, cross, W):
    """icka_cls_head_bwd, dl the logical [M, C]:
      dx = dl W [M, 2H]: (C + 4) U sum_c |dl_c W_c|;  dseq = bf16(dx[:, :H]);
      gated half: du = dx cross g (1 - g) with gate and cross EXACT as read: |cross g (1 - g)| e_dx + 4 U |du| (1 - g and
      three products); dcross = dx g: |g| e_dx + U |dcross|; both stored in bf16;
      slab k (tokens 16 k .. 16 k + nt): weight part [C, 2H] = dl^T x: (nt + 4) U sum_t |dl x|; bias part [16] = sum_t dl,
      (nt + 4) U sum_t |dl|, the entries c >= C exactly 0 (bound 0)."""
    dl, w = _d(dl), _d(W)
    M, C = dl.shape
    H = seq.shape[1]
    x = torch.cat([_d(seq), _d(gated)], 1)
    dx, e_dx = dl @ w, (C + 4) * U * (dl.abs() @ w.abs())
    out = {"dseq": (dx[:, :H], stored(e_dx[:, :H], dx[:, :H], BF16))}
    g, cr = _d(gate), _d(cross)
    k = cr * g * (1 - g)
    du = dx[:, H:] * k
    out["du"] = (du, stored(k.abs() * e_dx[:, H:] + 4 * U * du.abs(), du, BF16))
    dc = dx[:, H:] * g
    out["dcross"] = (dc, stored(g.abs() * e_dx[:, H:] + U * dc.abs(), dc, BF16))
    ns = cls_slabs(M)
    dlp = torch.zeros(ns * CLS_TB, CLS_MAXC, dtype=F64, device=dl.device)
    dlp[:M, :C] = dl
    xp = torch.zeros(ns * CLS_TB, 2 * H, dtype=F64, device=dl.device)
    xp[:M] = x
    dlp, xp = dlp.reshape(ns, CLS_TB, CLS_MAXC), xp.reshape(ns, CLS_TB, 2 * H)
    nt = torch.tensor([min(CLS_TB, M - CLS_TB * i) for i in range(ns)], dtype=F64, device=dl.device)
    sw = dlp.transpose(1, 2) @ xp
    aw = dlp.abs().transpose(1, 2) @ xp.abs()
    out["slab_w"] = (sw[:, :C], stored((nt[:, None, None] + 4) * U * aw[:, :C], sw[:, :C], F32))
    sb, ab = dlp.sum(1), dlp.abs().sum(1)
    eb = stored((nt[:, None] + 4) * U * ab, sb, F32)
    eb[:, C:] = 0.0
    out["slab_b"] = (sb, eb)
    out["_abs_w"], out["_abs_b"] = aw[:, :C].sum(0), ab[:, :C].sum(0)
    return out


def cls_wiring_refs(refs, accumulate, dW0, db0):
    """dW [C, 2H] and db [C] (+)= the sum of the slabs (K.slab_reduction through K.gemm_grouped): the per-slab bounds add,
    and the sum over the ns slabs and the prefilled value costs (ns + 5) U (sum|terms| + |prefill|)."""
    sw, ew = refs["slab_w"]
    sb, eb = refs["slab_b"]
    ns, C = sw.shape[0], sw.shape[1]
    dW, db = sw.sum(0), sb[:, :C].sum(0)
    aW, ab = refs["_abs_w"], refs["_abs_b"]
    if accumulate:
        dW, aW = dW + _d(dW0), aW + _d(dW0).abs()
        db, ab = db + _d(db0), ab + _d(db0).abs()
    return {"dW": (dW, stored(ew.sum(0) + (ns + 5) * U * aW, dW, F32)),
            "db": (db, stored(eb[:, :C].sum(0) + (ns + 5) * U * ab, db, F32))}


# ---------------------------------------------------------------------------------------------------- contrastive
def _lse_parts(S, Delta):
    """per row of S: see steps 2 and 3 of the module docstring"""
    B = S.shape[0]
    m, jm = S.max(dim=1)
    dmax = Delta.max(dim=1).values
    x = S - m[:, None]
    keep = torch.ones_like(S, dtype=torch.bool)
    keep[torch.arange(B, device=S.device), jm] = False
    ex = torch.where(keep, torch.exp(x), torch.zeros_like(x))
    sigma = ex.sum(1)
    L = torch.log1p(sigma)
    e_sigma = (ex * (U * x.abs() + LIBM_REL)).sum(1) + (B + 4) * U * sigma
    e_L = (sigma * torch.expm1(2 * dmax) + e_sigma) / (1 + sigma * torch.exp(-2 * dmax)) + LIBM_REL * L
    if B > 1:
        top = S.topk(2, dim=1).values
        strict = (S.diagonal() == m) & ((top[:, 0] - top[:, 1]) > 2 * dmax)
    else:
        strict = torch.ones(1, dtype=torch.bool, device=S.device)
    md = m - S.diagonal()
    e_md = torch.where(strict, torch.zeros_like(md), dmax + Delta.diagonal() + U * md.abs())
    term = md + L
    return dict(m=m, dmax=dmax, L=L, e_L=e_L, strict=strict, term=term, e_term=e_md + e_L + U * term.abs())


def _softmax_minus_eye(S, Delta, p):
    """[B, B] p_ij - d_ij of the rows of S as the backward forms it, and its error (step 4)"""
    B = S.shape[0]
    eye = torch.eye(B, dtype=torch.bool, device=S.device)
    sm = S - p["m"][:, None]
    x = sm - p["L"][:, None]
    e_x = torch.where(eye & p["strict"][:, None], torch.zeros_like(x), Delta + p["dmax"][:, None]) + p["e_L"][:, None] + \
        2 * U * (sm.abs() + x.abs())
    pr = torch.where(eye, torch.expm1(x), torch.exp(x))
    return pr, torch.exp(x) * torch.expm1(e_x) + LIBM_REL * pr.abs()


def _proj(G, e_G, own, other, n_own, n_other, r_n, coef):
    """rows r: dx_r = (acc - x proj) / n, acc = sum_j g_j other_j, g_j = G_rj coef / n_other_j, proj = (x . acc) / n^2"""
    B, D = own.shape
    g = G * coef / n_other[None, :]
    e_g = (e_G + G.abs() * (r_n + 5 * U)) * abs(coef) / n_other[None, :]
    acc = g @ other
    e_acc = e_g @ other.abs() + (B + 4) * U * (g.abs() @ other.abs())
    dot = (own * acc).sum(1)
    e_dot = (own.abs() * e_acc).sum(1) + (D + 4) * U * (own * acc).abs().sum(1)
    n2 = n_own * n_own
    proj = dot / n2
    e_proj = e_dot / n2 + proj.abs() * (2 * r_n + 2 * U)
    out = (acc - own * proj[:, None]) / n_own[:, None]
    e = (e_acc + own.abs() * e_proj[:, None] + 2 * U * (acc.abs() + (own * proj[:, None]).abs())) / n_own[:, None] + \
        out.abs() * (r_n + U)
    return out, stored(e, out, F32)


def crs_ce_refs(crs, n_neg, dcrs_loss):
    """the relevance cross-entropy half: stats[1] = mean_b (lse(crs_b) - crs_b[y_b]), y_b = 0 for the last n_neg samples else
    1; dcrs = (softmax - onehot) dcrs_loss / B.  lse = max + log1p(exp(min - max))."""
    c = _d(crs).reshape(-1, 2)
    B = c.shape[0]
    y = OO.crs_labels(B, n_neg).to(c.device)
    mx, mn = c.max(1).values, c.min(1).values
    xx = mn - mx
    ex = torch.exp(xx)
    lp = torch.log1p(ex)
    l = mx + lp
    term = l - c.gather(1, y[:, None])[:, 0]
    rel = U * xx.abs() + LIBM_REL
    e_term = ex * rel / (1 + ex) + LIBM_REL * lp + U * l.abs() + U * term.abs()
    s1 = term.sum() / B
    e_s1 = (e_term.sum() + (B + 4) * U * term.abs().sum()) / B
    p = torch.softmax(c, 1)
    dc = float(dcrs_loss) / B
    onehot = torch.nn.functional.one_hot(y, 2).to(F64)
    ref = (p - onehot) * dc
    e_p = p * (1 - p) * rel[:, None] + 3 * U * p
    e = (e_p + U * (p - onehot).abs()) * abs(dc) + 2 * U * ref.abs()
    return (s1, stored(e_s1, s1, F32)), (ref, stored(e, ref, F32))


def contrastive_refs(t, v, temp, temp_lamb, crs=None, n_neg=0, dcl=1.0, dcrs_loss=1.0):
    """icka_contrastive_fwd + icka_contrastive_bwd of rows t, v [B, D] (any of the three dtypes, read exactly) ->
    {"stats" [2], "ws" [B B + 6 B] (S, m_row, m_col, L_row, L_col, |t|, |v|), "dt", "dv" [B, D], "dcrs" [B, 2] with crs}.
    temp, temp_lamb, dcl and dcrs_loss are taken as the f32 values the kernels read."""
    B, D = t.shape
    temp, tl, dcl = f32r(temp), f32r(temp_lamb), f32r(dcl)
    t64, v64 = _d(t), _d(v)
    nt, nv = t64.norm(dim=1), v64.norm(dim=1)
    r_n = (D + 4) * U / 2 + U
    nn = nt[:, None] * nv[None, :]
    cosv = (t64 @ v64.t()) / nn
    S = cosv / temp
    Delta = ((D + 4) * U * (t64.abs() @ v64.abs().t()) / nn + cosv.abs() * (2 * r_n + 3 * U)) / temp
    row, col = _lse_parts(S, Delta), _lse_parts(S.t(), Delta.t())
    wr, wc = tl * row["term"], (1 - tl) * col["term"]
    s0 = (wr + wc).sum() / B
    e_s0 = ((tl * row["e_term"] + (1 - tl) * col["e_term"]).sum() + (2 * B + 4) * U * (wr.abs() + wc.abs()).sum()) / B
    stats = [(s0, stored(e_s0, s0, F32))]
    out = {}
    if crs is not None:
        s1, out["dcrs"] = crs_ce_refs(crs, n_neg, f32r(dcrs_loss))
        stats.append(s1)
    else:
        stats.append((torch.zeros((), dtype=F64, device=S.device), torch.zeros((), dtype=F64, device=S.device)))
    out["stats"] = (torch.stack([s[0] for s in stats]), torch.stack([s[1] for s in stats]))
    ws_ref = [S.reshape(-1), row["m"], col["m"], row["L"], col["L"], nt, nv]
    ws_err = [Delta.reshape(-1), row["dmax"], col["dmax"], row["e_L"], col["e_L"], nt * r_n, nv * r_n]
    out["ws"] = (torch.cat(ws_ref), torch.cat([stored(e, r, F32) for e, r in zip(ws_err, ws_ref)]))
    pr, e_pr = _softmax_minus_eye(S, Delta, row)
    pc, e_pc = _softmax_minus_eye(S.t(), Delta.t(), col)
    pc, e_pc = pc.t(), e_pc.t()
    G = tl * pr + (1 - tl) * pc
    e_G = tl * e_pr + (1 - tl) * e_pc + 3 * U * (tl * pr.abs() + (1 - tl) * pc.abs())
    coef = dcl / (B * temp)
    out["dt"] = _proj(G, e_G, t64, v64, nt, nv, r_n, coef)
    out["dv"] = _proj(G.t(), e_G.t(), v64, t64, nv, nt, r_n, coef)
    return out


# ---------------------------------------------------------------------------------- the cases both test files run
GATE_SHAPES = ((1, 1, 8), (3, 5, 24), (2, 33, 504))       # (B, S, H); the last: 2079 chunks > 8 * 256
CRS_SHAPES = ((1, 1, 8), (3, 5, 24))
CRS_BIG = (8, 128, 4104)                                   # 525312 chunks > 2048 * 256
CLS_FWD_M, CLS_FWD_H, CLS_FWD_C = (1, 2, 9), (8, 24, 768, 1024), (1, 11, 13, 16)   # (C = 11: the 44 KiB LDS limit at H = 1024)
CLS_FWD_BIG = (4099, 8)                                    # (M, H): 513 passes of 8 rows over 512 blocks, an odd last pair
CLS_BWD_M, CLS_BWD_C, CLS_BWD_H = (1, 15, 16, 17, 19), (1, 13, 14, 16), (8, 24, 1024)
CL_B = (1, 2, 32, 33, 64, 65, 128, 129, 256)
CL_TEMPS, CL_TLS = (0.05, 1.0), (0.0, 0.7, 1.0)
CL_DTYPES = (F32, BF16, F16)


def cl_D(B):
    kc = kc_of(nb_of(B))
    return (8, kc, kc + 8, 2 * kc - 8)


def cl_cases():
    """(B, D, temp, temp_lamb, n_neg or None (crs NULL)): every B with the four D of its NB; two (temp, temp_lamb) pairs per
    (B, D), rotating so that every pair and every n_neg of {0, 1, B - 1, B} meets every NB; crs NULL on every fourth."""
    out, i = [], 0
    for B in CL_B:
        for D in cl_D(B):
            nneg = (0, 1, B - 1, B)[i % 4]
            out.append((B, D, CL_TEMPS[0], CL_TLS[i % 3], nneg))
            out.append((B, D, CL_TEMPS[1], CL_TLS[(i + 1) % 3], None if i % 4 == 3 else (0, 1, B - 1, B)[(i + 1) % 4]))
            i += 1
    return out


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def gate_inputs(B, S, H, mode, saturated=False):
    """a, c, dout bf16 [B S, H]; gate f32 [B] (mode 0) or [B, 2]; prefill of dgate.  ``saturated``: logits of +30 and -30 on the
    first two samples (mode 1: a difference of +-30)."""
    a, c, d = (rnd(B * S, H, seed=s, dtype=BF16) for s in (1, 2, 3))
    gate = rnd(B, seed=4, scale=1.5) if mode == 0 else rnd(B, 2, seed=5, scale=1.5)
    if saturated:
        if mode == 0:
            gate[0], gate[1 % B] = 30.0, -30.0
        else:
            gate[0, 0], gate[0, 1] = -15.0, 15.0
            gate[1 % B, 0], gate[1 % B, 1] = 15.0, -15.0
    pre = rnd(*gate.shape, seed=6)
    return a, c, d, gate, pre


def gate_h_inputs(B, S, H, mode):
    """a16 fp16 [B S, H] with +-65504 planted in sample 0, whose gate is saturated (g = 1 in f32): the product sits at the
    fp16 limit; the other samples have g in (0.5, 1) so that a second rounding through bf16 would leave the fp16 bound."""
    a = rnd(B * S, H, seed=7, scale=3.0, dtype=F16)
    a[0, 0], a[0, H - 1] = FP16_MAX, -FP16_MAX
    gate = rnd(B, seed=8).abs() + 0.5 if mode == 0 else torch.stack([-rnd(B, seed=8).abs() - 0.5, rnd(B, seed=9).abs()], 1)
    if mode == 0:
        gate[0] = 30.0
    else:
        gate[0, 0], gate[0, 1] = -15.0, 15.0
    return a, gate.to(F32)


def crs_inputs(B, S, H):
    seq, cross = rnd(B * S, H, seed=11, dtype=BF16), rnd(B * S, H, seed=12, dtype=BF16)
    W = rnd(2, S * 2 * H, seed=13, scale=0.1, dtype=BF16)
    return seq, cross, W, rnd(2, seed=14), rnd(B, 2, seed=15), rnd(B, 2, seed=16), rnd(2, S * 2 * H, seed=17), rnd(2, seed=18)


def cls_inputs(M, H, C, dtype=BF16):
    """seq, gated, W, bias, dl [M, C], gate (in (0, 1)), cross"""
    seq, gated = rnd(M, H, seed=21, dtype=dtype), rnd(M, H, seed=22, dtype=dtype)
    W = rnd(C, 2 * H, seed=23, scale=0.1, dtype=dtype)
    gate = torch.sigmoid(rnd(M, H, seed=26, scale=2.0)).to(BF16)
    return seq, gated, W, rnd(C, seed=24), rnd(M, C, seed=25, dtype=BF16), gate, rnd(M, H, seed=27, dtype=BF16)


def cl_inputs(B, D, dtype, tie=False):
    """correlated pairs (a non-trivial softmax); ``tie``: rows 0 and 1 of t and of v identical -- S[0, 0] == S[0, 1] bitwise"""
    g = torch.Generator().manual_seed(B * 7919 + D)
    t = torch.randn(B, D, generator=g).to(dtype)
    v = (0.5 * torch.randn(B, D, generator=g) + 0.3 * t.float()).to(dtype)
    if tie and B > 1:
        t[1], v[1] = t[0], v[0]
    crs = torch.randn(B, 2, generator=g) * 2.0
    return t, v, crs
