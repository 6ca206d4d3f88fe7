"""CPU restatement (vectorised, any float dtype) of the auxiliary training objective of the gated taggers, as the reference
computes it with labels (my_bert/gate_cl_modeling.py:1276-1395, my_bert/cl_modeling.py:1376-1382):

  * ``negatives(B, negative_rate)``: how many trailing samples become negatives (0 unless B > negative_rate);
  * ``swap(x, n)``: of the last n samples of x [B, ...], sample b0 + i and b0 + h + i trade places (b0 = B - n, h = n // 2);
  * ``cl_loss(t, v, temp, temp_lamb)``: the text <-> image InfoNCE loss of total_loss (:1276-1317);
  * ``crs_loss(crs, n)``: the two-class cross-entropy of the relevance logits against 1, 0 for the last n samples;
  * ``cl_grad(t, v, temp, temp_lamb)``: the closed-form gradient of cl_loss that csrc/objective.hip implements.

tests/golden/make_golden_objective.py asserts this module equals the reference on every fixture it writes."""
from __future__ import annotations

import torch


def negatives(B: int, negative_rate) -> int:
    return int(negative_rate) if (negative_rate is not None and B > negative_rate) else 0


def swap_index(B: int, n: int) -> torch.Tensor:
    idx = torch.arange(B)
    b0, h = B - n, n // 2
    idx[b0:b0 + h], idx[b0 + h:b0 + 2 * h] = torch.arange(b0 + h, b0 + 2 * h), torch.arange(b0, b0 + h)
    return idx


def swap(x: torch.Tensor, n: int) -> torch.Tensor:
    return x[swap_index(x.shape[0], n)]


def similarity(t: torch.Tensor, v: torch.Tensor, temp: float) -> torch.Tensor:
    """s_ij = cos(t_i, v_j) / temp (no epsilon in the norms, as the reference)."""
    return (t @ v.t()) / (t.norm(dim=1)[:, None] * v.norm(dim=1)[None, :]) / temp


def cl_loss(t: torch.Tensor, v: torch.Tensor, temp: float, temp_lamb: float) -> torch.Tensor:
    s = similarity(t, v, temp)
    d = s.diagonal()
    t2i = (torch.logsumexp(s, dim=1) - d).sum()
    i2t = (torch.logsumexp(s, dim=0) - d).sum()
    return (temp_lamb * t2i + (1 - temp_lamb) * i2t) / t.shape[0]


def crs_labels(B: int, n: int) -> torch.Tensor:
    y = torch.ones(B, dtype=torch.long)
    y[B - n:] = 0
    return y


def crs_loss(crs: torch.Tensor, n: int) -> torch.Tensor:
    return torch.nn.functional.cross_entropy(crs, crs_labels(crs.shape[0], n))


def cl_grad(t: torch.Tensor, v: torch.Tensor, temp: float, temp_lamb: float):
    """(dt, dv) of cl_loss:  G_ij = (1/B)[tl (softmax_row_i(j) - d_ij) + (1 - tl)(softmax_col_j(i) - d_ij)] / temp,
    dt^ = G v^, dv^ = G^T t^, dx = (dx^ - x^ (x^ . dx^)) / |x|."""
    B = t.shape[0]
    nt, nv = t.norm(dim=1, keepdim=True), v.norm(dim=1, keepdim=True)
    th, vh = t / nt, v / nv
    s = (th @ vh.t()) / temp
    eye = torch.eye(B, dtype=t.dtype)
    G = (temp_lamb * (torch.softmax(s, dim=1) - eye) + (1 - temp_lamb) * (torch.softmax(s, dim=0) - eye)) / (B * temp)
    dth, dvh = G @ vh, G.t() @ th
    dt = (dth - th * (th * dth).sum(1, keepdim=True)) / nt
    dv = (dvh - vh * (vh * dvh).sum(1, keepdim=True)) / nv
    return dt, dv
