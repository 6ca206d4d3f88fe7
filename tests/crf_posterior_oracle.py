"""Helpers of the CRF-posterior tests (no test functions): a float64 restatement of the definitions of ``icka_crf_posterior``
(include/icka_hip.h) with plain loops over the on-positions, and an enumeration of all paths for tiny cases.

Per sample the on-positions are position 0 and every t >= 1 with mask[t] != 0; the model is the chain over them,
score(y) = start[y_0] + x_0[y_0] + sum_{i>=1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}].  A path has one tag per
on-position.  Span posterior of path positions s .. e-1: alpha_s[y_s] prod_{i=s+1}^{e-1} psi_i(y_{i-1}, y_i) beta_{e-1}[y_{e-1}] / Z."""
import itertools
import math

import torch

from icka_amd.metrics import chunks

F64 = torch.float64


def on_positions(mask_row, S):
    return [0] + [t for t in range(1, S) if mask_row is None or bool(mask_row[t])]


def _lse(v):
    return float(torch.logsumexp(torch.as_tensor(v, dtype=F64), 0))


class Sample(object):
    """Forward-backward of ONE sample in float64: ``pos``, ``L``, ``log_z``, ``marg`` [S, C] (zeros at off-positions)."""

    def __init__(self, e, mask_row, start, end, trans):
        self.S, self.C = e.shape
        self.pos = on_positions(mask_row, self.S)
        self.L = L = len(self.pos)
        C = self.C
        self.x = x = [e[t].to(F64) for t in self.pos]
        self.start, self.end, self.trans = start.to(F64), end.to(F64), trans.to(F64)
        T = self.trans
        al = [self.start + x[0]]
        for i in range(1, L):
            al.append(torch.logsumexp(al[i - 1][:, None] + T, 0) + x[i])
        be = [None] * L
        be[L - 1] = self.end
        for i in range(L - 1, 0, -1):
            be[i - 1] = torch.logsumexp(T + (x[i] + be[i])[None, :], 1)
        self.alpha, self.beta = al, be
        self.log_z = float(torch.logsumexp(al[L - 1] + self.end, 0))
        self.marg = torch.zeros(self.S, C, dtype=F64)
        for i, t in enumerate(self.pos):
            self.marg[t] = torch.exp(al[i] + be[i] - self.log_z)

    def score(self, path):
        assert len(path) == self.L
        s = float(self.start[path[0]]) + float(self.x[0][path[0]])
        for i in range(1, self.L):
            s += float(self.trans[path[i - 1], path[i]]) + float(self.x[i][path[i]])
        return s + float(self.end[path[-1]])

    def seq_logp(self, path):
        return self.score(path) - self.log_z

    def token_conf(self, path):
        return [float(self.marg[t, path[i]]) for i, t in enumerate(self.pos)]

    def span(self, path, s, e):
        v = float(self.alpha[s][path[s]]) + float(self.beta[e - 1][path[e - 1]]) - self.log_z
        for i in range(s + 1, e):
            v += float(self.trans[path[i - 1], path[i]]) + float(self.x[i][path[i]])
        return math.exp(v)

    def entities(self, path, id_to_label, default="O"):
        """[(type name, start, end, posterior)] of the chunks of ``path`` (``metrics.chunks``)."""
        return [(ty, s, e, self.span(path, s, e)) for ty, s, e in chunks(path, id_to_label, default)]


def enumerate_sample(e, mask_row, start, end, trans, path, spans):
    """All C^L paths of one sample: (log Z, marginals [S, C], seq_logp of ``path``, [P(tags s..e-1 equal the path's)])."""
    S, C = e.shape
    pos = on_positions(mask_row, S)
    L = len(pos)
    scores = {}
    for y in itertools.product(range(C), repeat=L):
        s = float(start[y[0]]) + float(e[pos[0], y[0]])
        for i in range(1, L):
            s += float(trans[y[i - 1], y[i]]) + float(e[pos[i], y[i]])
        scores[y] = s + float(end[y[-1]])
    log_z = _lse(list(scores.values()))
    marg = [[0.0] * C for _ in range(S)]
    sp = [0.0] * len(spans)
    for y, s in scores.items():
        p = math.exp(s - log_z)
        for i, t in enumerate(pos):
            marg[t][y[i]] += p
        for n, (a, b) in enumerate(spans):
            if list(y[a:b]) == list(path[a:b]):
                sp[n] += p
    return log_z, torch.tensor(marg, dtype=F64), scores[tuple(path)] - log_z, sp


def batch(e, mask, start, end, trans):
    """[Sample] of a batch-first float tensor e [B, S, C] and a mask [B, S] (or None)."""
    e, start, end, trans = e.double(), start.double(), end.double(), trans.double()
    return [Sample(e[b], None if mask is None else mask[b], start, end, trans) for b in range(e.shape[0])]
