"""Helpers of the constrained-CRF tests (no test functions): a float64 restatement of the definitions of
``icka_crf_constrained_llh`` / ``_grad`` / ``_decode`` (include/icka_hip.h) with plain loops over the on-positions, and an
enumeration of all paths for tiny cases.

The chain is ``crf_posterior_oracle.Sample``'s.  ``allowed`` is an int64 bit set per position (bit j = tag j); A_i is the set at
on-position i; Z_A sums exp score(y) over the paths with y_i in A_i for every i.  A sample with an empty A_i is infeasible.
Decoding takes the first maximum over the allowed tags at both places (the previous tag of every step, the final tag), which
among the optimal paths is the one whose reversed tag sequence is lexicographically smallest."""
import itertools
import math

import torch

import crf_posterior_oracle as PO

F64 = torch.float64
NEG = float("-inf")


def tag_set(word, C):
    """the tags below C whose bit is set in the (signed 64-bit) integer ``word``"""
    w = int(word)
    return [j for j in range(C) if (w >> j) & 1]


def _masked(v, tags):
    out = torch.full_like(v, NEG)
    if tags:
        out[tags] = v[tags]
    return out


class Sample(object):
    """ONE sample in float64.  Free lattice: ``free`` (a ``crf_posterior_oracle.Sample``), ``log_z``, ``marg`` [S, C], ``pair``
    [C, C] (pair marginals summed over i >= 1), ``first`` / ``last`` [C] (marginals at i = 0 / L-1).  Restricted lattice, when
    ``feasible``: ``log_za``, ``marg_a``, ``pair_a``, ``first_a``, ``last_a``; an infeasible sample has ``log_za = llh = -inf``
    and zeros there.  ``llh = log_za - log_z``; ``d_e = marg_a - marg`` [S, C] (zeros for an infeasible sample)."""

    def __init__(self, e, mask_row, allowed_row, start, end, trans):
        self.free = f = PO.Sample(e, mask_row, start, end, trans)
        self.S, self.C, self.pos, self.L = f.S, f.C, f.pos, f.L
        L, C, T, x = f.L, f.C, f.trans, f.x
        self.sets = [tag_set(allowed_row[t], C) for t in f.pos]
        self.feasible = all(len(a) > 0 for a in self.sets)
        self.log_z, self.marg = f.log_z, f.marg
        self.pair = torch.zeros(C, C, dtype=F64)
        for i in range(1, L):
            self.pair += torch.exp(f.alpha[i - 1][:, None] + T + (x[i] + f.beta[i])[None, :] - f.log_z)
        self.first, self.last = f.marg[f.pos[0]].clone(), f.marg[f.pos[L - 1]].clone()
        self.marg_a = torch.zeros(f.S, C, dtype=F64)
        self.pair_a = torch.zeros(C, C, dtype=F64)
        self.first_a, self.last_a = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
        self.log_za = self.llh = NEG
        if self.feasible:
            al = [_masked(f.start + x[0], self.sets[0])]
            for i in range(1, L):
                al.append(_masked(torch.logsumexp(al[i - 1][:, None] + T, 0) + x[i], self.sets[i]))
            be = [None] * L
            be[L - 1] = f.end
            for i in range(L - 1, 0, -1):
                be[i - 1] = torch.logsumexp(T + _masked(x[i] + be[i], self.sets[i])[None, :], 1)
            self.log_za = float(torch.logsumexp(al[L - 1] + f.end, 0))
            self.llh = self.log_za - self.log_z
            for i, t in enumerate(f.pos):
                self.marg_a[t] = torch.exp(al[i] + be[i] - self.log_za)
            for i in range(1, L):
                self.pair_a += torch.exp(al[i - 1][:, None] + T + _masked(x[i] + be[i], self.sets[i])[None, :] - self.log_za)
            self.first_a, self.last_a = self.marg_a[f.pos[0]].clone(), self.marg_a[f.pos[L - 1]].clone()
        self.d_e = (self.marg_a - self.marg) if self.feasible else torch.zeros(f.S, C, dtype=F64)

    def score(self, path):
        return self.free.score(path)

    def viterbi(self):
        """(path, score) of the best path inside the sets with the first-maximum tie rule, or (None, -inf)."""
        if not self.feasible:
            return None, NEG
        f, L, C = self.free, self.L, self.C
        T = f.trans.tolist()
        x = [r.tolist() for r in f.x]
        st, en = f.start.tolist(), f.end.tolist()
        sc = [(st[j] + x[0][j]) if j in self.sets[0] else NEG for j in range(C)]
        bp = []
        for i in range(1, L):
            nxt, row = [], []
            for j in range(C):
                m, am = NEG, 0
                for k in range(C):
                    v = sc[k] + T[k][j]
                    if v > m:
                        m, am = v, k
                row.append(am)
                nxt.append((m + x[i][j]) if j in self.sets[i] else NEG)
            bp.append(row)
            sc = nxt
        fin = [sc[j] + en[j] for j in range(C)]
        bt = 0
        for j in range(1, C):
            if fin[j] > fin[bt]:
                bt = j
        best = fin[bt]
        path = [bt]
        for i in range(L - 1, 0, -1):
            bt = bp[i - 1][bt]
            path.append(bt)
        return path[::-1], best


def batch(e, mask, allowed, start, end, trans):
    """[Sample] of a batch-first float tensor e [B, S, C], a mask [B, S] (or None) and int64 bit sets [B, S]."""
    e, start, end, trans = e.double(), start.double(), end.double(), trans.double()
    return [Sample(e[b], None if mask is None else mask[b], allowed[b], start, end, trans) for b in range(e.shape[0])]


def param_grads(samples, weights=None):
    """Expected-count tensors of ``sum_b w_b llh_b``: ((G_A start, end, trans), (G start, end, trans)), each the weighted sum
    over the FEASIBLE samples of the restricted / the free marginals.  The gradient is G_A - G, element by element."""
    C = samples[0].C
    ga = [torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64), torch.zeros(C, C, dtype=F64)]
    gf = [torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64), torch.zeros(C, C, dtype=F64)]
    for b, s in enumerate(samples):
        if not s.feasible:
            continue
        w = 1.0 if weights is None else float(weights[b])
        for acc, parts in ((ga, (s.first_a, s.last_a, s.pair_a)), (gf, (s.first, s.last, s.pair))):
            for a, p in zip(acc, parts):
                a += w * p
    return ga, gf


def enumerate_sample(e, mask_row, allowed_row, start, end, trans):
    """All C^L paths of one sample -> dict(log_z, log_za, marg, marg_a [S, C], pair, pair_a [C, C], best = (path, score) by the
    tie rule or (None, -inf), feasible)."""
    S, C = e.shape
    pos = PO.on_positions(mask_row, S)
    L = len(pos)
    sets = [set(tag_set(allowed_row[t], C)) for t in pos]
    scores = {}
    for y in itertools.product(range(C), repeat=L):
        s = float(start[y[0]]) + float(e[pos[0], y[0]])
        for i in range(1, L):
            s += float(trans[y[i - 1], y[i]]) + float(e[pos[i], y[i]])
        scores[y] = s + float(end[y[-1]])
    inside = {y: s for y, s in scores.items() if all(y[i] in sets[i] for i in range(L))}
    lse = lambda v: float(torch.logsumexp(torch.tensor(v, dtype=F64), 0)) if v else NEG
    log_z, log_za = lse(list(scores.values())), lse(list(inside.values()))

    def marginals(table, lz):
        marg = [[0.0] * C for _ in range(S)]
        pair = [[0.0] * C for _ in range(C)]
        for y, s in table.items():
            p = math.exp(s - lz)
            for i, t in enumerate(pos):
                marg[t][y[i]] += p
            for i in range(1, L):
                pair[y[i - 1]][y[i]] += p
        return torch.tensor(marg, dtype=F64), torch.tensor(pair, dtype=F64)

    marg, pair = marginals(scores, log_z)
    marg_a, pair_a = marginals(inside, log_za) if inside else (torch.zeros(S, C, dtype=F64), torch.zeros(C, C, dtype=F64))
    best = (None, NEG)
    if inside:
        top = max(inside.values())
        y = min((y for y, s in inside.items() if s == top), key=lambda y: y[::-1])
        best = (list(y), top)
    return {"log_z": log_z, "log_za": log_za, "marg": marg, "marg_a": marg_a, "pair": pair, "pair_a": pair_a, "best": best,
            "feasible": bool(inside)}


# ---------------------------------------------------------------------------------------------------- test inputs
def every(C):
    return -1 if C == 64 else (1 << C) - 1


def _signed(w):
    return w - (1 << 64) if w >= (1 << 63) else w


def allowed_sets(kind, B, S, C, seed, path=None):
    """int64 [B, S] bit sets: ``all`` | ``random`` (non-empty) | ``partial`` (about half the positions a singleton of ``path``,
    the rest every tag) | ``single`` (the singletons of ``path`` [B, S])."""
    g = torch.Generator().manual_seed(seed)
    if kind == "all":
        return torch.full((B, S), every(C), dtype=torch.int64)
    if kind == "random":
        bits = torch.rand(B, S, C, generator=g) < 0.5
        keep = torch.randint(0, C, (B, S), generator=g)
        bits.scatter_(2, keep[..., None], True)
        rows = [[_signed(sum(1 << j for j in range(C) if bits[b, t, j])) for t in range(S)] for b in range(B)]
        return torch.tensor(rows, dtype=torch.int64)
    if path is None:
        path = torch.randint(0, C, (B, S), generator=g)
    one = torch.tensor([[_signed(1 << int(path[b, t])) for t in range(S)] for b in range(B)], dtype=torch.int64)
    if kind == "single":
        return one
    if kind == "partial":
        known = torch.rand(B, S, generator=g) < 0.5
        return torch.where(known, one, torch.full_like(one, every(C)))
    raise ValueError(kind)


def make_mask(kind, B, S, seed):
    """None | ``prefix`` (lens[0] = S, lens[1] = 1) | ``holes`` (random, position 0 on) | ``first_off`` (holes with mask[b,0] = 0)."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    if kind == "prefix":
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0] = S
        if B > 1:
            lens[1] = 1
        return (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64)
    m = (torch.rand(B, S, generator=g) < 0.6).to(torch.int64)
    m[0, :] = 1
    if B > 1:
        m[1, 1:] = 0
    m[:, 0] = 0 if kind == "first_off" else 1
    return m


def inputs(B, S, C, seed, grid=None):
    """(e, start, end, trans) f32: normal draws (emissions x 2), or on a grid of multiples of 1/8 in [-16, 16], where every f32
    sum of a path is exact: ``fine`` (all of the grid) or ``coarse`` (the integers -2 .. 2: ties at almost every step)."""
    g = torch.Generator().manual_seed(seed)
    if grid == "fine":
        draw = lambda *shape: torch.randint(-128, 129, shape, generator=g).float() / 8.0
        return draw(B, S, C), draw(C), draw(C), draw(C, C)
    if grid == "coarse":
        draw = lambda *shape: torch.randint(-2, 3, shape, generator=g).float()
        return draw(B, S, C), draw(C), draw(C), draw(C, C)
    return (torch.randn(B, S, C, generator=g) * 2.0, torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5,
            torch.randn(C, C, generator=g) * 0.5)
