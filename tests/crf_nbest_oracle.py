"""Float64 restatement of N-best CRF decoding as include/icka_hip.h defines it for icka_crf_nbest (no test functions).

The chain runs over the on-positions of a sample (position 0 and every t >= 1 with mask != 0), x_0 .. x_{L-1} the emission
rows at them:  score(y) = start[y_0] + x_0[y_0] + sum_{i >= 1} (trans[y_{i-1}, y_i] + x_i[y_i]) + end[y_{L-1}].  The result
of a sample is its min(K, C^L) distinct paths of highest score by non-increasing score; among paths of equal score the one
whose REVERSED tag sequence is lexicographically smaller comes first.

``nbest_sample`` is a K-list Viterbi whose every selection is a STABLE sort of the candidates laid out in ascending
(previous tag, previous rank) -- at the end ascending (tag, rank) -- which produces exactly that order; ``brute`` sorts all
C^L paths by (-score, reversed path) and is what test_crf_nbest_cpu.py holds the Viterbi against.

Grids on which every partial sum of a score is exact in f32 in any association (so that a device result must equal the
float64 one bit for bit):
  coarse  every parameter and emission a multiple of 1/2 in [-2, 2]: ties everywhere; |sum| <= 2 (2 S + 1) needs 13 bits at
          S = 512
  fine    emissions multiples of 2^-10 in [-4, 4], start / end / transitions multiples of 2^-10 in [-1, 1]:
          |sum| <= 5 S + 2 < 4096 at S = 512, times 2^10: 22 bits of the 24 an f32 holds
"""
import itertools

import numpy as np
import torch

BRUTE_MAX_PATHS = 20000


def on_positions(mask_row, S):
    return [0] + [t for t in range(1, S) if mask_row is None or bool(mask_row[t])]


def score(x, start, end, trans, path):
    """Float64 score of ``path`` (one tag per row of x [L, C])."""
    s = start[path[0]] + x[0, path[0]]
    for i in range(1, len(path)):
        s += trans[path[i - 1], path[i]] + x[i, path[i]]
    return float(s + end[path[-1]])


def nbest_sample(x, start, end, trans, K):
    """x [L, C], start / end [C], trans [C, C] float64 numpy -> [(score, path)] of the min(K, C^L) best paths, in order."""
    L, C = x.shape
    sc = np.full((C, K), -np.inf)
    sc[:, 0] = start + x[0]
    bps = []
    for i in range(1, L):
        cand = (sc[:, :, None] + trans[:, None, :]).reshape(C * K, C)     # row p * K + r: ascending (previous tag, rank)
        idx = np.argsort(-cand, axis=0, kind="stable")[:K]
        sc = np.take_along_axis(cand, idx, 0).T + x[i][:, None]
        bps.append(idx.T.copy())
    fin = (sc + end[:, None]).reshape(-1)                                   # index c * K + r: ascending (tag, rank)
    out = []
    for o in np.argsort(-fin, kind="stable")[:K]:
        if fin[o] == -np.inf:
            break
        c, r = divmod(int(o), K)
        path = [c]
        for bp in reversed(bps):
            c, r = divmod(int(bp[c, r]), K)
            path.append(c)
        out.append((float(fin[o]), path[::-1]))
    return out


def brute(x, start, end, trans, K):
    """The same by enumeration: all C^L paths sorted by (-score, reversed path)."""
    L, C = x.shape
    assert C ** L <= BRUTE_MAX_PATHS, (C, L)
    rows = [(-score(x, start, end, trans, p), p[::-1]) for p in itertools.product(range(C), repeat=L)]
    rows.sort()
    return [(-v, list(p[::-1])) for v, p in rows[:K]]


def _np(t):
    return t.detach().cpu().double().numpy()


def rows_of(e, mask, b):
    """The on-positions' emission rows of sample b of a batch-first e [B, S, C] (torch) as float64 numpy [L, C]."""
    pos = on_positions(None if mask is None else mask[b], e.shape[1])
    return _np(e[b])[pos]


def nbest_batch(e, mask, start, end, trans, K, fn=nbest_sample):
    """[[(score, path)]] per sample of a batch-first e [B, S, C] and a mask [B, S] (or None); torch tensors in."""
    st, en, tr = _np(start), _np(end), _np(trans)
    return [fn(rows_of(e, mask, b), st, en, tr, K) for b in range(e.shape[0])]


def _grid(g, shape, lo, hi, step):
    n = torch.randint(int(lo / step), int(hi / step) + 1, shape, generator=g)
    return (n.double() * step).float()


def coarse(B, S, C, seed):
    """-> (e [B, S, C], start, end, trans) f32, every value a multiple of 1/2 in [-2, 2]."""
    g = torch.Generator().manual_seed(seed)
    return tuple(_grid(g, s, -2, 2, 0.5) for s in ((B, S, C), (C,), (C,), (C, C)))


def fine(B, S, C, seed):
    """-> (e, start, end, trans) f32: emissions multiples of 2^-10 in [-4, 4], the parameters in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    return (_grid(g, (B, S, C), -4, 4, 2.0 ** -10),) + tuple(_grid(g, s, -1, 1, 2.0 ** -10) for s in ((C,), (C,), (C, C)))


GRIDS = {"coarse": coarse, "fine": fine}


def prefix_mask(B, S, seed):
    """Ragged prefix masks [B, S] bool with a full-length sample first and, when B > 1, a length-1 sample second."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    return torch.arange(S)[None, :] < lens[:, None]


def holes_mask(B, S, seed):
    """Masks with holes: about 60 % on, position 0 on; one row all off but position 0."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(B, S, generator=g) < 0.6
    mask[B - 1] = False
    mask[:, 0] = True
    return mask
