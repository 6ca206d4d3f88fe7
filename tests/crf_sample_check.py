"""Helpers of the icka_crf_sample tests (no test functions): the uniforms restated in numpy, the float64 chain, a checker that
conditions every step on the kernel's own next tag, a plain f32 emulation of the normative algorithm (include/icka_hip.h) and
planted-fault variants of it.

The checker replays no path of its own: for every (sample b, draw k, on-position i) it takes the stored y_i (or ``end`` at the
last position), forms the float64 CDF F_j of the step and accepts the stored tag j iff F_{j-1} - tol <= r <= F_j + tol.  So one
borderline draw cannot make the rest of a path incomparable.

tol per step (nothing fitted; conventions of tests/crf_check.py: u = U_ACC = 2^-23 per f32 operation, EXP_REL and LOG_ABS as
there).  The kernel's exponent of tag t is v_t = alpha_{i-1}(t) + trans[t, y_i] with the CENTRED alpha of include/icka_hip.h: off
by d_t = da_{i-1}(t) + u |v_t|, with da the absolute error of the centred log-domain alpha (``alpha_errors``: the recursion of
crf_check.log_errors with the magnitudes of the centred values; a constant per position is no error, no CDF sees it).
w_t = exp(v_t - m): the row maximum m is common to every tag and cancels in the CDF; what stays is the rounding of the
difference, u |v_t - m|, and EXP_REL(v_t - m):
    rho_t = expm1(d_t) + 2^-22 + 2 u |v_t - m|
With p_t the exact probabilities of the step, a sequential f32 prefix sum of non-negative terms adds at most C u relative, so
do W and one more u the product r W:
    |F^_j - F_j| <= 2 sum_t rho_t p_t + (2 C + 1) u + C 2^-116 = tol
(numerator and normaliser; the last term: weights below 2^-116 may be flushed to zero).
A step is BORDERLINE when r lies within tol of an interior boundary F_0 .. F_{C-2}: two tags are acceptable there.  ``check``
returns the share of such steps; every test caps it at 5 %, so that a loose tol cannot hide a wrong sampler."""
import functools
import math

import numpy as np
import torch

import crf_check as CC
from kernel_check import U_ACC
from test_dropout_hash_cpu import icka_hash

F64 = torch.float64
CAP = 0.05                                  # largest share of borderline steps a case may have
ZERO_W = -150.0 * math.log(2.0)             # v - m below this: the f32 weight is exactly 0 whatever the rounding
M32 = 0xffffffff


# ------------------------------------------------------------------------------------------------------- uniforms
def seed_words(seed, seed_dev=(0, 0)):
    return (seed & M32) ^ (seed_dev[0] & M32), ((seed >> 32) & M32) ^ (seed_dev[1] & M32)


def uniforms(seed, seed_dev, b, K, k, S, positions):
    """r of draw k of sample b at the given positions, float64 (exact: 24 bits)"""
    s0, s1 = seed_words(seed, seed_dev)
    idx = (((b * K + k) * S + np.asarray(positions, dtype=np.int64)) & M32).astype(np.uint32)
    return (icka_hash(s0, s1, idx) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def seed_with_zero_uniform(idx):
    """a seed (s1 = 0) whose hash at element ``idx`` is 0, so r = 0: the hash inverted step by step"""
    inv = lambda m: pow(m, -1, 1 << 32)
    x = 0                                                   # h = 0; x ^= x >> 16 undone: still 0
    x = (x * inv(0x846ca68b)) & M32                         # s1 = 0
    x = x ^ (x >> 15) ^ (x >> 30)
    x = (x * inv(0x7feb352d)) & M32
    x = x ^ (x >> 16)
    return (x - idx * 0x9E3779B1) & M32


# ---------------------------------------------------------------------------------------------------------- chain
def chain(inp, b):
    S = inp["e"].shape[1]
    return CC.Chain(inp["e"][b], None if inp["mask"] is None else inp["mask"][b], torch.zeros(S, dtype=torch.int64),
                    inp["start"], inp["end"], inp["trans"])


def alpha_errors(c):
    """-> (n [L, C], da [L, C], dz): the exact CENTRED forward scores n_i = alpha_i - max_v alpha_i(v), the absolute error
    bounds of the kernel's centred alpha (up to the constant of its position, which no CDF sees) and the bound of log Z.

    The recursion of crf_check.log_errors term by term, with the magnitudes of the centred values the kernel really holds
    (include/icka_hip.h): v = n_{i-1}(t) + trans costs u |v| and enters the log-sum-exp weighted by softmax(v); LSE_C as
    there; u |lse| for the add of m, u |a| for the add of x_i, and one more u |n_i| for the subtraction of kappa_i.
    log Z = (kappa_0 + .. + kappa_{L-1}) + lse(n_{L-1} + end): the running sum of the kappas costs u |K_i| per add (K_i = their
    exact partial sum = max_v alpha_i(v)), the last log-sum-exp as above, the final add u |log Z|."""
    L, C, u = c.L, c.C, U_ACC
    lseC = 2.0 ** -22 + (2 * C / math.e) * u + (C + 6) * u + 2.0 ** -22 * (1.0 + math.log(C))
    T, al, x = c.T, c.alpha, c.x
    Kc = al.max(1).values
    n = al - Kc[:, None]
    da = [u * al[0].abs() + u * n[0].abs()]
    for k in range(1, L):
        v = n[k - 1][:, None] + T
        w = torch.softmax(v, 0)
        lse = torch.logsumexp(v, 0)
        da.append((w * (da[-1][:, None] + u * v.abs())).sum(0) + lseC + u * lse.abs() + u * (lse + x[k]).abs() + u * n[k].abs())
    v = n[L - 1] + c.end
    w = torch.softmax(v, 0)
    dz = float((w * (da[-1] + u * v.abs())).sum() + lseC + u * torch.logsumexp(v, 0).abs() + u * Kc[1:].abs().sum()
               + u * c.log_z.abs())
    return n, torch.stack(da), dz


def step_cdf(v, da_row, C):
    """float64 exponents v [C] of one step and the alpha bounds of its row -> (F [C], tol, certainly-zero weights [C])"""
    u = U_ACC
    m = v.max()
    p = np.exp(v - m)
    p /= p.sum()
    rho = np.expm1(da_row + u * np.abs(v)) + 2.0 ** -22 + 2 * u * np.abs(v - m)
    tol = 2.0 * float((rho * p).sum()) + (2 * C + 1) * u + C * 2.0 ** -116
    return np.cumsum(p), tol, (v - m) < ZERO_W - (da_row + u * np.abs(v))


# -------------------------------------------------------------------------------------------------------- checker
def split_rows(lens, rows):
    """rows [K][>= sum(lens)] -> paths[k][b]"""
    out = []
    for row in rows:
        o, per = 0, []
        for n in lens:
            per.append([int(t) for t in row[o:o + n]])
            o += n
        out.append(per)
    return out


def check(inp, out, K, seed, seed_dev=(0, 0), verbose=None):
    """Assert everything the module docstring and the entry's contract state about ``out`` = {"lens" [B], "log_z" [B],
    "scores" [B][K], "tags" [K][capacity]} (python lists) -> the share of borderline steps."""
    B, S, C = inp["e"].shape
    u = U_ACC
    steps = borderline = 0
    worst = {"cdf": 0.0, "score": 0.0, "log_z": 0.0}
    lens_ref = []
    chains_ = [chain(inp, b) for b in range(B)]
    for b, c in enumerate(chains_):
        lens_ref.append(c.L)
    assert list(out["lens"]) == lens_ref, ("lens", out["lens"], lens_ref)
    paths = split_rows(lens_ref, out["tags"])
    for b, c in enumerate(chains_):
        L = c.L
        n, da, dz = alpha_errors(c)
        al, T, en, da = n.numpy(), c.T.numpy(), c.end.numpy(), da.numpy()
        lz_tol = dz + u * abs(float(c.log_z))
        err = abs(out["log_z"][b] - float(c.log_z))
        worst["log_z"] = max(worst["log_z"], err / lz_tol)
        assert err <= lz_tol, ("log_z", b, out["log_z"][b], float(c.log_z), lz_tol)
        for k in range(K):
            y = paths[k][b]
            assert len(y) == L and all(0 <= t < C for t in y), ("tags out of range", b, k, y)
            r = uniforms(seed, seed_dev, b, K, k, S, c.pos)
            for i in range(L - 1, -1, -1):
                v = al[i] + (en if i == L - 1 else T[:, y[i + 1]])
                F, tol, zero = step_cdf(v, da[i], C)
                j = y[i]
                assert not zero[j], ("a tag whose f32 weight is exactly 0 was drawn", b, k, i, j)
                lo = F[j - 1] if j > 0 else 0.0
                hi = F[j] if j < C - 1 else 1.0
                miss = max(lo - r[i], r[i] - hi)
                worst["cdf"] = max(worst["cdf"], miss / tol)
                assert miss <= tol, ("the drawn tag does not match its uniform", b, k, i, j, r[i], lo, hi, tol)
                steps += 1
                borderline += bool(C > 1 and np.any(np.abs(F[:C - 1] - r[i]) <= tol))
            terms = CC.path_terms(y, c.x, c.start, c.end, c.T)
            s_tol = CC.viterbi_tol(L, terms) / 2 + u * abs(sum(terms))      # one f32 running sum, and its stored value
            err = abs(out["scores"][b][k] - sum(terms))
            worst["score"] = max(worst["score"], err / s_tol if s_tol > 0 else float(err > 0))
            assert err <= s_tol, ("score", b, k, out["scores"][b][k], sum(terms), s_tol)
    share = borderline / max(steps, 1)
    if verbose:
        print("SAMPLE %s: %d steps, borderline %.4f, worst err / tol: cdf %.3f score %.3f log_z %.3f"
              % (verbose, steps, share, worst["cdf"], worst["score"], worst["log_z"]))
    return share


# ------------------------------------------------------------------------------------------------------ emulation
FAULTS = ("uniform_weights", "no_end", "trans_transposed", "uniform_of_previous_position", "uniform_of_next_draw",
          "greater_equal")


def emulate(inp, K, seed, seed_dev=(0, 0), fault=None):
    """The normative algorithm in plain f32 (numpy), sums in tag order -> the dict ``check`` takes.  ``fault``: one of FAULTS."""
    f32 = np.float32
    B, S, C = inp["e"].shape
    E, st, en, T = (inp[k].numpy().astype(f32) for k in ("e", "start", "end", "trans"))
    out = {"lens": [], "log_z": [], "scores": [], "tags": [[] for _ in range(K)]}
    seq_sum = lambda a: f32(0) if a.size == 0 else np.cumsum(a, dtype=f32)[-1]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for b in range(B):
            pos = CC.PO.on_positions(None if inp["mask"] is None else inp["mask"][b], S)
            L = len(pos)
            x = E[b][pos]
            al = np.zeros((L, C), dtype=f32)
            a = st + x[0]
            lz = a.max()
            al[0] = a - lz
            for i in range(1, L):
                v = al[i - 1][:, None] + T
                m = v.max(0)
                s = np.stack([seq_sum(np.exp(v[:, j] - m[j])) for j in range(C)])
                a = (m + np.log(s)).astype(f32) + x[i]
                lz = f32(lz + a.max())
                al[i] = a - a.max()
            v = al[L - 1] + en
            m = v.max()
            out["lens"].append(L)
            out["log_z"].append(float(f32(lz + f32(m + np.log(seq_sum(np.exp(v - m)))))))
            sc_row = []
            for k in range(K):
                ku = k + 1 if fault == "uniform_of_next_draw" else k
                pu = [p - 1 for p in pos] if fault == "uniform_of_previous_position" else pos
                r = uniforms(seed, seed_dev, b, K, ku, S, pu).astype(f32)
                y = [0] * L
                for i in range(L - 1, -1, -1):
                    if i == L - 1:
                        t = np.zeros(C, dtype=f32) if fault == "no_end" else en
                    else:
                        t = T[y[i + 1], :] if fault == "trans_transposed" else T[:, y[i + 1]]
                    v = al[i] + t
                    w = np.exp(v - v.max()).astype(f32)
                    if fault == "uniform_weights":
                        w = np.ones(C, dtype=f32)
                    cum = np.cumsum(w, dtype=f32)
                    thr = f32(r[i] * cum[-1])
                    hit = np.nonzero(cum >= thr if fault == "greater_equal" else cum > thr)[0]
                    live = np.nonzero(w > 0)[0]
                    y[i] = int(hit[0]) if hit.size else (int(live[-1]) if live.size else 0)
                s = f32(0)
                for i in range(L):
                    s = f32(f32(s + (st[y[0]] if i == 0 else T[y[i - 1], y[i]])) + x[i][y[i]])
                sc_row.append(float(f32(s + en[y[L - 1]])))
                out["tags"][k] += y
            out["scores"].append(sc_row)
    return out


# ---------------------------------------------------------------------------------------------------------- cases
# (name, B, S, C, K, mask kind of crf_check.make_masks, emission scale, row stride ld - C); "holes_zero_row": "holes" with
# the mask of row 1 zero everywhere, position 0 included (one on-position all the same)
CASES = [
    ("one_tag", 3, 5, 1, 3, "none", 1.0, 0),
    ("one_position", 1, 1, 2, 1, "none", 1.0, 0),
    ("c13_holes_ld", 3, 9, 13, 5, "holes_zero_row", 2.0, 3),
    ("c16_first_off", 3, 8, 16, 4, "first_off", 2.0, 0),
    ("c17_holes", 3, 8, 17, 3, "holes", 2.0, 1),
    ("c64_prefix", 1, 5, 64, 5, "prefix", 2.0, 0),
    ("b70", 70, 12, 13, 4, "holes", 2.0, 0),
    ("k64", 3, 6, 13, 64, "none", 2.0, 0),
    ("s512", 2, 512, 13, 3, "holes", 4.0, 0),
    ("lds_full_c64", 1, 192, 64, 2, "holes", 8.0, 0),
    ("lds_full_c16", 1, 768, 16, 1, "holes", 8.0, 0),
]
SEED = 0x1234_5678_9abc_def1


def case_id(c):
    return c[0]


@functools.lru_cache(maxsize=None)
def make_case(case):
    """The inputs of a case (CPU tensors, f32 / int64), seeded by the case; computed once and left unchanged."""
    name, B, S, C, K, mk, scale, pad = case
    g = torch.Generator().manual_seed(B * 100003 + S * 1009 + C * 17 + K)
    e = torch.randn(B, S, C, generator=g) * scale
    start, end = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    trans = torch.randn(C, C, generator=g) * 0.7
    mask = CC.make_masks(B, S, "holes" if mk == "holes_zero_row" else mk, g)
    if mk == "holes_zero_row":
        mask[1, :] = 0
    return {"e": e, "mask": mask, "start": start, "end": end, "trans": trans}


BIO_NAMES = ["O", "B-PER", "I-PER", "B-LOC", "I-LOC"]


def bio_illegal(prev, cur):
    """I-X may follow only B-X or I-X (prev None: the start)"""
    if not BIO_NAMES[cur].startswith("I-"):
        return False
    return prev is None or BIO_NAMES[prev].split("-")[-1] != BIO_NAMES[cur].split("-")[-1] or BIO_NAMES[prev] == "O"


@functools.lru_cache(maxsize=None)
def bio_case(B=8, S=10):
    C = len(BIO_NAMES)
    g = torch.Generator().manual_seed(99)
    e = torch.randn(B, S, C, generator=g) * 2.0
    start, end = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    trans = torch.randn(C, C, generator=g) * 0.7
    for cur in range(C):
        if bio_illegal(None, cur):
            start[cur] = -1e4
        for prev in range(C):
            if bio_illegal(prev, cur):
                trans[prev, cur] = -1e4
    return {"e": e, "mask": CC.make_masks(B, S, "holes", g), "start": start, "end": end, "trans": trans}
