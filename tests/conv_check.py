"""Helpers of the element-wise tests of the ResNet encoder's convolution and train-mode BatchNorm kernels (icka_conv3x3_gemm,
icka_conv3x3_gemm_stats, icka_gemm_bn_stats: the CONV loader and the STATS branch of gemm_ws_body, csrc/gemm_ws.inc;
icka_bn_finalize, icka_bn_apply: csrc/conv.hip); no test functions.  For every kernel a function that takes the very values
the kernel reads and returns float64 references with their bounds, plus the case lists and input builders that
tests/test_conv_check_cpu.py (emulations, planted faults) and tests/test_conv_elements_gpu.py (the device) share.  The
buffers and the comparison are those of tests/kernel_check.py.  Nothing here is a fitted constant.

Where the bounds come from (u = U_ACC = 2^-23 per f32 operation, as tests/kernel_check.py charges it)
-------------------------------------------------------------------------------------------------
* Convolution: the accumulator is a length-9C f32 dot product of exact bf16 products: ``gemm_acc_bound`` on |x| (*) |w|, the
  epilogue through ``epilogue_bounds``, the bf16 store through ``stored``.  A padded row has a zero accumulator: its value is
  bf16(epilogue(f32(bias) (+ aux))) EXACTLY, which ``conv_pad_rows`` computes in f32.
* Statistics of one 128-row tile (bn_stats_tile), per column: thread q sums the RQ rows of its slice in row order, divides,
  then sums the squared deviations from ITS mean; the NQ slices are merged in slice order by bn_chan_merge.  With a the exact
  accumulators, E their error bound, cnt the valid rows of the slice:
      e_mean_q = mean(E) + cnt u mean|a|                 (cnt - 1 additions and the division, each charged on sum|a| / cnt)
      d = a - mean_q:  e_d = E + e_mean_q + u |d|
      e_m2_q  = sum(2 |d| e_d + e_d^2) + (cnt + 1) u sum d^2      (the squares, then cnt - 1 additions)
  and ``chan_merge`` carries (e_mean, e_m2) through every merge next to the float64 values (see its docstring).  Counts are
  integers below 2^24: exact.
* icka_bn_finalize: the same merge over the tiles in the kernel's order (16 slices of tiles j, j + 16, .., then the slices
  in order), then one u per operation of the kernel's formula on the absolute terms; 1 / sqrtf costs 2 u relative (one rounding
  each for the square root and the division, as ``ln_fwd_bounds`` charges rstd).  See ``finalize_refs``.
"""
import functools

import torch
import torch.nn.functional as F_

import kernel_check as kc
from kernel_check import BF16, F32, U_ACC, assert_within, report, stored  # noqa: F401

F64 = torch.float64
BM = 128
EPIS = ("NONE", "RELU", "ADD", "ADD_RELU")


def pad128(n):
    return (n + 127) // 128 * 128


def out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def f32_of(x):
    """the float a C ``float`` argument receives"""
    return float(torch.tensor(x, dtype=F32))


def case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items())


# ================================================================================================== convolution
# single-pixel maps, one-row and one-column maps, odd sizes under stride 2, a 128-row tile that spans samples, tiles that start
# in the middle of a sample
MAPS = ((1, 1, 1), (2, 1, 9), (2, 9, 1), (3, 5, 7), (2, 8, 8), (1, 15, 9))


def ccase(B, H, W, C, Cout, stride, epi="NONE", bias=True, ldaux=0, extra=0):
    """ldaux: pad columns of aux's row stride (0 or 8); extra: whole 128-row tiles of padding after pad128(rows)"""
    return dict(B=B, H=H, W=W, C=C, Cout=Cout, stride=stride, epi=epi, bias=bias, ldaux=ldaux, extra=extra)


def conv_shape_cases(B, H, W):
    return [ccase(B, H, W, C, Cout, s, epi=EPIS[(C // 64 + Cout // 64 + s) % 4], bias=(Cout != 128))
            for C in (64, 128) for Cout in (64, 128, 192) for s in (1, 2)]


# every epilogue x bias x aux stride at two shapes (64-wide tiles with three column tiles, stride 2, two channel blocks; and a
# 128-wide tile whose rows span two samples), and whole tiles of padding
CONV_OPTION_CASES = ([ccase(*shape, epi=e, bias=b, ldaux=l) for shape in ((3, 5, 7, 128, 192, 2), (2, 8, 8, 64, 128, 1))
                      for e in EPIS for b in (True, False) for l in (0, 8)] +
                     [ccase(1, 15, 9, 64, 128, 1, epi="ADD_RELU", extra=1), ccase(3, 5, 7, 128, 64, 2, epi="RELU", extra=1),
                      ccase(1, 1, 1, 64, 64, 1, epi="ADD", bias=False, ldaux=8, extra=1)])
CONV_STATS_CASES = [ccase(B, H, W, C, Cout, s, bias=False) for (B, H, W) in MAPS for C in (64, 128) for Cout in (64, 128) for s in (1, 2)]


def conv_dims(c):
    Ho, Wo = out_hw(c["H"], c["W"], c["stride"])
    rows = c["B"] * Ho * Wo
    return Ho, Wo, rows, pad128(rows) + 128 * c["extra"]


@functools.lru_cache(maxsize=None)
def _conv_inputs(B, H, W, C, Cout, stride, extra):
    _, _, rows, rp = conv_dims(dict(B=B, H=H, W=W, stride=stride, extra=extra))
    pix = torch.arange(B * H * W).reshape(B, H, W, 1)
    x = (rnd(B, H, W, C, seed=1 + B + 3 * H + 5 * W + C) * 2.0 ** -(pix % 12).float()).to(BF16)      # a small pixel cannot hide
    w = (rnd(Cout, 9 * C, seed=2 + C + Cout) * 0.05).to(BF16)
    bias = rnd(Cout, seed=3 + Cout).to(F32)
    aux = rnd(rp, Cout, seed=4 + rows + Cout).to(BF16)
    x64 = x.double().permute(0, 3, 1, 2)
    w64 = w.double().view(Cout, 3, 3, C).permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(rows, Cout)
    acc = nhwc(F_.conv2d(x64, w64, stride=stride, padding=1))
    ab = nhwc(F_.conv2d(x64.abs(), w64.abs(), stride=stride, padding=1))
    return dict(x=x, w=w, bias=bias, aux=aux, acc=acc, abs=ab)


def conv_inputs(c):
    """CPU tensors of a case (shared, do not modify): x bf16 NHWC, w bf16 [Cout, 9 C] (k = tap * C + c), bias f32, aux bf16
    [rows_padded, Cout]; acc / abs: the float64 convolution of the values / of their absolute values, [rows, Cout]"""
    return _conv_inputs(c["B"], c["H"], c["W"], c["C"], c["Cout"], c["stride"], c["extra"])


def conv_refs(c, inp):
    """-> (reference [rows, Cout], bound) of the valid rows of icka_conv3x3_gemm"""
    rows = inp["acc"].shape[0]
    bias = inp["bias"].double() if c["bias"] else None
    z = inp["acc"] + (bias if bias is not None else 0.0)
    E = kc.gemm_acc_bound(inp["abs"], 9 * c["C"], bias=bias)
    aux = inp["aux"][:rows].double()
    ref = kc.epilogue_ref(c["epi"], z, aux)[0]
    return ref, stored(kc.epilogue_bounds(c["epi"], z, E, aux)[0], ref, BF16)


def conv_pad_rows(c, inp):
    """rows [rows, rows_padded): a zero accumulator through the epilogue -- exact in f32, then the bf16 rounding"""
    rows, rp = inp["acc"].shape[0], inp["aux"].shape[0]
    v = torch.zeros(rp - rows, c["Cout"], dtype=F32)
    if c["bias"]:
        v = v + inp["bias"]
    if c["epi"] in ("ADD", "ADD_RELU"):
        v = v + inp["aux"][rows:].float()
    if c["epi"] in ("RELU", "ADD_RELU"):
        v = v.clamp_min(0)
    return v.to(BF16)


def same_bits(out, ref, what):
    idt = torch.int32 if out.dtype == F32 else torch.int16
    same = out.detach().cpu().contiguous().view(idt) == ref.detach().cpu().contiguous().view(idt)
    assert bool(same.all()), "%s: %d of %d elements differ bitwise" % (what, int((~same).sum()), same.numel())


# =================================================================================================== statistics
RV_256 = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256)       # either side of the 16- and 32-row slices, of a tile, of M


def gcase(M, N, K, rv, lda=0, ldw=0, ldy=0, big=False, exact=False):
    """lda / ldw / ldy: pad columns of the row strides; big: accumulators with a column mean ~ 50 x their spread; exact: small
    integer operands, so that every accumulator is an integer below 2^24 -- exact in f32 in any summation order (E = 0: the
    bounds of the partials are then those of the slice sums and the merges alone)"""
    return dict(M=M, N=N, K=K, rv=rv, lda=lda, ldw=ldw, ldy=ldy, big=big, exact=exact)


def gemm_stats_cases(K, N):
    return [gcase(256, N, K, rv) for rv in RV_256] + [gcase(384, N, K, 130)]


GEMM_STATS_KN = [(K, N) for K in (64, 192) for N in (64, 128, 192)]
GEMM_STATS_LD_CASES = [gcase(256, 64, 64, 129, lda=8), gcase(256, 128, 192, 129, ldw=8), gcase(256, 192, 64, 129, ldy=8),
                       gcase(384, 128, 64, 130, lda=8, ldw=8, ldy=8), gcase(384, 64, 192, 130, lda=8, ldw=8, ldy=8)]
GEMM_STATS_BIG_CASES = [gcase(256, 128, 64, 129, big=True), gcase(384, 64, 192, 130, big=True)]
GEMM_STATS_EXACT_CASES = [gcase(256, N, K, rv, exact=True, big=big) for (N, K) in ((64, 64), (128, 192)) for rv in (33, 129, 256)
                          for big in (False, True)]


@functools.lru_cache(maxsize=None)
def _gemm_inputs(M, N, K, rv, big, exact):
    a = (rnd(M, K, seed=5 + M + K) * 0.5 + 0.1)
    w = rnd(N, K, seed=6 + N + K) * (1.0 / K ** 0.5)
    if exact:                   # integers in [-4, 4] x [-2, 2]: |accumulator| <= 8 K, spread ~ 3.7 sqrt(K)
        g = torch.Generator().manual_seed(8 + M + N + K)
        a = torch.randint(-4, 5, (M, K), generator=g).float()
        w = torch.randint(-2, 3, (N, K), generator=g).float()
    if big and exact:           # + 64 * 32 = 2048 on accumulators of spread ~ 30 (K = 64) / ~ 50 (K = 192)
        a[:, 0] = 64.0
        w[:, 0] = 32.0
    elif big:                   # a constant column against a constant row: + 25 on accumulators of spread ~ 0.5
        a[:, 0] = 5.0
        w[:, 0] = 5.0
    a[rv:] = 9.0                # reaches the raw output, must not reach the statistics
    a, w = a.to(BF16), w.to(BF16)
    return dict(a=a, w=w, acc=a.double() @ w.double().t(), abs=a.double().abs() @ w.double().abs().t())


def gemm_inputs(c):
    """CPU tensors (shared, do not modify): a bf16 [M, K] (rows from rows_valid on hold 9.0), w bf16 [N, K]; acc / abs
    float64 [M, N]"""
    return _gemm_inputs(c["M"], c["N"], c["K"], c["rv"], c["big"], c["exact"])


def gemm_E(c, inp):
    """error bound of the f32 accumulators of a statistics GEMM case"""
    return torch.zeros_like(inp["acc"]) if c["exact"] else kc.gemm_acc_bound(inp["abs"], c["K"])


def tile_width(N):
    return 128 if N % 128 == 0 else 64


def chan_merge(state, nb, mb, m2b, e_mb, e_m2b):
    """One bn_chan_merge, (n, mean, m2) <- (n, mean, m2) + (nb, mb, m2b), in float64 with the running error bounds of the f32
    kernel: state = (n, mean, m2, e_mean, e_m2), tensors of one shape.  The kernel computes
        nn = n + nb (exact), d = mb - mean, f = nb / nn, mean += d f, m2 += m2b + d d n f
    so with e_d = e_mb + e_mean + u |d| and e_f = u f:
        e_mean' = e_mean + f e_d + |d| e_f + u |d f| + u |mean'|
        e_t     = (2 |d| e_d + e_d^2) n f + d^2 n e_f + 3 u t,           t = d^2 n f (three multiplications)
        e_m2'   = e_m2 + e_m2b + e_t + u (m2b + t) + u m2'                (two additions of non-negative terms)
    A part with nb == 0 is skipped whatever it holds; the first live part is copied exactly (x * 1, + 0)."""
    n, mu, m2, e_mu, e_m2 = state
    live = nb > 0
    first = live & (n == 0)
    nn = n + nb
    f = nb / nn.clamp_min(1.0)
    d = mb - mu
    e_d = e_mb + e_mu + U_ACC * d.abs()
    e_f = U_ACC * f
    mu2 = mu + d * f
    e_mu2 = e_mu + f * e_d + d.abs() * e_f + U_ACC * (d * f).abs() + U_ACC * mu2.abs()
    t = d * d * n * f
    e_t = (2 * d.abs() * e_d + e_d * e_d) * n * f + d * d * n * e_f + 3 * U_ACC * t
    m22 = m2 + m2b + t
    e_m22 = e_m2 + e_m2b + e_t + U_ACC * (m2b + t) + U_ACC * m22
    pick = lambda a_first, a_merged, a_old: torch.where(first, a_first, torch.where(live, a_merged, a_old))
    return (torch.where(live, nn, n), pick(mb, mu2, mu), pick(m2b, m22, m2), pick(e_mb, e_mu2, e_mu), pick(e_m2b, e_m22, e_m2))


def _zero_state(like):
    z = torch.zeros_like(like, dtype=F64)
    return (z, z, z, z, z)


def stats_refs(acc, E, rows_valid, bnt):
    """Partials of bn_stats_tile.  acc, E float64 [M, N] (exact accumulators, their error bound), tile width bnt.
    -> {"count": ref, "mean": (ref, bound), "m2": (ref, bound)}, each [M / 128, N]: the references are the float64 statistics of
    the tile's valid rows taken directly; the bounds follow the kernel's slices and merges (module docstring)."""
    M, N = acc.shape
    nq = 512 // bnt
    rq = BM // nq
    cnts, means, m2s, e_means, e_m2s = [], [], [], [], []
    for t in range(M // BM):
        nv = min(max(rows_valid - t * BM, 0), BM)
        st = _zero_state(acc[0])
        for q in range(nq):
            r0, r1 = q * rq, min(q * rq + rq, nv)
            cnt = max(r1 - r0, 0)
            if cnt == 0:
                continue
            a, e = acc[t * BM + r0:t * BM + r1], E[t * BM + r0:t * BM + r1]
            mq = a.mean(0)
            e_mq = e.mean(0) + cnt * U_ACC * a.abs().mean(0)
            d = a - mq
            e_d = e + e_mq + U_ACC * d.abs()
            m2q = (d * d).sum(0)
            e_m2q = (2 * d.abs() * e_d + e_d * e_d).sum(0) + (cnt + 1) * U_ACC * m2q
            st = chan_merge(st, torch.full_like(mq, float(cnt)), mq, m2q, e_mq, e_m2q)
        v = acc[t * BM:t * BM + nv]
        mean = v.mean(0) if nv else torch.zeros(N, dtype=F64)
        cnts.append(torch.full((N,), float(nv), dtype=F64))
        means.append(mean)
        m2s.append(((v - mean) ** 2).sum(0))
        e_means.append(st[3])
        e_m2s.append(st[4])
    S = torch.stack
    return {"count": S(cnts), "mean": (S(means), stored(S(e_means), S(means), F32)), "m2": (S(m2s), stored(S(e_m2s), S(m2s), F32)),
            "e_mean": S(e_means), "e_m2": S(e_m2s)}


def compare_partials(part, refs, what, verbose=False):
    """part [3, tiles, N] against ``stats_refs``: counts exact, mean and M2 inside their bounds; a tile without a valid row
    holds (0, 0, 0)"""
    part = part.detach().cpu()
    assert torch.isfinite(part).all(), what + ": non-finite partials"
    same_bits(part[0], refs["count"].float(), what + " count")
    assert_within(part[1], refs["mean"][0], refs["mean"][1], what + " mean", verbose=verbose)
    assert_within(part[2], refs["m2"][0], refs["m2"][1], what + " m2", verbose=verbose)
    empty = refs["count"] == 0
    assert not bool(part[1][empty].ne(0).any()) and not bool(part[2][empty].ne(0).any()), what + ": an empty tile is not (0, 0, 0)"


# ===================================================================================================== finalize
FIN_TILES = (1, 15, 16, 17, 33)
FIN_C = (8, 16, 24, 72)
FIN_MOMENTA = ((0.0, 0), (0.1, 0), (1.0, 0), (None, 0), (None, 4))        # (momentum, num_batches_tracked)
FIN_EPS = (1e-5, 1e-3)


def fcase(tiles, C, momentum, nbt, eps, kind="rand"):
    """kind: "rand" (unequal counts, some zero), "big" (tile means ~ 100 against a spread of 1), "one" (total n == 1),
    "none" (every count zero)"""
    return dict(tiles=tiles, C=C, momentum=momentum, nbt=nbt, eps=eps, kind=kind)


def fin_cases(tiles, C):
    return [fcase(tiles, C, m, nbt, eps) for (m, nbt) in FIN_MOMENTA for eps in FIN_EPS]


FIN_SPECIAL_CASES = [fcase(t, C, m, nbt, 1e-5, kind) for kind in ("big", "one", "none")
                     for (t, C, m, nbt) in ((17, 24, 0.1, 0), (33, 72, None, 4), (1, 8, 1.0, 0))]


@functools.lru_cache(maxsize=None)
def _fin_inputs(tiles, C, kind):
    g = torch.Generator().manual_seed(7 + 31 * tiles + C)
    n = torch.randint(1, 129, (tiles, 1), generator=g).float().expand(tiles, C).clone()      # a tile's count: one per tile ..
    if tiles > 1:
        n[torch.rand(tiles, generator=g) < 0.25] = 0.0
    n[:, C // 2] = torch.randint(0, 129, (tiles,), generator=g).float()                         # .. and one column of its own
    mean = torch.randn(tiles, C, generator=g)
    if kind == "big":
        mean = mean * 0.1 + 100.0
    m2 = torch.rand(tiles, C, generator=g) * n + 0.01
    if kind in ("one", "none"):
        n = torch.zeros(tiles, C)
    if kind == "one":
        n[tiles // 2] = 1.0
    m2[n == 1] = 0.0
    # (a part of count 0 is skipped whatever it holds: its mean and M2 stay the junk drawn above)
    part = torch.stack([n, mean, m2]).to(F32)
    vec = lambda: torch.randn(C, generator=g).to(F32)
    return dict(part=part, weight=vec() + 1.5, bias=vec(), rm=vec(), rv=vec().abs() + 0.5)


def fin_inputs(c):
    """CPU tensors (shared, do not modify): part f32 [3, tiles, C], weight, bias, rm, rv f32 [C]"""
    return _fin_inputs(c["tiles"], c["C"], c["kind"])


def pooled(part):
    """exact pooled (n, mean, M2) of partials [3, tiles, C] in float64; n == 0: (0, 0, 0)"""
    n_t, mean_t, m2_t = part.double()
    live = n_t > 0
    mean_t, m2_t = torch.where(live, mean_t, 0.0), torch.where(live, m2_t, 0.0)
    n = n_t.sum(0)
    mean = (n_t * mean_t).sum(0) / n.clamp_min(1.0)
    m2 = m2_t.sum(0) + (n_t * (mean_t - mean) ** 2).sum(0)
    return n, mean, m2


def finalize_refs(part, weight, bias, rm, rv, nbt, momentum, eps, e_mean=None, e_m2=None):
    """icka_bn_finalize.  part [3, tiles, C] (f32 values; with e_mean / e_m2 [tiles, C] the error bounds of its mean / M2 planes
    against exact partials -- the chained test); the rest as the kernel takes them.  -> {"scale", "shift", "running_mean",
    "running_var": (float64 reference, bound)} and "mean" / "var" / "n" (the batch statistics and their bounds, unrounded).

    The merge runs in the kernel's order with ``chan_merge``; the references themselves come from ``pooled``.  Then, one u per
    operation, each charged on the absolute value of its result:
        var = m2 / n                              e_var = e_m2 / n + u var                         (n == 0: var = 0 exactly)
        rs = 1 / sqrtf(var + eps)                 r_rs  = (e_var + u (var + eps)) / (2 (var + eps)) + 2 u        (relative)
        scale = weight rs                         e_sc  = |scale| (r_rs + u)
        shift = bias - mean scale                 e_sh  = |mean| e_sc + |scale| e_mean + u |mean scale| + u (|bias| + |mean scale|)
        m = momentum, or 1 / (nbt + 1)            e_m   = 0, or u m
        unbiased = var n / (n - 1) if n > 1 else var        e_unb = (e_var + 2 u var) n / (n - 1)
        running = m new + (1 - m) old             e = m e_new + e_m |new| + u |m new| + (e_m + u |1 - m|) |old| + u |(1 - m) old|
                                                      + u (|m new| + |(1 - m) old|)
    What include/icka_hip.h promises of n <= 1: with n == 1 the variance and the value blended into running_var are 0; with
    n == 0 also the mean, so scale = weight / sqrt(eps), shift = bias and both running statistics move towards 0."""
    n_t, mean_t, m2_t = part.double()
    tiles, C = n_t.shape
    z = torch.zeros(tiles, C, dtype=F64)
    e_mean = z if e_mean is None else e_mean.double()
    e_m2 = z if e_m2 is None else e_m2.double()
    slices = []
    for ty in range(16):
        st = _zero_state(n_t[0])
        for t in range(ty, tiles, 16):
            st = chan_merge(st, n_t[t], mean_t[t], m2_t[t], e_mean[t], e_m2[t])
        slices.append(st)
    st = slices[0]
    for j in range(1, 16):
        st = chan_merge(st, slices[j][0], slices[j][1], slices[j][2], slices[j][3], slices[j][4])
    _, _, _, e_mu, e_M2 = st
    n, mu, M2 = pooled(part)
    assert torch.equal(n, st[0])
    u = U_ACC
    w, b, rm, rv = weight.double(), bias.double(), rm.double(), rv.double()
    eps = f32_of(eps)
    n1 = n.clamp_min(1.0)
    var = torch.where(n > 0, M2 / n1, 0.0)
    e_var = torch.where(n > 0, e_M2 / n1 + u * var, 0.0)
    v = var + eps
    r_rs = (e_var + u * v) / (2 * v) + 2 * u
    sc = w / torch.sqrt(v)
    e_sc = sc.abs() * (r_rs + u)
    ms = mu * sc
    sh = b - ms
    e_sh = mu.abs() * e_sc + sc.abs() * e_mu + u * ms.abs() + u * (b.abs() + ms.abs())
    if momentum is None:
        m = 1.0 / (nbt + 1)
        e_m = u * m
    else:
        m, e_m = f32_of(momentum), 0.0
    fac = torch.where(n > 1, n / (n - 1).clamp_min(1.0), 1.0)
    unb = var * fac
    e_unb = torch.where(n > 1, (e_var + 2 * u * var) * fac, e_var)

    def blend(new, e_new, old):
        t1, t2 = m * new, (1 - m) * old
        e = m * e_new + e_m * new.abs() + u * t1.abs() + (e_m + u * abs(1 - m)) * old.abs() + u * t2.abs() + u * (t1.abs() + t2.abs())
        return t1 + t2, stored(e, t1 + t2, F32)

    return {"scale": (sc, stored(e_sc, sc, F32)), "shift": (sh, stored(e_sh, sh, F32)), "running_mean": blend(mu, e_mu, rm),
            "running_var": blend(unb, e_unb, rv), "mean": (mu, e_mu), "var": (var, e_var), "n": n, "e_scale": e_sc, "e_shift": e_sh}


def compare_finalize(out, refs, what, verbose=False):
    for name in ("scale", "shift", "running_mean", "running_var"):
        assert_within(out[name], refs[name][0], refs[name][1], "%s %s" % (what, name), verbose=verbose)


# ======================================================================================================== chain
CHAIN = gcase(256, 64, 64, 130)
CHAIN_EPS, CHAIN_MOMENTUM = 1e-5, 0.1


def chain_refs(inp, rows_valid, weight, bias, rm, rv, nbt, momentum, eps):
    """stats GEMM -> finalize -> bn_apply (ReLU) of one layer against float64 F.batch_norm(training=True) + ReLU of the exact
    accumulators.  The bound is propagated: the partials' bounds (``stats_refs``) feed ``finalize_refs``, whose scale / shift bounds
    meet the bf16 rounding of the raw output in  y = raw scale + shift:
        e = |scale| e_raw + (|acc| + e_raw) e_scale + e_shift + 3 u (|acc scale| + |shift|),  then the bf16 store."""
    acc, N = inp["acc"], inp["acc"].shape[1]
    E = kc.gemm_acc_bound(inp["abs"], inp["a"].shape[1])          # (the chained case is not an exact one)
    st = stats_refs(acc, E, rows_valid, tile_width(N))
    part = torch.stack([st["count"], st["mean"][0], st["m2"][0]])
    fr = finalize_refs(part, weight, bias, rm, rv, nbt, momentum, eps, e_mean=st["e_mean"], e_m2=st["e_m2"])
    v = acc[:rows_valid]
    ref = F_.batch_norm(v, None, None, weight.double(), bias.double(), True, 0.0, f32_of(eps)).clamp_min(0)
    e_raw = stored(E[:rows_valid], v, BF16)
    sc, sh = fr["scale"][0], fr["shift"][0]
    e = sc.abs() * e_raw + (v.abs() + e_raw) * fr["scale"][1] + fr["shift"][1] + 3 * U_ACC * ((v * sc).abs() + sh.abs())
    return ref, stored(e, ref, BF16), fr
