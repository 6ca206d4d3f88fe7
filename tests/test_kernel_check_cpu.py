"""CPU: the bounds of tests/kernel_check.py hold for an honest f32 emulation of each kernel (same rounding points: operands in
16 bits, f32 accumulation, P in bf16 before P.V, xhat in bf16, outputs in their format) and are MISSED by each seeded fault
-- the proof that the GPU tests built on them fail on a subtly wrong kernel.  The guard check catches a single flipped byte."""
import math

import pytest
import torch

import kernel_check as kc
from kernel_check import BF16, F16, F32

SHAPES = [(1, 1, 1), (100, 13, 72), (129, 130, 65), (77, 200, 13), (13, 200, 1100), (256, 384, 1536)]


def _rnd(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _gemm_case(M, N, K, seed=0):
    A, B = _rnd(M, K, seed=seed + 1), _rnd(N, K, seed=seed + 2)
    A = (A.float() * (2.0 ** -(torch.arange(M) % 12).float())[:, None]).to(BF16)      # rows span magnitudes
    bias = _rnd(N, seed=seed + 3, dtype=F32)
    return A, B, bias


def _outside(out, ref, bound):
    return int(((out.double() - ref).abs() > bound).sum())


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("odt", [BF16, F16, F32])
def test_gemm_bound_holds_for_f32_matmul_and_catches_seeded_faults(M, N, K, odt):
    A, B, bias = _gemm_case(M, N, K)
    z32 = A.float() @ B.float().t() + bias
    ref = A.double() @ B.double().t() + bias.double()
    E = kc.gemm_acc_bound(A.double().abs() @ B.double().abs().t(), K, bias=bias)
    bound = kc.stored(E, ref, odt)
    kc.assert_within(z32.to(odt), ref, bound, "cpu gemm %s" % str(odt)[6:])
    # fault 1: one k term dropped
    kd = K // 2
    drop = (z32 - A[:, kd:kd + 1].float() * B[:, kd].float()[None, :]).to(odt)
    frac = _outside(drop, ref, bound) / ref.numel()
    assert frac > 0 and (K > 200 or min(M, N) < 2 or frac >= 0.5), frac
    # fault 2: bias missing on one column
    nb = (z32 - torch.nn.functional.one_hot(torch.tensor(N - 1), N).float() * bias).to(odt)
    assert _outside(nb, ref, bound) > 0
    # fault 3: two adjacent rows swapped where the values are 2^-10 of the largest rows
    if M >= 12:
        sw = z32.clone()
        sw[[10, 11]] = z32[[11, 10]]
        assert _outside((sw - bias).to(odt), ref - bias.double(), kc.stored(kc.gemm_acc_bound(
            A.double().abs() @ B.double().abs().t(), K), ref - bias.double(), odt)) > 0


@pytest.mark.parametrize("epi", ["GELU", "DGELU", "ADD", "GATE", "TANH", "RELU", "ADD_RELU"])
def test_epilogue_bounds_hold_for_f32_torch(epi):
    M, N, K = 100, 13, 72
    A, B, bias = _gemm_case(M, N, K, seed=5)
    aux = _rnd(M, N, seed=9)
    z32 = 0.5 * (A.float() @ B.float().t()) + bias
    z = 0.5 * (A.double() @ B.double().t()) + bias.double()
    E = kc.gemm_acc_bound(A.double().abs() @ B.double().abs().t(), K, alpha=0.5, bias=bias)
    a32 = aux.float()
    main32, out2_32 = {
        "GELU": lambda: (torch.nn.functional.gelu(z32), z32),
        "DGELU": lambda: (z32 * kc.gelu_prime64(aux).float(), None),
        "ADD": lambda: (z32 + a32, None),
        "GATE": lambda: (torch.sigmoid(z32) * a32, torch.sigmoid(z32)),
        "TANH": lambda: (torch.tanh(z32), None),
        "RELU": lambda: (z32.clamp_min(0), None),
        "ADD_RELU": lambda: ((z32 + a32).clamp_min(0), None)}[epi]()
    ref, ref2 = kc.epilogue_ref(epi, z, aux)
    e, e2 = kc.epilogue_bounds(epi, z, E, aux)
    for odt in (BF16, F16):
        kc.assert_within(main32.to(odt), ref, kc.stored(e, ref, odt), "cpu epilogue %s" % epi)
    if ref2 is not None:
        kc.assert_within(out2_32.to(BF16), ref2, kc.stored(e2, ref2, BF16), "cpu epilogue %s out2" % epi)
    # beta on a bf16 output, one more rounding
    c_old = _rnd(M, N, seed=11)
    rb, eb = kc.with_beta(e, ref, 1.0, c_old)
    kc.assert_within((main32 + c_old.float()).to(BF16), rb, kc.stored(eb, rb, BF16), "cpu epilogue %s beta" % epi)
    # a missing bias column leaves the bound wherever the epilogue still depends on z there
    if epi in ("GELU", "ADD", "TANH"):
        zb = z32.clone(); zb[:, 3] -= bias[3]
        wrong = {"GELU": torch.nn.functional.gelu(zb), "ADD": zb + a32, "TANH": torch.tanh(zb)}[epi]
        assert _outside(wrong.to(BF16), ref, kc.stored(e, ref, BF16)) > 0


# ------------------------------------------------------------------------------------------------------- attention
def _attn_emul(q, k, v, add_mask, scale, dmask=None, last_key=None):
    """f32 online-softmax stand-in: scores and row statistics in f32, P rounded to bf16 before P.V, O rounded to bf16."""
    s = (q.float() @ k.float().t()) * scale + add_mask[None, :]
    if last_key is not None:
        s = s[:, :last_key]; v = v[:last_key]
        dmask = None if dmask is None else dmask[:, :last_key]
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pd = p if dmask is None else p * dmask
    o = (pd.to(BF16).float() @ v.float()) / l
    return o.to(BF16), (m + torch.log(l))[:, 0]


def _attn_ref(q, k, v, add_mask, scale, dmask=None):
    s = (q.double() @ k.double().t()) * scale + add_mask.double()[None, :]
    p = torch.softmax(s, -1)
    delta = kc.attn_delta(q, k, scale, s, p > 0)
    pd = p if dmask is None else p * dmask.double()
    return pd @ v.double(), torch.logsumexp(s, -1), kc.attn_fwd_bound(pd, v, delta), delta


@pytest.mark.parametrize("Sq,Skv", [(1, 1), (5, 7), (65, 129), (130, 257)])
@pytest.mark.parametrize("qk_scale", [1.0, 4.0, 16.0])
def test_attention_bound_holds_and_catches_a_dropped_key_and_a_shifted_mask(Sq, Skv, qk_scale):
    q, k, v = _rnd(Sq, 64, seed=1, scale=qk_scale), _rnd(Skv, 64, seed=2, scale=qk_scale), _rnd(Skv, 64, seed=3)
    add_mask = torch.zeros(Skv)
    if Skv > 4:
        add_mask[Skv // 2] = -10000.0            # a hole; the last key stays valid
    ref, lse, bound, delta = _attn_ref(q, k, v, add_mask, 0.125)
    o, l = _attn_emul(q, k, v, add_mask, 0.125)
    kc.assert_within(o, ref, bound, "cpu attn out")
    kc.assert_within(l, lse, kc.attn_lse_bound(lse, delta), "cpu attn lse")
    # (sharper scores make the softmax one-hot: the last key then only matters in the rows it wins, which the small
    #  shapes need not have -- the fault is required at plain scores, and at 4x in the 130 x 257 case)
    if Skv > 1 and (qk_scale == 1.0 or (qk_scale == 4.0 and (Sq, Skv) == (130, 257))):
        o2, _ = _attn_emul(q, k, v, add_mask, 0.125, last_key=Skv - 1)
        assert _outside(o2, ref, bound) > 0
    if Skv > 4:
        g = torch.Generator().manual_seed(7)
        dmask = (torch.rand(Sq, Skv, generator=g) >= 0.1).float() / 0.9
        refd, _, boundd, _ = _attn_ref(q, k, v, add_mask, 0.125, dmask)
        od, _ = _attn_emul(q, k, v, add_mask, 0.125, dmask)
        kc.assert_within(od, refd, boundd, "cpu attn dropout out")
        os_, _ = _attn_emul(q, k, v, add_mask, 0.125, torch.roll(dmask, 1, dims=1))
        assert _outside(os_, refd, boundd) > 0


def _attn_bwd_emul(q, k, v, add_mask, scale, dout, lse32, dmask):
    """f32 recomputation backward: P from the saved lse, D = rowsum(P m dP) in f32, P and dS rounded to bf16 as matrix
    operands, dP - D in f32, outputs in bf16."""
    s = (q.float() @ k.float().t()) * scale + add_mask[None, :]
    p = torch.exp(s - lse32[:, None])
    dv = (p * dmask).to(BF16).float().t() @ dout.float()
    dP = dout.float() @ v.float().t()
    D = (p * dmask * dP).sum(-1)
    dS = (p.to(BF16).float() * (dmask * dP - D[:, None])).to(BF16).float()
    return (scale * (dS @ k.float())).to(BF16), (scale * (dS.t() @ q.float())).to(BF16), dv.to(BF16), D


@pytest.mark.parametrize("Sq,Skv", [(5, 7), (65, 129), (130, 257)])
@pytest.mark.parametrize("qk_scale", [1.0, 4.0])
def test_attention_backward_bound_holds_and_catches_a_shifted_mask(Sq, Skv, qk_scale):
    q, k, v = _rnd(Sq, 64, seed=1, scale=qk_scale), _rnd(Skv, 64, seed=2, scale=qk_scale), _rnd(Skv, 64, seed=3)
    dout = _rnd(Sq, 64, seed=4)
    add_mask = torch.zeros(Skv); add_mask[Skv // 2] = -10000.0
    g = torch.Generator().manual_seed(7)
    dmask = (torch.rand(Sq, Skv, generator=g) >= 0.1).float() / 0.9
    o, lse32 = _attn_emul(q, k, v, add_mask, 0.125, dmask)
    s = (q.double() @ k.double().t()) * 0.125 + add_mask.double()[None, :]
    p = torch.softmax(s, -1)
    delta = kc.attn_delta(q, k, 0.125, s, p > 0)
    b = kc.attn_bwd_bounds(q, k, v, s, p, dmask.double(), dout, torch.logsumexp(s, -1), delta, 0.125)
    dq, dk, dv, D = _attn_bwd_emul(q, k, v, add_mask, 0.125, dout, lse32, dmask)
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv), ("delta", D)):
        kc.assert_within(t, *b[name], "cpu attn bwd " + name)
    wq, wk, wv, _ = _attn_bwd_emul(q, k, v, add_mask, 0.125, dout, lse32, torch.roll(dmask, 1, dims=1))
    assert _outside(wv, *b["dv"]) > 0
    if qk_scale == 1.0:     # (4x scores: a near one-hot softmax has dS = P (dP - D) ~ 0, below the error the bound must grant D)
        assert _outside(wq, *b["dq"]) > 0 and _outside(wk, *b["dk"]) > 0
    if qk_scale == 1.0:     # at every element no looser than the bar of test_attention_fwd_bwd (3e-2 of the largest reference)
        for name in ("dq", "dk", "dv"):
            assert bool((b[name][1] <= 3e-2 * b[name][0].abs().max()).all()), name


# ------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_emul(x, bias, res, gamma, beta, eps, mean_cols=None):
    s = (x.float() + bias) + res.float()
    H = s.shape[1]
    mean = s.sum(-1, keepdim=True) / H if mean_cols is None else s[:, :mean_cols].sum(-1, keepdim=True) / mean_cols
    c = s - mean
    var = (c * c).sum(-1, keepdim=True) / H
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = c * rstd
    return (gamma * xh + beta).to(BF16), xh.to(BF16), rstd[:, 0]


@pytest.mark.parametrize("M,H", [(5, 8), (5, 72), (3, 520), (3, 2048)])
@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_ln_bound_holds_and_catches_a_short_mean(M, H, offset):
    dt = F32 if offset else BF16
    x, res = (_rnd(M, H, seed=1, dtype=F32) + offset).to(dt), _rnd(M, H, seed=2).to(dt)
    bias, gamma, beta = _rnd(H, seed=3, dtype=F32), _rnd(H, seed=4, dtype=F32) + 1.0, _rnd(H, seed=5, dtype=F32)
    s = x.double() + bias.double() + res.double()
    t_abs = x.double().abs() + bias.double().abs() + res.double().abs()
    b = kc.ln_fwd_bounds(t_abs, s, gamma, beta, 1e-12)
    y, xh, rstd = _ln_emul(x, bias, res, gamma, beta, 1e-12)
    kc.assert_within(y, *b["y"], "cpu ln y")
    kc.assert_within(xh, *b["xhat"], "cpu ln xhat")
    kc.assert_within(rstd, *b["rstd"], "cpu ln rstd")
    if H > 8 and not offset:    # (around a mean of 100 the shift of the short mean is below the f32 noise of the sum itself)
        yw, xw, _ = _ln_emul(x, bias, res, gamma, beta, 1e-12, mean_cols=H - 8)
        assert _outside(xw, *b["xhat"]) > 0 and _outside(yw, *b["y"]) > 0
    # at every element no looser than the bar of test_ln_fwd_bwd (1e-2 of the largest reference) -- for rows of mean 100 up to
    # H = 520, the size the GPU test runs them at; beyond, see "Known limit" in ln_fwd_bounds
    if not offset or H <= 520:
        assert bool((b["y"][1] <= 1e-2 * b["y"][0].abs().max()).all())
        assert bool((b["xhat"][1] <= 1e-2 * b["xhat"][0].abs().max()).all())


@pytest.mark.parametrize("M,H", [(5, 8), (130, 72), (5, 520), (3, 2048)])
def test_ln_backward_bound_holds_and_catches_a_short_mean(M, H):
    dy, xhat = _rnd(M, H, seed=1), _rnd(M, H, seed=2)
    rstd, gamma = _rnd(M, seed=3, dtype=F32).abs() + 0.5, _rnd(H, seed=4, dtype=F32) + 1.0
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(M, H, generator=g) >= 0.1).float() / 0.9
    b = kc.ln_bwd_bounds(dy, xhat, rstd, gamma, mask)

    def emul(cols):
        gd = gamma * dy.float()
        c1 = gd[:, :cols].sum(-1, keepdim=True) / cols
        c2 = (gd * xhat.float()).sum(-1, keepdim=True) / H
        ds = rstd[:, None] * (gd - c1 - xhat.float() * c2)
        return ds.to(BF16), (ds * mask).to(BF16), (dy.float() * xhat.float()).sum(0), dy.float().sum(0)
    dres, dx, dg, db = emul(H)
    for name, t in (("dres", dres), ("dx", dx), ("dgamma", dg), ("dbeta", db)):
        kc.assert_within(t, *b[name], "cpu ln bwd " + name)
    if H > 8:
        wres, wx, _, _ = emul(H - 8)
        assert _outside(wres, *b["dres"]) > 0 and _outside(wx, *b["dx"]) > 0
    assert _outside(torch.roll(dx, 1, dims=1), *b["dx"]) > 0            # a dropout mask shifted by one column
    for name in ("dres", "dx"):     # no looser than the bar of test_ln_fwd_bwd (2e-2 of the largest reference)
        assert bool((b[name][1] <= 2e-2 * b[name][0].abs().max()).all()), name


def test_ln_zero_row_is_beta_exactly():
    H = 72
    z = torch.zeros(1, H, dtype=F32)
    beta = _rnd(H, seed=5, dtype=F32)
    b = kc.ln_fwd_bounds(z.double(), z.double(), torch.ones(H), beta, 1e-12, y_dtype=F32)
    assert torch.equal(b["y_raw"][0][0], beta.double()) and float(b["y_raw"][1].max()) <= 2 * kc.U_ACC * float(beta.abs().max())


# ----------------------------------------------------------------------------------------------------------- guards
@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("where", ["pad column", "row before", "row after", "offset gap"])
def test_guard_check_catches_one_flipped_byte(dtype, where):
    rows, cols, ld, off = 5, 13, 16, 2
    g = kc.Guarded(rows, cols, dtype, ld=ld, offset=off, device="cpu")
    g.view.copy_(torch.arange(rows * cols).reshape(rows, cols).to(dtype))
    g.check()
    at = {"pad column": g.start + 2 * ld + cols, "row before": g.start - ld + 3, "row after": g.start + rows * ld + 1,
          "offset gap": g.start - 1}[where]
    raw = g.flat.view(torch.uint8)
    raw[at * g.flat.element_size()] ^= 0x10
    with pytest.raises(AssertionError):
        g.check()
    raw[at * g.flat.element_size()] ^= 0x10
    g.check()
    # the last pad column of the last row and the very first / last element of the allocation
    for at in (g.start + (rows - 1) * ld + ld - 1, 0, g.flat.numel() - 1):
        raw[at * g.flat.element_size() + g.flat.element_size() - 1] ^= 0x01
        with pytest.raises(AssertionError):
            g.check()
        raw[at * g.flat.element_size() + g.flat.element_size() - 1] ^= 0x01


def test_guard_tail_contract_and_nan_inputs():
    v, check = kc.guarded(5, 13, BF16, ld=16, device="cpu")
    assert bool(torch.isnan(v.float()).all())            # outputs start as NaN: a tile left out shows
    g = kc.Guarded(5, 13, F32, ld=16, device="cpu", init=1.0)
    g.flat[g.start + 5 * 16: g.start + 8 * 16].view(3, 16)[:, :13] = 0.0     # three zeroed tail rows
    g.check(tail_rows=3, expect=0)
    with pytest.raises(AssertionError):
        g.check()                                         # without the contract it is an overrun
    with pytest.raises(AssertionError):
        g.check(tail_rows=4, expect=0)                    # a tail row that was NOT zeroed
    g.flat[g.start + 13: g.start + 16] = 0.0
    with pytest.raises(AssertionError):
        g.check(tail_rows=3, expect=0)                    # pad columns are not part of a row-tail contract
    x = kc.guarded_input(_rnd(5, 13, seed=1), ld=16, device="cpu")
    wide = x.as_strided((5, 16), (16, 1), x.storage_offset())
    assert bool(torch.isfinite(x.float()).all()) and bool(torch.isnan(wide[:, 13:].float()).all())
    assert not math.isfinite(float(wide.float().sum()))


@pytest.mark.parametrize("verbose", [False, True])
def test_assert_within_fails_on_a_nan_ratio(verbose):
    """A NaN in the reference or in the bound, or inf / inf, makes the ratio NaN: that must fail, printed or not."""
    out, ref = torch.ones(3, 4), torch.ones(3, 4, dtype=torch.float64)
    assert kc.assert_within(out, ref, 1e-3, "cpu nan gate ok", verbose=verbose) == 0.0
    bad_ref = ref.clone(); bad_ref[1, 2] = float("nan")
    bad_bound = torch.full((3, 4), 1e-3, dtype=torch.float64); bad_bound[2, 1] = float("nan")
    inf_bound = torch.full((3, 4), float("inf"), dtype=torch.float64)
    inf_out = out.clone(); inf_out[0, 3] = float("inf")
    for o, r, b in ((out, bad_ref, 1e-3), (out * 1.5, ref, bad_bound), (inf_out, ref, inf_bound)):
        with pytest.raises(AssertionError):
            kc.assert_within(o, r, b, "cpu nan gate", verbose=verbose)
    kc._PENDING.clear()
