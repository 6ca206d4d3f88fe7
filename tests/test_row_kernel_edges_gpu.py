"""GPU: the row kernels (LayerNorm forward / backward, dropout, casts, column sums, add, gate backward, region tokens, transpose)
element by element against float64 -- data movement bitwise -- with every operand in NaN bands and every output in sentinel
bands (tests/kernel_check.py)."""
import math

import pytest
import torch

import kernel_check as kc
from kernel_check import BF16, F16, F32

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9abc


def _k():
    from icka_amd import kernels
    kernels.set_dropout_nonce(None)
    return kernels


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _vec(values):
    return kc.guarded_input(values.reshape(1, -1).to(F32))[0]


def _flat_in(values):
    return kc.guarded_input(values.reshape(1, -1))[0]


def _bits_equal(out, ref, what):
    idt = torch.int32 if out.dtype == F32 else torch.int16
    same = out.contiguous().view(idt) == ref.to(out.device).contiguous().view(idt)
    assert bool(same.all()), "%s: %d of %d elements differ bitwise" % (what, int((~same).sum()), same.numel())


# ------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_case(k, M, H, dt, p, x0, r0, bias0, eps=1e-12, what="ln"):
    gamma0, beta0 = _rnd(H, seed=4).to(F32) + 1.0, _rnd(H, seed=5).to(F32)
    pad = 8
    x, res = kc.guarded_input(x0, ld=H + pad), kc.guarded_input(r0, ld=H + pad)
    bias, gamma, beta = (None if bias0 is None else _vec(bias0)), _vec(gamma0), _vec(beta0)
    y, c_y = kc.guarded(M, H, BF16, ld=H + pad)
    y2g = kc.Guarded(M, 2 * H, BF16, ld=2 * H + pad, init=1.0)        # y2 = the right half of a [M, 2H] buffer
    tdt = F16 if dt == F16 else F32
    twin, c_twin = kc.guarded(M, H, tdt)
    xhat, c_xhat = kc.guarded(M, H, BF16)
    rstd2, c_rstd = kc.guarded(1, M, F32)
    rstd = rstd2[0]
    k.ln_fwd(x, bias, res, gamma, beta, y, y2=y2g.view[:, H:], xhat=xhat, rstd=rstd, eps=eps, p_drop=p, seed=SEED,
             **({"y_f16": twin} if dt == F16 else {"y_f32": twin}))
    mask = k.dropout_mask(M * H, p, SEED, "cuda").view(M, H).double() if p > 0 else torch.ones(M, H, dtype=torch.float64, device="cuda")
    x64, r64 = x0.double().cuda(), r0.double().cuda()
    b64 = torch.zeros(H, dtype=torch.float64, device="cuda") if bias0 is None else bias0.double().cuda()
    s = (x64 + b64) * mask + r64
    t_abs = (x64.abs() + b64.abs()) * mask + r64.abs()
    b = kc.ln_fwd_bounds(t_abs, s, gamma0.cuda(), beta0.cuda(), eps)
    kc.assert_within(y, *b["y"], what + " y", verbose=False)
    kc.assert_within(twin, b["y_raw"][0], kc.stored(b["y_raw"][1], b["y_raw"][0], tdt), what + " twin", verbose=False)
    kc.assert_within(xhat, *b["xhat"], what + " xhat", verbose=False)
    kc.assert_within(rstd, *b["rstd"], what + " rstd", verbose=False)
    _bits_equal(y2g.view[:, H:], y, what + " y2")
    assert bool((y2g.view[:, :H] == 1.0).all()), what + ": the left half of the [M, 2H] buffer was written"
    for c, n in ((c_y, "y"), (y2g.check, "y2"), (c_twin, "twin"), (c_xhat, "xhat"), (c_rstd, "rstd")):
        c(what="%s %s" % (what, n))
    # backward from the saved xhat / rstd (inputs of the backward: exact as given)
    dy0, dy20 = _rnd(M, H, seed=6).to(BF16), _rnd(M, H, seed=7).to(BF16)
    dy, dy2 = kc.guarded_input(dy0, ld=H + pad), kc.guarded_input(dy20, ld=H + pad)
    dres, c_dres = kc.guarded(M, H, BF16, ld=H + pad)
    dx, c_dx = kc.guarded(M, H, BF16, ld=H + pad)
    outs = [kc.guarded(1, H, F32, init=0.5) for _ in range(3)]
    (dg, c_dg), (db, c_db), (dbias, c_dbias) = outs
    ws = k.ln_bwd_workspace(H, "cuda")
    k.ln_bwd(dy, xhat, rstd, gamma, dy2=dy2, dres=dres, dx=dx, dgamma=dg[0], dbeta=db[0], dbias=dbias[0], partials=ws,
             p_drop=p, seed=SEED)
    bb = kc.ln_bwd_bounds(dy0.double().cuda() + dy20.double().cuda(), xhat, rstd, gamma0.cuda(), mask)
    kc.assert_within(dres, *bb["dres"], what + " dres", verbose=False)
    kc.assert_within(dx, *bb["dx"], what + " dx", verbose=False)
    half = torch.full((H,), 0.5, dtype=torch.float64, device="cuda")
    for name, t in (("dgamma", dg[0]), ("dbeta", db[0])):
        ref, e = kc.with_beta(bb[name][1], bb[name][0], 1.0, half)
        kc.assert_within(t, ref, kc.stored(e, ref, F32), what + " " + name, verbose=False)
    dx64 = dx.double()              # dbias is the column sum of the STORED dx
    ref, e = kc.with_beta((M + 4) * kc.U_ACC * dx64.abs().sum(0), dx64.sum(0), 1.0, half)
    kc.assert_within(dbias[0], ref, kc.stored(e, ref, F32), what + " dbias", verbose=False)
    for c, n in ((c_dres, "dres"), (c_dx, "dx"), (c_dg, "dgamma"), (c_db, "dbeta"), (c_dbias, "dbias"), (c_xhat, "xhat"), (c_rstd, "rstd")):
        c(what="%s %s" % (what, n))
    # the single-launch form (no dbias), overwrite mode
    (dg2, c_dg2), (db2, c_db2) = kc.guarded(1, H, F32), kc.guarded(1, H, F32)
    k.ln_bwd(dy, xhat, rstd, gamma, dy2=dy2, dres=dres, dx=dx, dgamma=dg2[0], dbeta=db2[0], partials=ws, p_drop=p, seed=SEED,
             accumulate=False)
    kc.assert_within(dg2[0], *bb["dgamma"], what + " dgamma", verbose=False)
    kc.assert_within(db2[0], *bb["dbeta"], what + " dbeta", verbose=False)
    kc.assert_within(dres, *bb["dres"], what + " dres", verbose=False)
    kc.assert_within(dx, *bb["dx"], what + " dx", verbose=False)
    for c, n in ((c_dres, "dres"), (c_dx, "dx"), (c_dg2, "dgamma"), (c_db2, "dbeta")):
        c(what="%s fused %s" % (what, n))


@pytest.mark.parametrize("M", [1, 5, 130])
@pytest.mark.parametrize("H", [8, 72, 520, 2048])
def test_ln_fwd_bwd_strided_guarded(H, M):
    k = _k()
    for dt in (BF16, F32, F16):
        for p in (0.0, 0.1):
            x0, r0 = _rnd(M, H, seed=1).to(dt), _rnd(M, H, seed=2).to(dt)
            _ln_case(k, M, H, dt, p, x0, r0, _rnd(H, seed=3).to(F32), what="ln %s" % str(dt)[6:])
    kc.report("ln H=%d M=%d" % (H, M))


def test_ln_rows_of_mean_100_and_an_all_zero_row():
    """f32 rows of mean 100 and deviation 1 at eps = 1e-12 (a one-pass variance would cancel), and an all-zero row whose
    y is beta exactly."""
    k = _k()
    M, H = 5, 520
    x0 = (_rnd(M, H, seed=1) + 100.0).to(F32)
    r0 = torch.zeros(M, H, dtype=F32)
    x0[2] = 0.0
    _ln_case(k, M, H, F32, 0.0, x0, r0, None, what="ln mean-100")
    beta0 = _rnd(H, seed=5).to(F32)
    y, c_y = kc.guarded(M, H, BF16, ld=H + 8)
    k.ln_fwd(kc.guarded_input(x0, ld=H + 8), None, None, _vec(_rnd(H, seed=4).to(F32) + 1.0), _vec(beta0), y, eps=1e-12)
    _bits_equal(y[2], beta0.to(BF16), "all-zero row")
    c_y(what="ln zero-row y")
    kc.report("ln mean-100 / zero row")


# ------------------------------------------------------------------------------------------------- other row kernels
@pytest.mark.parametrize("H", [8, 520])
@pytest.mark.parametrize("M", [5, 130])
def test_dropout_add_gate_bwd_colsum(M, H):
    k = _k()
    x0 = _rnd(M, H, seed=1).to(BF16)
    # dropout with its second copy
    x = kc.guarded_input(x0, ld=H + 8)
    (y, c_y), (y2, c_y2) = kc.guarded(M, H, BF16, ld=H + 8), kc.guarded(M, H, BF16, ld=H + 16)
    k.dropout(x, y, y2=y2, p_drop=0.1, seed=5)
    mask = k.dropout_mask(M * H, 0.1, 5, "cuda").view(M, H).double()
    ref = x0.double().cuda() * mask
    kc.assert_within(y, ref, kc.stored(kc.U_ACC * ref.abs(), ref, BF16), "dropout y")
    _bits_equal(y2, y, "dropout y2")
    c_y(what="dropout y"); c_y2(what="dropout y2")
    # add (flat, contiguous): bitwise
    a0, b0 = _rnd(M, H, seed=2).to(BF16), _rnd(M, H, seed=3).to(BF16)
    o, c_o = kc.guarded(1, M * H, BF16)
    k.add_bf16(_flat_in(a0), _flat_in(b0), o[0])
    _bits_equal(o[0], (a0.float() + b0.float()).to(BF16).reshape(-1), "add_bf16")
    c_o(what="add_bf16 out")
    # gate backward: strided dout / cross / dcross_in / dcross, contiguous g / du
    do0, g0 = _rnd(M, H, seed=4).to(BF16), torch.sigmoid(_rnd(M, H, seed=5)).to(BF16)
    cr0, ci0 = _rnd(M, H, seed=6).to(BF16), _rnd(M, H, seed=7).to(BF16)
    (du, c_du), (dc, c_dc) = kc.guarded(M, H, BF16), kc.guarded(M, H, BF16, ld=H + 8)
    k.gate_bwd(kc.guarded_input(do0, ld=H + 8), kc.guarded_input(g0), kc.guarded_input(cr0, ld=H + 16), du, dc,
               dcross_in=kc.guarded_input(ci0, ld=H + 24))
    d64, g64, c64, i64 = (t.double().cuda() for t in (do0, g0, cr0, ci0))
    ref = d64 * c64 * g64 * (1 - g64)          # four f32 roundings of the product
    kc.assert_within(du, ref, kc.stored(4 * kc.U_ACC * ref.abs(), ref, BF16), "gate_bwd du")
    ref = d64 * g64 + i64
    kc.assert_within(dc, ref, kc.stored(2 * kc.U_ACC * ((d64 * g64).abs() + i64.abs()), ref, BF16), "gate_bwd dcross")
    c_du(what="gate_bwd du"); c_dc(what="gate_bwd dcross")
    # column sums: ragged N inside a padded leading dimension, accumulate into ones
    for N, ld in ((H, H + 8), (13, 16)) if H > 8 else ((8, 8), (5, 8)):
        xs0 = _rnd(M, N, seed=8).to(BF16)
        out, c_out = kc.guarded(1, N, F32, init=1.0)
        k.colsum(kc.guarded_input(xs0, ld=ld), out[0], k.colsum_workspace(N, "cuda"), accumulate=True)
        x64 = xs0.double().cuda()
        ref, e = kc.with_beta((M + 4) * kc.U_ACC * x64.abs().sum(0), x64.sum(0), 1.0, torch.ones(N, dtype=torch.float64, device="cuda"))
        kc.assert_within(out[0], ref, kc.stored(e, ref, F32), "colsum N=%d ld=%d" % (N, ld))
        c_out(what="colsum out")
    kc.report("row kernels M=%d H=%d" % (M, H))


@pytest.mark.parametrize("lds", [13, 17])
@pytest.mark.parametrize("M", [5, 130])
def test_cast_pad_zeroes_its_pad_columns_and_nothing_else(M, lds):
    k = _k()
    N, ldd = 13, 16
    s0 = _rnd(M, N, seed=1).to(F32)
    g = kc.Guarded(M, N, BF16, ld=ldd)
    dst = g.flat.as_strided((M, ldd), (ldd, 1), g.start)         # the launcher takes the contiguous [M, ldd] matrix
    k.cast_pad_f32_to_bf16(kc.guarded_input(s0, ld=lds), dst)
    _bits_equal(g.view, s0.to(BF16), "cast_pad values")
    g.check(tail_cols=ldd - N, expect=0, what="cast_pad dst")


def _token_ce_case(M, C):
    """logits, labels, mask and the float64 reference of a token-CE case.  A row COUNTS iff mask != 0 and 0 <= label < C in 64
    bits (include/icka_hip.h); the first valid rows (up to three, never the last one) carry the labels -100, C and 2^32 + 3,
    which do not count: their gradient rows are zero and they add nothing to the loss or the count.

    Bound of a gradient element (p = softmax probability, x the f32 logits, exact as given):  the exponent x_c - lse carries
    u (|x_c| + |lse|) from the subtraction and the error of lse -- u |mx| for max + log, 2 u for logf, (C + 4) u relative
    for the f32 sum of C exponentials, each of which has the 2 u of expf and u |x_c - mx| <= u (|x_c| + |mx|) in its own
    exponent (|mx| <= |lse| + log C).  Together  D_c = u (2 |x_c| + 3 |lse| + 3 log C + C + 8), and
    e_g = p expm1(D_c) + 2 u p (expf) + u |g| (the onehot subtraction), then the store.  The loss of a row is
    lse - x_y: D_y + u |loss|; the sum adds the rows in any order: (M + 4) u sum|loss|."""
    x0 = _rnd(M, C, seed=1, scale=3.0).to(F32)
    labels0 = torch.randint(0, C, (M,), generator=torch.Generator().manual_seed(2))
    mask0 = (torch.arange(M) % 3 != 1).long()
    mask0[0] = 1
    rows = torch.nonzero(mask0)[:, 0].tolist()
    for row, lab in zip(rows[:len(rows) - 1], (-100, C, 2 ** 32 + 3)):      # (the last valid row always stays in range)
        labels0[row] = lab
    counts0 = (mask0 != 0) & (labels0 >= 0) & (labels0 < C)
    x = x0.double().cuda()
    lse = torch.logsumexp(x, -1, keepdim=True)
    p = torch.exp(x - lse)
    valid = counts0.double().cuda()[:, None]
    onehot = torch.nn.functional.one_hot(torch.where(counts0, labels0, torch.zeros_like(labels0)), C).double().cuda() * valid
    ref = (p - onehot) * valid
    D = kc.U_ACC * (2 * x.abs() + 3 * lse.abs() + 3 * math.log(C) + C + 8)
    e = (p * torch.expm1(D) + 2 * kc.U_ACC * p + kc.U_ACC * ref.abs()) * valid
    loss = (lse - (x * onehot).sum(-1, keepdim=True)) * valid
    e_loss = ((D * onehot).sum(-1, keepdim=True) + kc.U_ACC * loss.abs()) * valid
    return dict(x0=x0, labels0=labels0, mask0=mask0, n=int(counts0.sum()), ref=ref, e=e, loss_sum=loss.sum(),
                e_sum=e_loss.sum() + (M + 4) * kc.U_ACC * loss.abs().sum())


@pytest.mark.parametrize("C,ldd,ld", [(13, 16, 13), (13, 16, 16), (9, 16, 12), (8, 8, 8)])
@pytest.mark.parametrize("M", [1, 5, 130, 300])
def test_token_ce_zeroes_its_pad_columns_and_nothing_else(M, C, ldd, ld):
    """icka_token_ce: dlogits bf16 [M, ldd] = (softmax - onehot) * valid on the C logical columns, ZEROS in the pad columns
    [C, ldd) of every row; loss_sum / count accumulate over the rows that count (``_token_ce_case``).  M = 300 takes two
    blocks."""
    k = _k()
    t = _token_ce_case(M, C)
    logits = kc.guarded_input(t["x0"], ld=ld)
    g = kc.Guarded(M, C, BF16, ld=ldd)
    dl = g.flat.as_strided((M, ldd), (ldd, 1), g.start)
    (acc, c_acc) = kc.guarded(1, 2, F32, init=torch.tensor([[0.5, 2.0]]))
    k.token_ce(logits, t["labels0"].cuda(), t["mask0"].cuda(), acc[0, 0:1], acc[0, 1:2], dl)
    kc.assert_within(g.view, t["ref"], kc.stored(t["e"], t["ref"], BF16), "token_ce dlogits")
    g.check(tail_cols=ldd - C, expect=0, what="token_ce dlogits")
    ref_sum, e_sum = kc.with_beta(t["e_sum"], t["loss_sum"], 1.0, torch.tensor(0.5, dtype=torch.float64, device="cuda"))
    ref_sum, e_sum = ref_sum.reshape(1), e_sum.reshape(1)
    kc.assert_within(acc[0, 0:1], ref_sum, kc.stored(e_sum, ref_sum, F32), "token_ce loss_sum")
    assert float(acc[0, 1]) == 2.0 + t["n"]
    c_acc(what="token_ce accumulators")
    kc.report("token_ce M=%d C=%d ldd=%d ld=%d" % (M, C, ldd, ld))


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("M", [5, 300])
def test_token_ce_fused_counts_the_same_rows(M, dt):
    """icka_token_ce_fused (per-block partials, fixed order): stats = {loss sum, rows that count, mean}; the gradient rows of
    the rows that do not count -- masked out, or a label outside [0, C) on a valid row -- are zero, pad columns too."""
    k = _k()
    C, ldd, ld = 13, 16, 16
    t = _token_ce_case(M, C)
    logits = kc.guarded_input(t["x0"], ld=ld)
    g = kc.Guarded(M, C, dt, ld=ldd)
    dl = g.flat.as_strided((M, ldd), (ldd, 1), g.start)
    stats, c_stats = kc.guarded(1, 3, F32)
    k.token_ce_fused(logits, t["labels0"].cuda(), t["mask0"].cuda(), stats[0], dl)
    kc.assert_within(g.view, t["ref"], kc.stored(t["e"], t["ref"], dt), "token_ce_fused dlogits")
    g.check(tail_cols=ldd - C, expect=0, what="token_ce_fused dlogits")
    ref_sum, e_sum = t["loss_sum"].reshape(1), kc.stored(t["e_sum"], t["loss_sum"], F32).reshape(1)
    kc.assert_within(stats[0, 0:1], ref_sum, e_sum, "token_ce_fused loss sum")
    assert float(stats[0, 1]) == t["n"]
    ref_mean = ref_sum / max(t["n"], 1)               # one more rounding: the division
    kc.assert_within(stats[0, 2:3], ref_mean, kc.stored(e_sum / max(t["n"], 1), ref_mean, F32), "token_ce_fused mean")
    c_stats(what="token_ce_fused stats")
    kc.report("token_ce_fused M=%d %s" % (M, str(dt)[6:]))


@pytest.mark.parametrize("n", [1, 7, 8, 1000003])
def test_casts_saturate_and_stay_inside_their_buffers(n):
    k = _k()
    s0 = _rnd(n, seed=1, scale=1e3).to(F32)
    edge = torch.tensor([65504.0, -65504.0, 65520.0, -65520.0, 1e6, -1e6, 3e38])
    s0[: min(n, edge.numel())] = edge[: min(n, edge.numel())]
    sat = lambda t: t.float().clamp(-65504.0, 65504.0).to(F16)
    (d, c_d), (dh, c_dh) = kc.guarded(1, n, BF16), kc.guarded(1, n, F16)
    k.cast_f32_to_bf16_f16(_flat_in(s0), d[0], dh[0])
    _bits_equal(d[0], s0.to(BF16), "cast_f32_to_bf16_f16 bf16")
    _bits_equal(dh[0], sat(s0), "cast_f32_to_bf16_f16 fp16")
    c_d(what="cast bf16"); c_dh(what="cast fp16")
    for src in (s0, s0.to(BF16)):
        dh, c_dh = kc.guarded(1, n, F16)
        k.cast_to_f16(_flat_in(src), dh[0])
        _bits_equal(dh[0], sat(src), "cast_to_f16 from %s" % src.dtype)
        c_dh(what="cast_to_f16 dst")


@pytest.mark.parametrize("C", [8, 520])
@pytest.mark.parametrize("R", [1, 49])
def test_region_tokens_and_transpose_bitwise(R, C):
    k = _k()
    Bn = 2
    f0 = _rnd(Bn * R * C, seed=1, scale=100.0).to(F32)
    f0[0] = 1e6          # saturates in the fp16 twin
    for layout in (0, 1):
        (t, c_t), (t16, c_t16) = kc.guarded(Bn * R, C, BF16), kc.guarded(Bn * R, C, F16)
        k.regions_to_tokens_h(_flat_in(f0), t, t16, Bn, R, C, layout)
        ref = f0.view(Bn, R, C) if layout == 0 else f0.view(Bn, C, R).permute(0, 2, 1)
        ref = ref.reshape(Bn * R, C)
        _bits_equal(t, ref.to(BF16), "regions_to_tokens_h bf16 layout %d" % layout)
        _bits_equal(t16, ref.clamp(-65504.0, 65504.0).to(F16), "regions_to_tokens_h fp16 layout %d" % layout)
        c_t(what="region tokens"); c_t16(what="region tokens fp16")


@pytest.mark.parametrize("R,C", [(1, 8), (49, 72)])
def test_transpose_bitwise(R, C):
    k = _k()
    s0 = _rnd(2, R, C, seed=1).to(BF16)
    d, c_d = kc.guarded(1, 2 * R * C, BF16)
    k.transpose_bf16(_flat_in(s0), d[0], 2, R, C)
    _bits_equal(d[0].view(2, C, R), s0.transpose(1, 2).contiguous(), "transpose_bf16")
    c_d(what="transpose dst")
