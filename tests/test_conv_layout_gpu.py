"""GPU: the ResNet layout kernels (stem patches, 3x3 patch matrix, subsample, max-pool, features_out) against torch on the
same bf16 values: moved values bitwise, zeros in rows [rows, rows_padded) and in patch columns 147..191, guard bands intact
after rows_padded (tests/kernel_check.py).  Operands sit in NaN bands."""
import pytest
import torch
import torch.nn.functional as F

import kernel_check as kc
from kernel_check import BF16, F32

pytestmark = pytest.mark.gpu

B = 2
SIZES = [(7, 7), (15, 9), (16, 16)]


def _k():
    from icka_amd import kernels
    return kernels


def _rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _pad128(n):
    return (n + 127) // 128 * 128


def _flat_in(values):
    return kc.guarded_input(values.reshape(1, -1))[0]


def _bits_equal(out, ref, what):
    idt = torch.int32 if out.dtype == F32 else torch.int16
    same = out.contiguous().view(idt) == ref.to(out.device).contiguous().view(idt)
    assert bool(same.all()), "%s: %d of %d elements differ bitwise" % (what, int((~same).sum()), same.numel())


def _patches(nchw, ksize, pad, stride):
    """torch.unfold -> [B * L, taps * C] with k = tap * C + c (the kernels' patch layout)"""
    Bn, C = nchw.shape[:2]
    u = F.unfold(nchw.float(), ksize, padding=pad, stride=stride)             # [B, C * taps, L], channel-major
    return u.view(Bn, C, ksize * ksize, -1).permute(0, 3, 2, 1).reshape(-1, ksize * ksize * C)


@pytest.mark.parametrize("H,W", SIZES)
def test_stem_patches(H, W):
    K = _k()
    img = _rnd(B, 3, H, W, seed=1).to(F32)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    rows, rp = B * Ho * Wo, _pad128(B * Ho * Wo)
    g = kc.Guarded(rows, 192, BF16)
    lib, xin = K._lib.load(), _flat_in(img)            # (xin stays referenced until the last launch that reads it)
    K.check(lib.icka_conv_stem_patches(xin.data_ptr(), g.view.data_ptr(), B, H, W, rp, K._stream()), "icka_conv_stem_patches")
    ref = torch.zeros(rows, 192)
    ref[:, :147] = _patches(img.to(BF16), 7, 3, 2)
    _bits_equal(g.view, ref.to(BF16), "stem patches (columns 147..191 are zero)")
    g.check(tail_rows=rp - rows, expect=0, what="stem patches")
    # a size the launcher refuses: the refusal is the assertion
    assert lib.icka_conv_stem_patches(xin.data_ptr(), g.view.data_ptr(), B, 6, 7, rp, K._stream()) != 0
    assert lib.icka_conv_stem_patches(xin.data_ptr(), g.view.data_ptr(), B, H, W, rows - 1, K._stream()) != 0
    g.check(tail_rows=rp - rows, expect=0, what="stem patches after refused calls")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", SIZES)
def test_im2col_subsample_maxpool(H, W, stride):
    K = _k()
    lib = K._lib.load()
    C = 64
    x = _rnd(B, H, W, C, seed=2).to(BF16)                  # NHWC
    nchw = x.permute(0, 3, 1, 2)
    xin = _flat_in(x)
    # 3x3 / pad 1 patch matrix
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    rows, rp = B * Ho * Wo, _pad128(B * Ho * Wo)
    g = kc.Guarded(rows, 9 * C, BF16)
    K.check(lib.icka_conv_im2col3x3(xin.data_ptr(), g.view.data_ptr(), B, H, W, C, stride, rp, K._stream()), "icka_conv_im2col3x3")
    _bits_equal(g.view, _patches(nchw, 3, 1, stride).to(BF16), "im2col3x3")
    g.check(tail_rows=rp - rows, expect=0, what="im2col3x3")
    # subsample
    Hs, Ws = (H - 1) // stride + 1, (W - 1) // stride + 1
    rows, rp = B * Hs * Ws, _pad128(B * Hs * Ws)
    g = kc.Guarded(rows, C, BF16)
    K.check(lib.icka_conv_subsample(xin.data_ptr(), g.view.data_ptr(), B, H, W, C, stride, rp, K._stream()), "icka_conv_subsample")
    _bits_equal(g.view, x[:, ::stride, ::stride, :].reshape(rows, C), "subsample")
    g.check(tail_rows=rp - rows, expect=0, what="subsample")
    if stride == 2:     # nn.MaxPool2d(3, 2, 1): the kernel has this one stride
        Hp, Wp = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        rows, rp = B * Hp * Wp, _pad128(B * Hp * Wp)
        g = kc.Guarded(rows, C, BF16)
        K.check(lib.icka_conv_maxpool3x3s2(xin.data_ptr(), g.view.data_ptr(), B, H, W, C, rp, K._stream()), "icka_conv_maxpool3x3s2")
        ref = F.max_pool2d(nchw.float(), 3, 2, 1).permute(0, 2, 3, 1).reshape(rows, C)
        _bits_equal(g.view, ref.to(BF16), "maxpool3x3s2")
        g.check(tail_rows=rp - rows, expect=0, what="maxpool3x3s2")
        assert lib.icka_conv_maxpool3x3s2(xin.data_ptr(), g.view.data_ptr(), B, H, W, C, rows - 1, K._stream()) != 0
        assert lib.icka_conv_maxpool3x3s2(xin.data_ptr(), g.view.data_ptr(), B, H, W, C + 4, rp, K._stream()) != 0
        g.check(tail_rows=rp - rows, expect=0, what="maxpool3x3s2 after refused calls")


@pytest.mark.parametrize("H,W", SIZES)
def test_features_out(H, W):
    K = _k()
    C, P = 64, H * W
    rows = _rnd(P, seed=4).abs()[None, :, None] * 2.0 ** -(torch.arange(C) % 12).float()     # channels span magnitudes
    x = (_rnd(B, P, C, seed=3) * rows).to(BF16)
    (att, c_att), (fc, c_fc), (tok, c_tok) = kc.guarded(B * C, P, F32), kc.guarded(B, C, F32), kc.guarded(B * P, C, BF16)
    xin = _flat_in(x)
    K.check(K._lib.load().icka_conv_features_out(xin.data_ptr(), att.data_ptr(), fc.data_ptr(), tok.data_ptr(), B, P, C,
                                                 K._stream()), "icka_conv_features_out")
    _bits_equal(att, x.permute(0, 2, 1).float().reshape(B * C, P), "features_out att")
    _bits_equal(tok, x.reshape(B * P, C), "features_out tokens")
    x64 = x.double().cuda()
    ref = x64.mean(1)
    # f32 sum of P terms in any order, then one division: (P + 4) u sum|x| / P, stored in f32
    kc.assert_within(fc, ref, kc.stored((P + 4) * kc.U_ACC * x64.abs().sum(1) / P, ref, F32), "features_out fc")
    c_att(what="features_out att"); c_fc(what="features_out fc"); c_tok(what="features_out tokens")
    kc.report("features_out %dx%d" % (H, W))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("residual", ["none", "plain", "scaled"])
@pytest.mark.parametrize("rows", [1, 98, 128, 200])
def test_bn_apply_zeroes_its_tail_rows_and_nothing_else(rows, residual, relu):
    """icka_bn_apply: y = [relu](raw * scale + shift [+ r]) on rows < rows_valid and ZEROS on [rows_valid, rows_padded), whatever
    raw holds there (NaN here); nothing after rows_padded.  Error of the unrounded value: one f32 rounding for each of the
    (at most) five operations, charged on the absolute terms, then the bf16 store."""
    K = _k()
    C, rp = 64, _pad128(rows)
    raw0 = torch.full((rp, C), float("nan"), dtype=BF16)
    raw0[:rows] = (_rnd(rows, C, seed=1) * 2.0 ** -(torch.arange(rows) % 12).float()[:, None]).to(BF16)
    res0 = torch.full((rp, C), float("nan"), dtype=BF16)
    res0[:rows] = _rnd(rows, C, seed=2).to(BF16)
    vec = lambda seed: _rnd(C, seed=seed).to(F32)
    sc0, sh0, rs0, rb0 = vec(3), vec(4), vec(5), vec(6)
    raw, res = kc.guarded_input(raw0), kc.guarded_input(res0)
    sc, sh, rs, rb = (kc.guarded_input(t.reshape(1, -1))[0] for t in (sc0, sh0, rs0, rb0))
    nbt = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    g = kc.Guarded(rows, C, BF16)
    out = g.flat.as_strided((rp, C), (C, 1), g.start)          # the launcher takes the whole [rows_padded, C] matrix
    K.bn_apply(raw, sc, sh, rows, relu=relu, residual=None if residual == "none" else res,
               res_scale=rs if residual == "scaled" else None, res_shift=rb if residual == "scaled" else None, nbt=(nbt,), out=out)
    d = lambda t: t.double().cuda()
    main, r = d(raw0[:rows]) * d(sc0), torch.zeros(rows, C, dtype=torch.float64, device="cuda")
    e_r = torch.zeros_like(r)
    if residual != "none":
        r = d(res0[:rows])
        if residual == "scaled":
            e_r = 2 * kc.U_ACC * ((r * d(rs0)).abs() + d(rb0).abs())
            r = r * d(rs0) + d(rb0)
    ref = main + d(sh0) + r
    e = e_r + 3 * kc.U_ACC * (main.abs() + d(sh0).abs() + r.abs())
    if relu:
        ref = ref.clamp_min(0)          # 1-Lipschitz
    kc.assert_within(g.view, ref, kc.stored(e, ref, BF16), "bn_apply y")
    g.check(tail_rows=rp - rows, expect=0, what="bn_apply y")
    assert int(nbt) == 42
    kc.report("bn_apply rows=%d residual=%s relu=%d" % (rows, residual, relu))
