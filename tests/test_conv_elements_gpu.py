"""GPU: the ResNet encoder's convolution and train-mode BatchNorm kernels element by element against float64 (references,
bounds and cases: tests/conv_check.py; tests/test_conv_check_cpu.py proves the bounds sound and not vacuous).  Every operand sits
in NaN bands, every output -- the partial statistics included -- in sentinel bands; the C entry points are called directly so
that leading dimensions, padded tiles and refusals can be expressed.

  icka_conv3x3_gemm          every (C, Cout, stride) on maps down to one pixel, all four epilogues, bias present and null, aux
                             at two row strides, whole tiles of padding; padded rows exact; refusals leave the output alone
  icka_gemm_bn_stats         raw output and EVERY (count, mean, M2) partial, rows_valid on either side of each slice and tile
                             boundary, row strides past the logical widths, accumulators of a large mean, integer accumulators
                             (exact in f32: the bound is then that of the slice sums and merges alone); refusals
  icka_conv3x3_gemm_stats    raw output bitwise the bias-less EPI_NONE convolution with exact zeros below, every partial
  icka_bn_finalize           synthetic partials (zero counts, unequal tiles), every momentum form with random old statistics
  the three launches of one layer chained, against F.batch_norm(training=True) + ReLU"""
import pytest
import torch

import conv_check as cc
import kernel_check as kc
from conv_check import BF16, F32, F64

pytestmark = pytest.mark.gpu


def _k():
    from icka_amd import kernels
    return kernels


def _vec(t):
    return kc.guarded_input(t.reshape(1, -1))[0]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(g):
    return g.flat.view(kc._INT[g.dtype]).clone()


def _untouched(g, before, what):
    assert torch.equal(g.flat.view(kc._INT[g.dtype]), before), what + ": a refused call wrote to the output"


# ================================================================================================== convolution
def _conv_operands(c, inp):
    """(x, w, bias or None, aux or None, ldaux, zeros): the zero page is exactly the 128 bytes the header asks for"""
    aux = kc.guarded_input(inp["aux"], ld=c["Cout"] + c["ldaux"]) if c["epi"] in ("ADD", "ADD_RELU") else None
    return (_vec(inp["x"]), kc.guarded_input(inp["w"]), _vec(inp["bias"]) if c["bias"] else None, aux,
            c["Cout"] + c["ldaux"] if aux is not None else 0, _vec(torch.zeros(64, dtype=BF16)))


def _conv_call(K, c, ops, y, rp, over=()):
    x, w, bias, aux, ldaux, zeros = ops
    a = dict(x=_ptr(x), w=_ptr(w), bias=_ptr(bias), aux=_ptr(aux), ldaux=ldaux, y=y, B=c["B"], H=c["H"], W=c["W"], C=c["C"],
             Cout=c["Cout"], stride=c["stride"], rp=rp, epi=getattr(K, "EPI_" + c["epi"]), zeros=_ptr(zeros))
    a.update(dict(over))
    return K._lib.load().icka_conv3x3_gemm(a["x"], a["w"], a["bias"], a["aux"], a["ldaux"], a["y"], a["B"], a["H"], a["W"], a["C"],
                                           a["Cout"], a["stride"], a["rp"], a["epi"], a["zeros"], K._stream())


def _run_conv(K, c):
    inp = cc.conv_inputs(c)
    _, _, rows, rp = cc.conv_dims(c)
    ops = _conv_operands(c, inp)
    g = kc.Guarded(rp, c["Cout"], BF16)
    K.check(_conv_call(K, c, ops, g.view.data_ptr(), rp), "icka_conv3x3_gemm")
    y = g.view.cpu()
    ref, bound = cc.conv_refs(c, inp)
    kc.assert_within(y[:rows], ref, bound, "conv3x3 y", verbose=False)
    cc.same_bits(y[rows:], cc.conv_pad_rows(c, inp), "conv3x3 padded rows " + cc.case_id(c))
    g.check(what="conv3x3 y " + cc.case_id(c))
    return g, ops


@pytest.mark.parametrize("B,H,W", cc.MAPS)
def test_conv3x3_every_element_at_every_shape(B, H, W):
    K = _k()
    for c in cc.conv_shape_cases(B, H, W):
        _run_conv(K, c)
    kc.report("conv3x3 %dx%dx%d" % (B, H, W))


def test_conv3x3_every_epilogue_bias_aux_stride_and_padded_tile():
    K = _k()
    for c in cc.CONV_OPTION_CASES:
        _run_conv(K, c)
    kc.report("conv3x3 options")


def test_conv3x3_refusals_leave_the_output_untouched():
    K = _k()
    c = cc.ccase(1, 15, 9, 64, 128, 1, epi="ADD_RELU", extra=1)            # 135 rows: rows_padded 384
    assert c in cc.CONV_OPTION_CASES
    g, ops = _run_conv(K, c)
    x, w, bias, aux, ldaux, zeros = ops
    y, before = g.view.data_ptr(), _bits(g)
    bad = [dict(C=96), dict(C=32), dict(Cout=96), dict(stride=3), dict(stride=0), dict(rp=128), dict(rp=200), dict(rp=136),
           dict(aux=None), dict(aux=None, epi=K.EPI_ADD), dict(ldaux=c["Cout"] + 4),
           dict(x=x.data_ptr() + 2), dict(w=w.data_ptr() + 2), dict(y=y + 2), dict(aux=aux.data_ptr() + 2),
           dict(bias=bias.data_ptr() + 4), dict(zeros=zeros.data_ptr() + 2)]
    for over in bad:
        assert _conv_call(K, c, ops, y, 384, over) != 0, "icka_conv3x3_gemm accepted %s" % over
    torch.cuda.synchronize()
    _untouched(g, before, "conv3x3")
    kc.report("conv3x3 refusals")


# =================================================================================================== statistics
def _gemm_stats_call(K, c, a, w, gy, gp, over=()):
    p = dict(a=a.data_ptr(), lda=c["K"] + c["lda"], w=w.data_ptr(), ldw=c["K"] + c["ldw"], y=gy.view.data_ptr(), ldy=c["N"] + c["ldy"],
             M=c["M"], N=c["N"], K=c["K"], rv=c["rv"], part=gp.view.data_ptr())
    p.update(dict(over))
    return K._lib.load().icka_gemm_bn_stats(p["a"], p["lda"], p["w"], p["ldw"], p["y"], p["ldy"], p["M"], p["N"], p["K"], p["rv"],
                                            p["part"], K._stream())


def _run_gemm_stats(K, c, nan_tile=False):
    inp = cc.gemm_inputs(c)
    M, N, Kd = c["M"], c["N"], c["K"]
    a0 = inp["a"]
    live = M
    if nan_tile:                     # a tile without a valid row: whatever ``a`` holds there stays out of the statistics
        live = cc.pad128(c["rv"])
        a0 = a0.clone()
        a0[live:] = float("nan")
    a, w = kc.guarded_input(a0, ld=Kd + c["lda"]), kc.guarded_input(inp["w"], ld=Kd + c["ldw"])
    gy, gp = kc.Guarded(M, N, BF16, ld=N + c["ldy"]), kc.Guarded(3 * (M // 128), N, F32)
    K.check(_gemm_stats_call(K, c, a, w, gy, gp), "icka_gemm_bn_stats")
    E = cc.gemm_E(c, inp)
    kc.assert_within(gy.view[:live], inp["acc"][:live], cc.stored(E, inp["acc"], BF16)[:live], "gemm_bn_stats raw", verbose=False)
    cc.compare_partials(gp.view.cpu().reshape(3, M // 128, N), cc.stats_refs(inp["acc"], E, c["rv"], cc.tile_width(N)), "gemm_bn_stats")
    gy.check(what="gemm_bn_stats raw " + cc.case_id(c))
    gp.check(what="gemm_bn_stats partials " + cc.case_id(c))
    return a, w, gy, gp


@pytest.mark.parametrize("Kd,N", cc.GEMM_STATS_KN)
def test_gemm_bn_stats_every_partial_around_every_slice_boundary(Kd, N):
    K = _k()
    for c in cc.gemm_stats_cases(Kd, N):
        _run_gemm_stats(K, c)
    _run_gemm_stats(K, cc.gcase(384, N, Kd, 130), nan_tile=True)
    kc.report("gemm_bn_stats K=%d N=%d" % (Kd, N))


def test_gemm_bn_stats_row_strides_large_mean_and_exact_accumulators():
    K = _k()
    for c in cc.GEMM_STATS_LD_CASES:
        _run_gemm_stats(K, c)
    kc.report("gemm_bn_stats strides")
    for c in cc.GEMM_STATS_BIG_CASES:
        _run_gemm_stats(K, c)
    kc.report("gemm_bn_stats large mean")
    for c in cc.GEMM_STATS_EXACT_CASES:
        _run_gemm_stats(K, c)
    kc.report("gemm_bn_stats exact accumulators")


def test_gemm_bn_stats_refusals_leave_the_outputs_untouched():
    K = _k()
    c = cc.gcase(256, 64, 64, 129, lda=8)
    a, w, gy, gp = _run_gemm_stats(K, c)
    by, bp = _bits(gy), _bits(gp)
    for over in (dict(M=200), dict(M=0), dict(N=96), dict(N=32), dict(K=32), dict(K=96), dict(rv=0), dict(rv=257), dict(lda=56),
                 dict(ldw=56), dict(ldy=56), dict(lda=68), dict(part=gp.view.data_ptr() + 4), dict(a=a.data_ptr() + 2),
                 dict(y=gy.view.data_ptr() + 2)):
        assert _gemm_stats_call(K, c, a, w, gy, gp, over) != 0, "icka_gemm_bn_stats accepted %s" % over
    torch.cuda.synchronize()
    _untouched(gy, by, "gemm_bn_stats raw")
    _untouched(gp, bp, "gemm_bn_stats partials")
    kc.report("gemm_bn_stats refusals")


@pytest.mark.parametrize("B,H,W", cc.MAPS)
def test_conv3x3_stats_raw_bitwise_and_every_partial(B, H, W):
    K = _k()
    lib = K._lib.load()
    for c in [c for c in cc.CONV_STATS_CASES if (c["B"], c["H"], c["W"]) == (B, H, W)]:
        inp = cc.conv_inputs(c)
        _, _, rows, rp = cc.conv_dims(c)
        ops = _conv_operands(c, inp)
        x, w, zeros = ops[0], ops[1], ops[5]
        gy, gp, ge = kc.Guarded(rp, c["Cout"], BF16), kc.Guarded(3 * (rp // 128), c["Cout"], F32), kc.Guarded(rp, c["Cout"], BF16)
        K.check(lib.icka_conv3x3_gemm_stats(x.data_ptr(), w.data_ptr(), gy.view.data_ptr(), B, H, W, c["C"], c["Cout"], c["stride"], rp,
                                            zeros.data_ptr(), gp.view.data_ptr(), K._stream()), "icka_conv3x3_gemm_stats")
        K.check(_conv_call(K, c, ops, ge.view.data_ptr(), rp), "icka_conv3x3_gemm")
        raw = gy.view.cpu()
        cc.same_bits(raw, ge.view, "conv3x3_stats raw against the bias-less EPI_NONE convolution")
        assert not bool(raw[rows:].view(torch.int16).ne(0).any()), "conv3x3_stats: padded rows are not exact zeros"
        pad = lambda t: torch.cat([t, torch.zeros(rp - rows, c["Cout"], dtype=F64)])
        E = pad(kc.gemm_acc_bound(inp["abs"], 9 * c["C"]))
        kc.assert_within(raw[:rows], inp["acc"], cc.stored(E[:rows], inp["acc"], BF16), "conv3x3_stats raw", verbose=False)
        cc.compare_partials(gp.view.cpu().reshape(3, rp // 128, c["Cout"]), cc.stats_refs(pad(inp["acc"]), E, rows, cc.tile_width(c["Cout"])),
                            "conv3x3_stats")
        for g, what in ((gy, "raw"), (gp, "partials"), (ge, "y")):
            g.check(what="conv3x3_stats %s %s" % (what, cc.case_id(c)))
    kc.report("conv3x3_stats %dx%dx%d" % (B, H, W))


# ===================================================================================================== finalize
def _run_finalize(K, c):
    inp = cc.fin_inputs(c)
    tiles, C = c["tiles"], c["C"]
    part = kc.guarded_input(inp["part"].reshape(3 * tiles, C))
    weight, bias = _vec(inp["weight"]), _vec(inp["bias"])
    g = {"running_mean": kc.Guarded(1, C, F32, init=inp["rm"].reshape(1, C)), "running_var": kc.Guarded(1, C, F32, init=inp["rv"].reshape(1, C)),
         "scale": kc.Guarded(1, C, F32), "shift": kc.Guarded(1, C, F32)}
    nbt = kc.Guarded(1, 1, torch.int64, init=torch.tensor([[c["nbt"]]]))
    K.check(K._lib.load().icka_bn_finalize(part.data_ptr(), tiles, C, weight.data_ptr(), bias.data_ptr(), g["running_mean"].view.data_ptr(),
                                           g["running_var"].view.data_ptr(), nbt.view.data_ptr(),
                                           -1.0 if c["momentum"] is None else c["momentum"], c["eps"], g["scale"].view.data_ptr(),
                                           g["shift"].view.data_ptr(), K._stream()), "icka_bn_finalize")
    refs = cc.finalize_refs(inp["part"], inp["weight"], inp["bias"], inp["rm"], inp["rv"], c["nbt"], c["momentum"], c["eps"])
    cc.compare_finalize({k: v.view.cpu()[0] for k, v in g.items()}, refs, "bn_finalize" + ("" if c["kind"] == "rand" else " " + c["kind"]))
    for k, v in g.items():
        v.check(what="bn_finalize %s %s" % (k, cc.case_id(c)))
    nbt.check(what="bn_finalize num_batches_tracked")
    assert int(nbt.view) == c["nbt"], "icka_bn_finalize changed num_batches_tracked"


@pytest.mark.parametrize("tiles", cc.FIN_TILES)
def test_bn_finalize_every_channel_at_every_momentum(tiles):
    K = _k()
    for C in cc.FIN_C:
        for c in cc.fin_cases(tiles, C):
            _run_finalize(K, c)
    kc.report("bn_finalize tiles=%d" % tiles)


def test_bn_finalize_large_mean_single_element_and_empty_batches():
    K = _k()
    for c in cc.FIN_SPECIAL_CASES:
        _run_finalize(K, c)
    kc.report("bn_finalize special")


# ======================================================================================================== chain
def test_stats_gemm_finalize_apply_chained_against_batch_norm():
    K = _k()
    lib = K._lib.load()
    c = cc.CHAIN
    M, N, rv = c["M"], c["N"], c["rv"]
    inp = cc.gemm_inputs(c)
    fi = cc.fin_inputs(cc.fcase(2, N, cc.CHAIN_MOMENTUM, 0, cc.CHAIN_EPS))
    a, w, gy, gp = _run_gemm_stats(K, c)
    weight, bias = _vec(fi["weight"]), _vec(fi["bias"])
    g = {"running_mean": kc.Guarded(1, N, F32, init=fi["rm"].reshape(1, N)), "running_var": kc.Guarded(1, N, F32, init=fi["rv"].reshape(1, N)),
         "scale": kc.Guarded(1, N, F32), "shift": kc.Guarded(1, N, F32)}
    nbt = kc.Guarded(1, 1, torch.int64, init=torch.tensor([[0]]))
    K.check(lib.icka_bn_finalize(gp.view.data_ptr(), M // 128, N, weight.data_ptr(), bias.data_ptr(), g["running_mean"].view.data_ptr(),
                                 g["running_var"].view.data_ptr(), nbt.view.data_ptr(), cc.CHAIN_MOMENTUM, cc.CHAIN_EPS,
                                 g["scale"].view.data_ptr(), g["shift"].view.data_ptr(), K._stream()), "icka_bn_finalize")
    out = kc.Guarded(rv, N, BF16)
    K.check(lib.icka_bn_apply(gy.view.data_ptr(), g["scale"].view.data_ptr(), g["shift"].view.data_ptr(), None, None, None,
                              out.view.data_ptr(), N, rv, M, 1, nbt.view.data_ptr(), None, K._stream()), "icka_bn_apply")
    ref, bound, fr = cc.chain_refs(inp, rv, fi["weight"], fi["bias"], fi["rm"], fi["rv"], 0, cc.CHAIN_MOMENTUM, cc.CHAIN_EPS)
    cc.compare_finalize({k: v.view.cpu()[0] for k, v in g.items()}, fr, "chain")
    kc.assert_within(out.view, ref, bound, "chain y", verbose=False)
    out.check(tail_rows=M - rv, expect=0, what="chain y")
    for k, v in g.items():
        v.check(what="chain " + k)
    nbt.check(what="chain num_batches_tracked")
    assert int(nbt.view) == 1
    kc.report("chain stats GEMM -> finalize -> apply")
