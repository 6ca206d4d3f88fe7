"""CPU: keeps tests/conv_check.py honest.  A plain torch-f32 emulation performs each kernel's operations in the kernel's own
summation structure -- the implicit convolution's gather with the loader's index arithmetic and its k-tiles in (tap, channel
block) order, the two-pass slice sums of bn_stats_tile, bn_chan_merge in slice order and then tile order, the 16 slices of
bn_finalize_kernel -- and at every case tests/test_conv_elements_gpu.py runs on the device it must stay inside every bound, and
so must the reference itself.  Then planted faults, one at a time, each emulated as the faulty kernel would behave: each must
leave a bound or break an exact check in at least one of those cases -- a fault that stays inside means the shapes or the bound
are too weak to trust the GPU test.  Last, the references are tied to torch: conv2d, BatchNorm2d and F.batch_norm in float64."""
import pytest
import torch
import torch.nn.functional as F

import conv_check as cc
import kernel_check as kc
from conv_check import BF16, F32, F64, BM


def caught(fn):
    """the check fails (a bound is left or an exact comparison breaks)"""
    try:
        fn()
    except AssertionError:
        kc._PENDING.clear()
        return True
    kc._PENDING.clear()
    return False


def f32(x):
    return torch.tensor(x, dtype=F32)


# ---------------------------------------------------------------------------------------- the kernels' summation forms
def gemm_f32(a, w):
    """[M, K] x [N, K]^T in f32: the k-steps of 32 (one MFMA each) in order"""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
    for k in range(0, a.shape[1], 32):
        acc = acc + a[:, k:k + 32].float() @ w[:, k:k + 32].float().t()
    return acc


def gather(x, stride, rp, fault=None):
    """The CONV loader of gemm_ws_body: the [rows_padded, 9 C] patch matrix it stages, k-tile by k-tile, from the NHWC map with its
    own index arithmetic (row m -> sample, output pixel, centre input pixel, the 9-bit mask of taps inside the image; a tap
    outside, and every tap of a padded row, reads the zero page).  A faulty address outside the map reads zero here."""
    B, H, W, C = x.shape
    Ho, Wo = cc.out_hw(H, W, stride)
    rows = B * Ho * Wo
    flat = torch.cat([x.reshape(B * H * W, C), torch.zeros(1, C, dtype=x.dtype)])            # last row: the zero page
    m = torch.arange(rp)
    mm = torch.where(m < rows, m, 0)
    hw = H * W if (fault == "sample_from_HW" and stride == 2) else Ho * Wo
    b = mm // hw
    r = mm - b * hw
    oy = r // Wo
    ox = r - oy * Wo
    s = 1 if fault == "centre_stride_1" else stride
    y0, x0 = oy * s, ox * s
    ctr = (b * H + y0) * W + x0
    out = torch.zeros(rp, 9, C, dtype=x.dtype)
    for t in range(9):
        y, xx = y0 + t // 3 - 1, x0 + t % 3 - 1
        ok = (m < rows) & (y >= 0) & (y < H)
        if fault != "border_wraps":
            ok = ok & (xx >= 0) & (xx < W)
        at = ctr + (t // 3 - 1) * W + (t % 3 - 1)
        ok = ok & (at >= 0) & (at < B * H * W)
        out[:, t] = flat[torch.where(ok, at, B * H * W)]
    if fault == "second_block_repeats" and C == 128:
        out[:, :, 64:] = out[:, :, :64]
    return out.reshape(rp, 9 * C)


def emu_epilogue(acc, c, inp):
    v = acc
    if c["bias"]:
        v = v + inp["bias"]
    if c["epi"] in ("ADD", "ADD_RELU"):
        v = v + inp["aux"].float()
    if c["epi"] in ("RELU", "ADD_RELU"):
        v = v.clamp_min(0)
    return v.to(BF16)


def emu_merge(st, nb, mb, m2b, fault=None):
    """bn_chan_merge in f32"""
    n, mu, m2 = st
    live = nb != 0
    nn = n + nb
    d = mb - mu
    f = nb / torch.where(live, nn, torch.ones_like(nn))
    mu2 = mu + d * f
    t = d * d * n * f
    m22 = m2 + (m2b + (torch.zeros_like(t) if fault == "no_between_term" else t))
    return torch.where(live, nn, n), torch.where(live, mu2, mu), torch.where(live, m22, m2)


def emu_stats(acc, rows_valid, bnt, fault=None):
    """bn_stats_tile on f32 accumulators [M, N] -> partials [3, M / 128, N]"""
    M, N = acc.shape
    nq = 512 // bnt
    rq = BM // nq
    part = torch.zeros(3, M // BM, N, dtype=F32)
    for t in range(M // BM):
        nv = BM if fault == "counts_padded_rows" else min(max(rows_valid - t * BM, 0), BM)
        st = (torch.zeros(N, dtype=F32),) * 3
        for q in range(nq):
            r0, r1 = q * rq, min(q * rq + rq, nv)
            cnt = max(r1 - r0, 0)
            rows = list(range(t * BM + r0, t * BM + r1))
            if fault == "last_row_dropped":
                rows = rows[:-1]
            s = torch.zeros(N, dtype=F32)
            for r in rows:
                s = s + acc[r]
            mean = s / f32(float(cnt)) if cnt else torch.zeros(N, dtype=F32)
            m2 = torch.zeros(N, dtype=F32)
            for r in rows:
                d = acc[r] - mean
                m2 = m2 + d * d
            st = emu_merge(st, torch.full((N,), float(cnt), dtype=F32), mean, m2, fault)
        part[0, t], part[1, t], part[2, t] = st
    return part


def emu_finalize(part, weight, bias, rm, rv, nbt, momentum, eps, fault=None):
    """bn_finalize_kernel in f32: thread (c, j) merges tiles j, j + 16, .., then slice 0 merges slices 1 .. 15 in order"""
    _, tiles, C = part.shape
    slices = []
    for ty in range(16):
        st = (torch.zeros(C, dtype=F32),) * 3
        for t in range(ty, tiles, 16):
            st = emu_merge(st, part[0, t], part[1, t], part[2, t])
        slices.append(st)
    n, mu, m2 = slices[0]
    for j in range(1, 16):
        n, mu, m2 = emu_merge((n, mu, m2), *slices[j])
    one = f32(1.0)
    var = torch.where(n > 0, m2 / torch.where(n > 0, n, one), torch.zeros_like(m2))
    sc = weight * (one / torch.sqrt(var + f32(eps)))
    shift = bias - (mu if fault == "shift_without_scale" else mu * sc)
    if momentum is None:
        m = one / f32(float(nbt if fault == "cumulative_1_over_nbt" else nbt + 1))
    else:
        m = f32(momentum)
    unb = torch.where(n > 1, var * (n / torch.where(n > 1, n - one, one)), var)
    if fault == "biased_running_var":
        unb = var
    keep = {"old_ignored": f32(0.0), "old_weighted_by_m": m}.get(fault, one - m)
    return {"scale": sc, "shift": shift, "running_mean": m * mu + keep * rm, "running_var": m * unb + keep * rv}


# ------------------------------------------------------------------------------------------------------- the checks
def check_conv(c, fault=None):
    inp = cc.conv_inputs(c)
    _, _, rows, rp = cc.conv_dims(c)
    out = emu_epilogue(gemm_f32(gather(inp["x"], c["stride"], rp, fault), inp["w"]), c, inp)
    ref, bound = cc.conv_refs(c, inp)
    kc.assert_within(out[:rows], ref, bound, "cpu conv3x3 y", verbose=False)
    cc.same_bits(out[rows:], cc.conv_pad_rows(c, inp), "cpu conv3x3 padded rows")
    if fault is None:
        kc.assert_within(ref.to(BF16), ref, bound, "cpu conv3x3 y (reference)", verbose=False)


def check_stats(acc32, acc, E, rows_valid, what, fault=None):
    bnt = cc.tile_width(acc.shape[1])
    refs = cc.stats_refs(acc, E, rows_valid, bnt)
    kc.assert_within(acc32.to(BF16), acc, cc.stored(E, acc, BF16), what + " raw", verbose=False)
    cc.compare_partials(emu_stats(acc32, rows_valid, bnt, fault), refs, what)
    if fault is None:
        cc.compare_partials(torch.stack([refs["count"], refs["mean"][0], refs["m2"][0]]).float(), refs, what + " (reference)")
    return refs


def check_gemm_stats(c, fault=None):
    inp = cc.gemm_inputs(c)
    what = "cpu gemm_bn_stats" + (" exact" if c["exact"] else "")
    return check_stats(gemm_f32(inp["a"], inp["w"]), inp["acc"], cc.gemm_E(c, inp), c["rv"], what, fault)


def check_conv_stats(c, fault=None):
    inp = cc.conv_inputs(c)
    _, _, rows, rp = cc.conv_dims(c)
    pad = lambda t: torch.cat([t, torch.zeros(rp - rows, c["Cout"], dtype=F64)])
    acc32 = gemm_f32(gather(inp["x"], c["stride"], rp, fault), inp["w"])
    assert not bool(acc32[rows:].ne(0).any())
    check_stats(acc32, pad(inp["acc"]), kc.gemm_acc_bound(pad(inp["abs"]), 9 * c["C"]), rows, "cpu conv3x3_stats", fault)


def check_fin(c, fault=None):
    inp = cc.fin_inputs(c)
    args = (inp["part"], inp["weight"], inp["bias"], inp["rm"], inp["rv"], c["nbt"], c["momentum"], c["eps"])
    refs = cc.finalize_refs(*args)
    cc.compare_finalize(emu_finalize(*args, fault=fault), refs, "cpu bn_finalize")
    if fault is None:
        cc.compare_finalize({k: refs[k][0].float() for k in ("scale", "shift", "running_mean", "running_var")}, refs,
                            "cpu bn_finalize (reference)")
    return refs


# -------------------------------------------------------------------------------- (a) the emulations stay inside
@pytest.mark.parametrize("B,H,W", cc.MAPS)
def test_conv_emulation_inside_at_every_shape_case(B, H, W):
    for c in cc.conv_shape_cases(B, H, W):
        check_conv(c)
    kc.report("cpu conv3x3 %dx%dx%d" % (B, H, W))


def test_conv_emulation_inside_at_every_option_case():
    for c in cc.CONV_OPTION_CASES:
        check_conv(c)
    kc.report("cpu conv3x3 options")


@pytest.mark.parametrize("K,N", cc.GEMM_STATS_KN)
def test_gemm_stats_emulation_inside(K, N):
    for c in cc.gemm_stats_cases(K, N):
        check_gemm_stats(c)
    # the device test's last case: NaN accumulators in the tile without a valid row stay out of the partials
    c = cc.gcase(384, N, K, 130)
    inp = cc.gemm_inputs(c)
    acc32 = gemm_f32(inp["a"], inp["w"])
    acc32[256:] = float("nan")
    refs = cc.stats_refs(inp["acc"], kc.gemm_acc_bound(inp["abs"], K), 130, cc.tile_width(N))
    cc.compare_partials(emu_stats(acc32, 130, cc.tile_width(N)), refs, "cpu gemm_bn_stats")
    kc.report("cpu gemm_bn_stats K=%d N=%d" % (K, N))


def test_gemm_stats_emulation_inside_at_strided_large_mean_and_exact_cases():
    for c in cc.GEMM_STATS_LD_CASES + cc.GEMM_STATS_BIG_CASES + cc.GEMM_STATS_EXACT_CASES:
        check_gemm_stats(c)
    for c in cc.GEMM_STATS_EXACT_CASES:      # exact means exact: the f32 accumulators of the emulation are the float64 ones
        inp = cc.gemm_inputs(c)
        assert torch.equal(gemm_f32(inp["a"], inp["w"]).double(), inp["acc"]) and float(inp["acc"].abs().max()) < 2 ** 24
    for c in cc.GEMM_STATS_BIG_CASES:        # the case is what it claims: column means ~ 50 x the column spread
        v = cc.gemm_inputs(c)["acc"][:c["rv"]]
        ratio = v.mean(0).abs() / v.std(0)
        assert float(ratio.min()) > 25 and float(ratio.median()) > 40, (float(ratio.min()), float(ratio.median()))
    kc.report("cpu gemm_bn_stats strides, large mean, exact")


@pytest.mark.parametrize("B,H,W", cc.MAPS)
def test_conv_stats_emulation_inside(B, H, W):
    for c in cc.CONV_STATS_CASES:
        if (c["B"], c["H"], c["W"]) == (B, H, W):
            check_conv_stats(c)
    kc.report("cpu conv3x3_stats %dx%dx%d" % (B, H, W))


@pytest.mark.parametrize("tiles", cc.FIN_TILES)
def test_finalize_emulation_inside(tiles):
    for C in cc.FIN_C:
        for c in cc.fin_cases(tiles, C):
            check_fin(c)
    kc.report("cpu bn_finalize tiles=%d" % tiles)


def test_finalize_emulation_inside_at_special_cases_and_what_the_header_promises():
    for c in cc.FIN_SPECIAL_CASES:
        refs = check_fin(c)
        inp = cc.fin_inputs(c)
        m = 1.0 / (c["nbt"] + 1) if c["momentum"] is None else cc.f32_of(c["momentum"])
        if c["kind"] == "one":
            assert bool((refs["n"] == 1).all()) and not bool(refs["var"][0].ne(0).any())
            assert torch.equal(refs["running_var"][0], (1 - m) * inp["rv"].double())
        if c["kind"] == "none":
            assert not bool(refs["n"].ne(0).any())
            assert torch.equal(refs["shift"][0], inp["bias"].double())
            assert torch.equal(refs["scale"][0], inp["weight"].double() / torch.sqrt(torch.tensor(cc.f32_of(c["eps"]), dtype=F64)))
            assert torch.equal(refs["running_mean"][0], (1 - m) * inp["rm"].double())
    kc.report("cpu bn_finalize special cases")


def _chain():
    c = cc.CHAIN
    inp = cc.gemm_inputs(c)
    fi = cc.fin_inputs(cc.fcase(2, c["N"], cc.CHAIN_MOMENTUM, 0, cc.CHAIN_EPS))
    return c, inp, fi


def test_chain_emulation_inside():
    c, inp, fi = _chain()
    ref, bound, fr = cc.chain_refs(inp, c["rv"], fi["weight"], fi["bias"], fi["rm"], fi["rv"], 0, cc.CHAIN_MOMENTUM, cc.CHAIN_EPS)
    acc32 = gemm_f32(inp["a"], inp["w"])
    part = emu_stats(acc32, c["rv"], cc.tile_width(c["N"]))
    o = emu_finalize(part, fi["weight"], fi["bias"], fi["rm"], fi["rv"], 0, cc.CHAIN_MOMENTUM, cc.CHAIN_EPS)
    cc.compare_finalize(o, fr, "cpu chain")
    y = (acc32.to(BF16).float()[:c["rv"]] * o["scale"] + o["shift"]).clamp_min(0).to(BF16)
    kc.assert_within(y, ref, bound, "cpu chain y", verbose=False)
    kc.assert_within(ref.to(BF16), ref, bound, "cpu chain y (reference)", verbose=False)
    # the propagated bound is not vacuous: a shift without the scale leaves it
    bad = (acc32.to(BF16).float()[:c["rv"]] * o["scale"] + (fi["bias"] - fr["mean"][0].float())).clamp_min(0).to(BF16)
    assert caught(lambda: kc.assert_within(bad, ref, bound, "cpu chain y, shift = bias - mean", verbose=False))
    kc.report("cpu chain")


# ------------------------------------------------------------------------------------------- (c) planted faults
def _some(cases, check, fault):
    return [c for c in cases if caught(lambda: check(c, fault))]


def test_planted_statistics_faults_are_caught():
    gemm = [c for K, N in cc.GEMM_STATS_KN for c in cc.gemm_stats_cases(K, N)] + cc.GEMM_STATS_BIG_CASES + cc.GEMM_STATS_EXACT_CASES
    # 1. the padded rows counted: every case with rows_valid short of M
    hit = _some(gemm, check_gemm_stats, "counts_padded_rows")
    assert len(hit) == sum(1 for c in gemm if c["rv"] < c["M"]), "statistics that count the padded rows"
    # 2. the last valid row of a slice dropped from the sums: every case
    assert len(_some(gemm, check_gemm_stats, "last_row_dropped")) == len(gemm), "the last valid row of a slice dropped"
    assert len(_some(cc.CONV_STATS_CASES, check_conv_stats, "last_row_dropped")) == len(cc.CONV_STATS_CASES)
    # 3. the between-slice term of the merge dropped: wherever a tile has two live slices
    hit = _some(gemm, check_gemm_stats, "no_between_term")
    two = [c for c in gemm if c["rv"] > BM // (512 // cc.tile_width(c["N"]))]
    assert two and all(c in hit for c in two), "the term d^2 n f of the merge dropped"


def test_planted_finalize_faults_are_caught():
    cases = [c for t in cc.FIN_TILES for C in cc.FIN_C for c in cc.fin_cases(t, C)] + cc.FIN_SPECIAL_CASES
    moving = [c for c in cases if c["momentum"] != 0.0 and c["kind"] in ("rand", "big")]
    # 4. biased running_var: wherever the running statistics move
    hit = _some(cases, check_fin, "biased_running_var")
    assert all(c in hit for c in moving), "biased instead of unbiased running_var"
    # 5. the old running value ignored (visible unless momentum is 1 -- or cumulative from zero batches) or weighted by m
    hit = _some(cases, check_fin, "old_ignored")
    assert all(c in hit for c in cases if c["momentum"] in (0.0, 0.1) or (c["momentum"] is None and c["nbt"] == 4)), "old ignored"
    hit = _some(cases, check_fin, "old_weighted_by_m")
    assert all(c in hit for c in cases if c["momentum"] in (0.0, 0.1) or (c["momentum"] is None and c["nbt"] == 4)), "old weighted by m"
    # 6. the cumulative average with 1 / nbt: every cumulative case (1 / 0 at nbt = 0)
    hit = _some(cases, check_fin, "cumulative_1_over_nbt")
    assert all(c in hit for c in cases if c["momentum"] is None) and any(c["momentum"] is None for c in cases), "1 / nbt"
    # 7. shift = bias - mean
    hit = _some(cases, check_fin, "shift_without_scale")
    assert all(c in hit for c in cases if c["kind"] in ("rand", "big")), "shift = bias - mean"


def test_planted_gather_faults_are_caught():
    conv = [c for (B, H, W) in cc.MAPS for c in cc.conv_shape_cases(B, H, W)] + cc.CONV_OPTION_CASES
    # 8. a border tap that wraps to the neighbouring row: every map more than one pixel wide
    hit = _some(conv, check_conv, "border_wraps")
    assert all(c in hit for c in conv if c["W"] > 1 and c["B"] * c["H"] > 1), "a border tap that wraps"
    # 9. the stride-2 centre taken at stride 1: every stride-2 case with more than one output pixel per sample
    hit = _some(conv, check_conv, "centre_stride_1")
    assert all(c in hit for c in conv if c["stride"] == 2 and c["H"] * c["W"] > 2), "the stride-2 centre taken at stride 1"
    assert not [c for c in hit if c["stride"] == 1]
    # 10. the second channel block of a tap repeating the first: every case with C = 128
    hit = _some(conv, check_conv, "second_block_repeats")
    assert hit == [c for c in conv if c["C"] == 128], "the second channel block repeating the first"
    # 11. the sample index from H * W under stride 2: every stride-2 case with more than one sample and pixel
    hit = _some(conv, check_conv, "sample_from_HW")
    assert all(c in hit for c in conv if c["stride"] == 2 and c["B"] > 1 and c["H"] * c["W"] > 1), "the sample index from H * W"
    # the statistics variant sees a gather fault too (its raw output and its partials)
    c = cc.ccase(3, 5, 7, 128, 128, 2, bias=False)
    assert c in cc.CONV_STATS_CASES
    for fault in ("border_wraps", "centre_stride_1", "second_block_repeats", "sample_from_HW"):
        assert caught(lambda: check_conv_stats(c, fault)), fault


# ------------------------------------------------------------------------------- (b) the references against torch's own
def test_references_equal_torch_float64():
    # the patch layout k = (ky * 3 + kx) * C + c: the gather of the emulation times w^T is conv2d
    for c in (cc.ccase(3, 5, 7, 128, 64, 2), cc.ccase(1, 15, 9, 64, 64, 1), cc.ccase(2, 1, 9, 64, 64, 2)):
        inp = cc.conv_inputs(c)
        _, _, rows, rp = cc.conv_dims(c)
        p = gather(inp["x"], c["stride"], rp).double()
        assert float((p[:rows] @ inp["w"].double().t() - inp["acc"]).abs().max()) < 1e-12
        assert float((p[:rows].abs() @ inp["w"].double().abs().t() - inp["abs"]).abs().max()) < 1e-12
        u = F.unfold(inp["x"].double().permute(0, 3, 1, 2), 3, padding=1, stride=c["stride"])
        u = u.view(c["B"], c["C"], 9, -1).permute(0, 3, 2, 1).reshape(rows, 9 * c["C"])
        assert torch.equal(u, p[:rows])
    # tile statistics: torch's mean / var of the tile's valid rows; pooled over the tiles: of all valid rows
    gc = cc.gcase(384, 64, 64, 130)
    inp = cc.gemm_inputs(gc)
    st = cc.stats_refs(inp["acc"], kc.gemm_acc_bound(inp["abs"], 64), 130, 64)
    assert float((st["mean"][0][1] - inp["acc"][128:130].mean(0)).abs().max()) < 1e-13
    assert float((st["m2"][0][0] - 128 * inp["acc"][:128].var(0, unbiased=False)).abs().max()) < 1e-10
    assert not bool(st["count"][2].ne(0).any()) and not bool(st["mean"][0][2].ne(0).any())
    part = torch.stack([st["count"], st["mean"][0], st["m2"][0]])
    n, mean, m2 = cc.pooled(part)
    v = inp["acc"][:130]
    assert float((mean - v.mean(0)).abs().max()) < 1e-13 and float((m2 / n - v.var(0, unbiased=False)).abs().max()) < 1e-12
    # finalize: nn.BatchNorm2d in float64, every momentum form
    C = 64
    for momentum, nbt, eps in ((0.1, 0, 1e-5), (1.0, 0, 1e-3), (0.0, 0, 1e-5), (None, 0, 1e-5), (None, 4, 1e-3)):
        fi = cc.fin_inputs(cc.fcase(2, C, momentum, nbt, eps))
        bn = torch.nn.BatchNorm2d(C, eps=cc.f32_of(eps), momentum=None if momentum is None else cc.f32_of(momentum)).double().train()
        with torch.no_grad():
            bn.weight.copy_(fi["weight"]); bn.bias.copy_(fi["bias"]); bn.running_mean.copy_(fi["rm"]); bn.running_var.copy_(fi["rv"])
            bn.num_batches_tracked.fill_(nbt)
            y = bn(v.t().reshape(1, C, 130, 1))[0, :, :, 0].t()
        fr = cc.finalize_refs(part, fi["weight"], fi["bias"], fi["rm"], fi["rv"], nbt, momentum, eps)
        assert float((v * fr["scale"][0] + fr["shift"][0] - y).abs().max()) < 1e-11
        assert float((fr["running_mean"][0] - bn.running_mean).abs().max()) < 1e-13
        assert float((fr["running_var"][0] - bn.running_var).abs().max()) < 1e-13
    # the chained reference is F.batch_norm + ReLU by construction; its scale / shift reproduce it
    c, inp, fi = _chain()
    ref, _, fr = cc.chain_refs(inp, c["rv"], fi["weight"], fi["bias"], fi["rm"], fi["rv"], 0, cc.CHAIN_MOMENTUM, cc.CHAIN_EPS)
    assert float(((inp["acc"][:c["rv"]] * fr["scale"][0] + fr["shift"][0]).clamp_min(0) - ref).abs().max()) < 1e-11
