"""GPU: every GEMM kernel element by element against float64, every tensor inside guard bands (tests/kernel_check.py).

Operands (A, B, A2, B2, aux, bias, bias2) sit in NaN bands with NaN pad columns: a result that depends on anything outside
an operand's logical shape turns non-finite.  Outputs (out, out2, out3, colsum_out) start as NaN inside sentinel bands: a
tile left out shows, and so does a store one row or column past the logical shape.  Row i of A is scaled by 2^-(i % 12), so
that an error in a small row cannot hide behind the largest element of the matrix."""
import pytest
import torch

import kernel_check as kc
from kernel_check import BF16, F16, F32

pytestmark = pytest.mark.gpu

EPIS = ["NONE", "GELU", "DGELU", "ADD", "GATE", "TANH", "RELU", "ADD_RELU"]
NEEDS_AUX = ("DGELU", "ADD", "GATE", "ADD_RELU")
# the options every epilogue runs with on the general path
OPTIONS = ["bias", "bias2", "alpha", "beta_bf16", "beta_f32", "f16_out3", "aux_f16"]


def _k():
    from icka_amd import kernels
    return kernels


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _vec(values):
    """contiguous f32 [N] inside NaN bands"""
    return kc.guarded_input(values.reshape(1, -1).to(F32))[0]


class Case:
    """One GEMM problem: logical A [M, K], B [N, K] (second segment: the trailing K2 columns), stored as the op wants them."""

    def __init__(self, op, M, N, K, *, K2=0, pad=0, offset=0, ab=BF16, seed=0, scale=1.0):
        k = _k()
        self.k, self.op, self.M, self.N, self.K, self.K2, self.pad, self.ab = k, op, M, N, K, K2, pad, ab
        rows = (2.0 ** -(torch.arange(M) % 12).float())[:, None]
        Al = (_rnd(M, K + K2, seed=seed + 1, scale=scale) * rows).to(ab)
        Bl = _rnd(N, K + K2, seed=seed + 2, scale=scale).to(ab)
        self.A64, self.B64 = Al.double().cuda(), Bl.double().cuda()
        self.acc = self.A64 @ self.B64.t()
        self.absprod = self.A64.abs() @ self.B64.abs().t()
        sa = (lambda x: x.t().contiguous()) if op == "TN" else (lambda x: x.contiguous())
        sb = (lambda x: x.contiguous()) if op == "NT" else (lambda x: x.t().contiguous())
        gi = lambda x: kc.guarded_input(x, ld=x.shape[1] + pad, offset=offset)
        self.A, self.B = gi(sa(Al[:, :K])), gi(sb(Bl[:, :K]))
        self.A2 = self.B2 = None
        if K2:
            self.A2, self.B2 = gi(sa(Al[:, K:])), gi(sb(Bl[:, K:]))
        self.kop = {"NT": k.GEMM_NT, "NN": k.GEMM_NN, "TN": k.GEMM_TN}[op]
        self.bias = _rnd(N, seed=seed + 3).to(F32)
        self.bias2 = _rnd(N, seed=seed + 4).to(F32)
        self.aux = {BF16: _rnd(M, N, seed=seed + 5).to(BF16), F16: _rnd(M, N, seed=seed + 5).to(F16)}
        self.c_old = _rnd(M, N, seed=seed + 6)

    def run(self, epi, option, *, tune=0, pad_out=None, odt=None, what=""):
        k, M, N = self.k, self.M, self.N
        pad16 = self.pad if pad_out is None else pad_out[0]
        pad32 = self.pad if pad_out is None else pad_out[1]
        bias = self.bias
        bias2 = self.bias2 if option == "bias2" else None
        alpha = 0.5 if option == "alpha" else 1.0
        beta = 1.0 if option in ("beta_bf16", "beta_f32") else 0.0
        if odt is None:
            odt = {"beta_f32": F32, "f16_out3": F16}.get(option, BF16)
        aux = self.aux[F16 if option == "aux_f16" else BF16] if epi in NEEDS_AUX else None
        z = alpha * self.acc + (bias.double().cuda() if bias is not None else 0.0) + (bias2.double().cuda() if bias2 is not None else 0.0)
        E = kc.gemm_acc_bound(self.absprod, self.K + self.K2, alpha, None if bias is None else bias.cuda(),
                              None if bias2 is None else bias2.cuda())
        aux64 = None if aux is None else aux.double().cuda()
        ref, ref2 = kc.epilogue_ref(epi, z, aux64)
        e, e2 = kc.epilogue_bounds(epi, z, E, aux64)
        kw = dict(epilogue=getattr(k, "EPI_" + epi), alpha=alpha, beta=beta, tune=tune)
        if bias is not None:
            kw["bias"] = _vec(bias)
        if bias2 is not None:
            kw["bias2"] = _vec(bias2)
        if aux is not None:
            kw["aux"] = kc.guarded_input(aux, ld=N + pad16)
        if self.K2:
            kw["A2"], kw["B2"] = self.A2, self.B2
        c_old = None
        if beta:
            c_old = self.c_old.to(odt)
            ref, e = kc.with_beta(e, ref, beta, c_old.double().cuda())
        out, check = kc.guarded(M, N, odt, ld=N + (pad32 if odt == F32 else pad16), init=c_old)
        checks = [("out", check)]
        out2 = out3 = None
        if epi in ("GELU", "GATE"):
            out2, c2 = kc.guarded(M, N, BF16, ld=N + pad16)
            kw["out2"] = out2; checks.append(("out2", c2))
        if odt == F16:
            out3, c3 = kc.guarded(M, N, BF16, ld=N + pad16)
            kw["out3"] = out3; checks.append(("out3", c3))
        k.gemm(self.kop, self.A, self.B, out, **kw)
        tag = "%s %s %s %s" % (what, epi, option, str(odt)[6:])
        kc.assert_within(out, ref, kc.stored(e, ref, odt), "gemm %s %s" % (what, epi), verbose=False)
        if out2 is not None:
            kc.assert_within(out2, ref2, kc.stored(e2, ref2, BF16), "gemm %s %s out2" % (what, epi), verbose=False)
        if out3 is not None:     # the bf16 copy is rounded from the same unrounded value, not from the fp16 one
            kc.assert_within(out3, ref, kc.stored(e, ref, BF16), "gemm %s %s out3" % (what, epi), verbose=False)
        for name, c in checks:
            c(what="%s %s" % (tag, name))


def _options(epi):
    for o in OPTIONS:
        if o == "aux_f16" and epi not in NEEDS_AUX:
            continue
        if o == "beta_f32" and epi in ("GATE", "TANH"):
            continue        # sigmoid / tanh: the 2^-12 allowance is a requirement for 16-bit outputs only
        yield o


# ---------------------------------------------------------------------------------------------------- general path
@pytest.mark.parametrize("pad", [3, 4, 8])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (100, 13, 72), (129, 130, 65), (77, 200, 13)])
@pytest.mark.parametrize("op", ["NT", "NN", "TN"])
def test_general_path_every_epilogue_and_option(op, M, N, K, pad):
    """gemm_kernel<.., ALIGNED=false>: ragged shapes, leading dimensions cols + 3 (scalar branches of load4 / store4_bf16 and
    of the operand loader), cols + 4 (their 8-byte branches) and cols + 8."""
    c = Case(op, M, N, K, pad=pad)
    for epi in EPIS:
        for o in _options(epi):
            c.run(epi, o, what="general " + op)
    kc.report("general %s %dx%dx%d ld+%d" % (op, M, N, K, pad))


@pytest.mark.parametrize("op", ["NT", "NN", "TN"])
def test_general_path_aligned_shape_with_a_pointer_offset_of_two_elements(op):
    c = Case(op, 128, 128, 64, pad=8, offset=2)
    assert c.A.data_ptr() % 16 == 4
    for epi in EPIS:
        for o in ("bias", "beta_f32") if epi not in ("GATE", "TANH") else ("bias",):
            c.run(epi, o, what="general offset " + op)
    kc.report("general offset %s" % op)


@pytest.mark.parametrize("M,N", [(100, 13), (129, 130)])
@pytest.mark.parametrize("op", ["NT", "NN", "TN"])
def test_general_path_dual_k_segment(op, M, N):
    """K1 = 64 from A / B plus a second segment of 40 from A2 / B2 (a k-tail inside the second segment)."""
    c = Case(op, M, N, 64, K2=40, pad=3)
    for epi in EPIS:
        for o in ("bias", "alpha", "beta_f32") if epi not in ("GATE", "TANH") else ("bias", "alpha"):
            c.run(epi, o, what="general dual-K " + op)
    kc.report("general dual-K %s %dx%d" % (op, M, N))


@pytest.mark.parametrize("pad", [3, 4, 8])
def test_general_path_fp16_operands(pad):
    c = Case("NT", 100, 13, 72, pad=pad, ab=F16)
    for epi in EPIS:
        for o in _options(epi):
            c.run(epi, o, what="general fp16 NT")
    kc.report("general fp16 NT 100x13x72 ld+%d" % pad)


# ---------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("Kt", [960, 1024, 1100])
def test_split_k_boundary_strided_c_and_k_tail(Kt, beta):
    """TN, f32, no epilogue, M = 13 (operand padded to 16 columns), N = 200, ldc = 203: 15 k-tiles (no split), 16 (split) and
    18 over 4 splits with a short last split and a 12-wide k-tail.  Atomics only reorder the sum: the same bound E."""
    k = _k()
    M, N = 13, 200
    rows = (2.0 ** -(torch.arange(M) % 12).float())[:, None]
    Al, Bl = (_rnd(M, Kt, seed=1) * rows).to(BF16), _rnd(N, Kt, seed=2).to(BF16)
    A = kc.guarded_input(Al.t().contiguous(), ld=16)
    B = kc.guarded_input(Bl.t().contiguous(), ld=N)
    c_old = _rnd(M, N, seed=3).to(F32)
    out, check = kc.guarded(M, N, F32, ld=203, init=c_old if beta else None)
    k.gemm(k.GEMM_TN, A, B, out, beta=beta)
    A64, B64 = Al.double().cuda(), Bl.double().cuda()
    ref, e = A64 @ B64.t(), kc.gemm_acc_bound(A64.abs() @ B64.abs().t(), Kt)
    if beta:
        ref, e = kc.with_beta(e, ref, beta, c_old.double().cuda())
    kc.assert_within(out, ref, kc.stored(e, ref, F32), "gemm split-K TN f32")
    check(what="split-K out")
    kc.report("split-K Kt=%d beta=%g" % (Kt, beta))


# -------------------------------------------------------------------------------------------------------- fast paths
FAST_EPIS = ["NONE", "GELU", "DGELU", "ADD"]


def _fast(c, tune, what):
    for epi in FAST_EPIS:
        c.run(epi, "bias", tune=tune, pad_out=(8, 4), what=what)
        c.run(epi, "bias", tune=tune, pad_out=(8, 4), odt=F32, what=what)
        c.run(epi, "alpha", tune=tune, pad_out=(8, 4), what=what)
    c.run("NONE", "beta_f32", tune=tune, pad_out=(8, 4), what=what)
    c.run("NONE", "beta_bf16", tune=tune, pad_out=(8, 4), what=what)


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("tile_n", [96, 128])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192)])
@pytest.mark.parametrize("op", ["NT", "NN"])
def test_fast_path_tiles_into_strided_guarded_outputs(op, M, N, K, tile_n, direct):
    """128x96 / 128x128 tiles of the warp-specialised kernels, direct and LDS-staged epilogues; operands at ld = K + 8 (N + 8),
    outputs at ld = N + 8 (16-bit) / N + 4 (f32): alignment holds, so the fast path is still the one that runs."""
    k = _k()
    c = Case(op, M, N, K, pad=8, scale=0.5)
    _fast(c, k.gemm_tune(tile_n=tile_n, direct_epilogue=bool(direct)), "fast " + op)
    kc.report("fast %s %dx%dx%d tile_n=%d direct=%d" % (op, M, N, K, tile_n, direct))


def _w3_tile_n(M, N, K):
    """Tile width the default heuristic of launch() (csrc/gemm.hip) gives an aligned NT / NN bf16-output call on the 12-wave
    kernel, or 0 where it stays on the 128-wide kernels.  Restated here so that a shape which stops selecting the kernel it
    is meant for fails this test instead of quietly testing another kernel:
      256x192 tiles: M % 256 == 0, N % 192 == 0, K <= 1024, the tile count nb3 a multiple of 8, >= 128 and filling at least
                     3/4 of its last round of 256 CUs;
      256x128 tiles: otherwise, M % 256 == 0 and 192 <= (M / 256) (N / 128) <= 256, a multiple of 8 (N % 96 == 0 does not
                     matter at the default tile width)."""
    if M % 256 == 0 and N % 192 == 0 and K <= 1024:
        nb3 = (M // 256) * (N // 192)
        if nb3 % 8 == 0 and nb3 >= 128 and 4 * nb3 >= 3 * 256 * ((nb3 + 255) // 256):
            return 192
    if M % 256 == 0 and N % 128 == 0:
        nb2 = (M // 256) * (N // 128)
        if nb2 % 8 == 0 and 192 <= nb2 <= 256:
            return 128
    return 0


@pytest.mark.parametrize("M,N,K,tile_n", [(2048, 3072, 64, 128), (2048, 3072, 1088, 128), (3072, 3072, 64, 192)])
@pytest.mark.parametrize("op", ["NT", "NN"])
def test_fast_path_12_wave_kernel(op, M, N, K, tile_n):
    """gemm_w3_kernel in both forms.  2048 x 3072 has 128 tiles of 256x192, half a round of the 256 CUs, so at K = 64 as at
    K = 1088 (> 1024) it runs the 256x128 form (192 tiles); 3072 x 3072 x 64 has 192 tiles of 256x192, 3/4 of a round, and
    runs the 256x192 form with its staged epilogue stores.  The plain f32 output with a short reduction stays on the
    128-wide kernel (direct epilogue) unless the 256x192 form takes the shape."""
    assert _w3_tile_n(M, N, K) == tile_n
    c = Case(op, M, N, K, pad=8, scale=0.5)
    what = "w3 %d-wide %s" % (tile_n, op)
    for epi in FAST_EPIS:
        c.run(epi, "bias", pad_out=(8, 4), what=what)
    c.run("NONE", "bias", pad_out=(8, 4), odt=F32, what=what)
    kc.report("12-wave %s %dx%dx%d" % (op, M, N, K))


def test_fast_path_128x64_tiles():
    """M = 128, N = 64, K = 64, NT: everything aligned except N % 128."""
    c = Case("NT", 128, 64, 64, pad=8, scale=0.5)
    _fast(c, 0, "128x64 NT")
    kc.report("128x64-tile NT 128x64x64")


# -------------------------------------------------------------------------------------------------------- grouped TN
@pytest.mark.parametrize("big", [0, 1, 2])
def test_grouped_tn_into_guarded_outputs(big):
    """The four problems of test_gemm_grouped_matches_individual_launches plus its ragged fifth, fused column sums on the first
    two, every output and column-sum vector inside guard bands."""
    k = _k()
    T, H, I = 1024, 256, 512
    tune = k.gemm_tune(big_tiles=big)
    descs, post, keep = [], [], []
    for i, (m, n) in enumerate([(H, I), (I, H), (H, H), (3 * H, H), (13, H)]):
        rows = (2.0 ** -(torch.arange(m) % 12).float())[:, None]
        Al, Bl = (_rnd(m, T, seed=10 + i) * rows).to(BF16), _rnd(n, T, seed=20 + i).to(BF16)
        A = kc.guarded_input(Al.t().contiguous(), ld=m if m % 8 == 0 else 16)
        B = kc.guarded_input(Bl.t().contiguous(), ld=n)
        c_old = _rnd(m, n, seed=30 + i).to(F32)
        out, check = kc.guarded(m, n, F32, ld=n + 4, init=c_old)
        kw = {}
        cs = cs_check = None
        if i < 2:
            cs2d, cs_check = kc.guarded(1, m, F32, init=2.0 if i == 0 else None)
            cs = cs2d[0]
            kw = dict(colsum_out=cs, colsum_accumulate=(i == 0))
        descs.append(k.gemm_desc(k.GEMM_TN, A, B, out, beta=1.0, tune=tune, **kw))
        keep.append((A, B, out, cs))
        post.append((i, Al, Bl, c_old, out, check, cs, cs_check))
    k.gemm_grouped(descs)
    for i, Al, Bl, c_old, out, check, cs, cs_check in post:
        A64, B64 = Al.double().cuda(), Bl.double().cuda()
        ref, e = kc.with_beta(kc.gemm_acc_bound(A64.abs() @ B64.abs().t(), T), A64 @ B64.t(), 1.0, c_old.double().cuda())
        kc.assert_within(out, ref, kc.stored(e, ref, F32), "gemm grouped TN", verbose=False)
        check(what="grouped out %d" % i)
        if cs is not None:
            base = 2.0 if i == 0 else 0.0
            rcs = A64.sum(1) + base
            ecs = (T + 4) * kc.U_ACC * (A64.abs().sum(1) + base)
            kc.assert_within(cs, rcs, kc.stored(ecs, rcs, F32), "gemm grouped colsum", verbose=False)
            cs_check(what="grouped colsum %d" % i)
    kc.report("grouped TN big_tiles=%d" % big)
