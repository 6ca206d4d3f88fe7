"""Helpers of the element-wise kernel tests (no test functions): guard-banded buffers, a per-element comparison against a
float64 reference, and error bounds DERIVED from the number formats (no fitted constants).

Worst err / bound ratios seen on an MI355X (the tests print them per case as "RATIO <test> <quantity> <ratio>"; a ratio
above 1 fails the test).  16-bit outputs sit just under 1 by construction: the last rounding alone takes half an ulp, which
is the eps_fmt |ref| term of the bound; f32 outputs show how much room the accumulation term leaves.

    GEMM, general path (NT / NN / TN, ld + 3 / + 4 / + 8), worst over options        main    out2    out3
      NONE / RELU                                                                    0.994     -     0.990
      GELU                                                                           0.975   0.994   0.956
      DGELU                                                                          0.985     -     0.957
      ADD / ADD_RELU                                                                 0.996     -     0.995
      GATE                                                                           0.986   0.884   0.926
      TANH                                                                           0.978     -     0.877
      pointer offset 0.990, dual K 0.990, fp16 operands 0.986
    GEMM, fast paths: 128x96 / 128x128 tiles 0.994, 128x64 tiles 0.993, 12-wave kernel: 256x128 tiles (2048 x 3072, K = 64
      and 1088) 0.996, 256x192 tiles (3072 x 3072 x 64) 0.996
    GEMM, f32 only: split-K 0.005, grouped TN 0.007, fused column sums < 0.001
    attention     out    out16    lse     dq      dk      dv     delta
      whole-head  0.645  0.985   0.109   0.522   0.652   0.922   0.085
      tiled       0.645  0.985   0.109   0.622   0.492   0.779   0.085
      packed      0.642    -     0.100   0.425   0.509   0.764   0.056   (samples of unequal length, up to 128 x 128)
    LayerNorm     y 0.994, twin 0.984 (fp16) / 0.055 (f32), xhat 0.990, rstd 0.046, dres 0.989, dx 0.989, dgamma 0.333,
                  dbeta 0.001, dbias 0.001; rows of mean 100: y 0.944, xhat 0.302, rstd < 0.001, dres / dx 0.974
    dropout 0.879, gate_bwd du / dcross 0.996, colsum 0.007, features_out fc 0.004; every data-movement kernel bitwise
    token_ce dlogits 0.991 (pad columns zero), loss_sum 0.020; bn_apply y 0.992 (tail rows zero)
    LSTM, step-wise (tests/lstm_check.py), worst over the cases of each form
      forward       y      c_all    act              backward   dgates_i  dgates_f  dgates_g  dgates_o  dc_carry
      LL          0.691  < 0.001   0.885             rs          0.988     0.985     0.984     0.899       -
      ticket      0.685  < 0.001   0.885             ticket      0.950     0.961     0.960     0.851       -
      per-step    0.691  < 0.001   0.885             per-step    0.961     0.954     0.963     0.861     0.004
      (y sits at 0.69, not just under 1: its bound carries the 2^-12 allowance of three device functions on top of the
      bf16 half-ulp, and the kernels' sigmoid / tanh use a small part of it.)  BiLSTM wiring: dW_ih 0.018, dW_hh 0.016,
      db 0.003, dx 0.896, the same after an accumulating second backward.
    CRF (tests/crf_check.py), against the float64 oracle, worst over the cases of each form ("mixed": the samples of the
    case took different forms; "either": the scaled form within 2^10 of giving up)
                          llh     de    d_start  d_end  d_trans             best_score / path
      scaled             0.059  0.312   0.059   0.078   0.037     small, staged     0.076
      log domain         0.090  0.627   0.090   0.062   0.064     small, unstaged   0.004
      mixed / either     0.009  0.000   0.030   0.031   0.023     LDS (C > 16)      0.054
      (worst-case bounds that grow with the chain: at 315 .. 512 positions every ratio is below 0.03; the 0.627 is a
      marginal of 1.1e-38 that the device flushes to zero, against the 2^-126 the bound grants for that.  Every integer case
      gave the exact path and score of the tie-rule reference.)
    fp32-exact (tests/exact_check.py), worst over the cases and both stride variants of each kernel
      x_gemm        C 0.299 (all four ops, K = 1 .. 50), batched 0.055; the gaps between batch slices untouched
      x_ln          y 0.135, xhat 0.059, rstd 0.057, dpre 0.135, ddense 0.126; rows of mean 100: y 0.003, dpre 0.015
      x_colsum      0.233
      x_embed       y 0.074, xhat 0.057, rstd 0.030; scatter dword 0.111, dpos 0.115, dtyp 0.090 (padding row bitwise)
      x_embed_prompt  y 0.099, xhat 0.057, rstd 0.055; scatter dword 0.112, dpos 0.122, dtyp 0.053 (dprompt bitwise)
      x_softmax     P 0.061, Pd 0.065, dS 0.155; a batch with every key at -10000: P / Pd 0.796
      x_act         gelu y 0.453, dx 0.654; tanh y 0.469, dx 0.492; gate y 0.596, y2 0.497, dx 0.696, dx2 0.999
      x_dropout 0.978, x_add 1.000, x_scale_by_ratio 0.595 (one or two roundings: the bound IS the half ulp);
      x_concat2 and x_regions_to_tokens bitwise
      x_sample_gate out 0.386, da 0.378, dc 0.437, dgate 0.117 (mode 1: the two words -t and +t bitwise)
      x_lstm_cell   act 0.471, c 0.367, y 0.248, dgates 0.386, dc_carry 0.445 (hprev bitwise the neighbouring y row)
      x_token_ce    dlogits 0.162, loss_sum 0.015, count exact (labels -100, C and 2^32 + 3 on valid rows: zero rows);
                    the fused form: dlogits 0.991 (bf16) / 0.162 (f32), loss sum and mean 0.016
      (the device's expf / logf / erff / tanhf meet the 2^-22 the bounds require of them: no replacement was needed.)
    gated head and contrastive objective (tests/head_check.py), worst over the cases and both stride variants of each kernel
      sample_gate   out 0.970, da 0.926, dc 0.821, dgate < 0.001 (its bound charges the 2^-12 sigmoid allowance on
                    sum|dout (a - c)|; mode 1 with one live block per sample: the two words -t and +t bitwise)
      sample_gate_fwd_h  out 0.937, out16 0.626 (+-65504 under a saturated gate stays +-65504)
      crs           forward crs 0.016; backward dseq 0.996, dcross 0.996, dW 0.140, dbias 0.035
      cls_head      forward logits 0.040 (bf16) / 0.046 (fp16); backward dseq 0.993, du 0.994, dcross 0.995, slab weight part
                    0.083, bias part < 0.001 (entries c >= C exactly zero); the slabs summed: dW 0.026, db 0.006
      contrastive   stats 0.226, ws 0.140, dt 0.024, dv 0.025, dcrs 0.265 (f32, bf16 and fp16 rows alike)
      (the device's __expf sigmoid meets the 2^-12, its expf / log1pf / expm1f the 2^-22 the bounds require of them.)
    embedding family and flat buffers (tests/embed_check.py), worst over the cases of each kernel
      embed         y 0.994, twin 0.993 (fp16; f32 below 0.1), xhat 0.993, rstd 0.060; backward dword 0.052, dtok 0.120,
                    dpos 0.100, dtype 0.043, dgamma 0.235, dbeta 0.281 (both backward kernels, n_type 1 .. 3, H 8 .. 2048;
                    untouched table rows and the padding row bitwise, dtok rows of the padding id exact zeros)
      embed_prompt  y 0.992, twin 0.078, xhat 0.972, rstd 0.043; dprompt 0.990 (bf16), dword 0.037, dpos 0.024, dtype 0.008,
                    dgamma 0.077, dbeta 0.023
      embed_scatter_rows  dword 0.087 (f32 and bf16 rows, T up to 4 x 4096 + 3)
      optim         sqnorm partials 0.004, norm 0.922 (f32 of a float64 sum: the bound IS the half ulp), coef < 0.001,
                    adamw p 0.254, m 0.303, v 0.278 (u = 2^-24 per operation); shadows bitwise from the stored p,
                    adamw_dev bitwise adamw
      dp casts      cast_chunks and cast_back_scaled bitwise (a NaN becomes 0x7fc0); copy_many, zero_f32 bitwise;
                    scalar_ratio 0.080, loss_accumulate exact
    convolution and train-mode BatchNorm (tests/conv_check.py), worst over the cases of each kernel
      conv3x3_gemm        y 0.973 (C 64 / 128, Cout 64 .. 192, both strides, maps from 1 x 1, all four epilogues, bias and null,
                          aux at ld Cout and Cout + 8; padded rows and whole padded tiles bitwise the epilogue of bias (+ aux))
      gemm_bn_stats       raw 0.996; partials: mean 0.008, M2 0.003, accumulators of a large mean: mean 0.023, M2 0.003 (the
                          worst-case accumulator error E carries these bounds); integer accumulators (E = 0: the slice sums and
                          merges alone): mean 0.014, M2 0.071; counts exact, tiles without a valid row (0, 0, 0)
      conv3x3_gemm_stats  raw 0.937 and bitwise the bias-less EPI_NONE convolution; mean < 0.001, M2 0.001
      bn_finalize         scale 0.220, shift 0.201, running_mean 0.246, running_var 0.238 (every momentum form, old statistics
                          random); tile means of 100: 0.101 / 0.055 / 0.065 / 0.128; n == 1: 0.175 / 0.174 / 0.231 / 0.158;
                          n == 0: 0.175 / 0 / 0.165 / 0.158; num_batches_tracked unchanged
      chain               stats GEMM -> finalize -> apply against F.batch_norm + ReLU: y 0.950 (scale / shift 0.001,
                          running_mean 0.008, running_var 0.028 of their propagated bounds)

No guard band was disturbed and no NaN pad reached a result in any case.  Two terms of the bounds go beyond the plain
roundoff sums, both named in the docstrings below: the GELU allowance is RELATIVE (1e-4 |gelu|) for z >= 1, as
tests/test_gelu_poly_cpu.py asserts it (the polynomial Phi is multiplied by z), and values below the smallest normal number
of the output format underflow (fp16 copies of attention outputs near 1e-8 become 0).

Known limits (stated again where they arise): the attention-backward bounds of dq / dk are no looser than the bar of the
existing test (3e-2 of the largest reference) at plain scores only -- see ``attn_bwd_bounds``; the LayerNorm forward bound
of rows with a large mean is looser than that test's bar from about H = 1000 on -- see ``ln_fwd_bounds``; the contrastive
gradient bounds, taken as a norm, are looser than the 1e-4 of tests/test_objective_gpu.py except at D = 8, temp = 1, and the
dgate bound of the per-sample gates is looser than 1e-2 from a few thousand elements per sample on and for saturated
gates -- see tests/head_check.py (tests/test_head_check_cpu.py asserts where).

Conventions
-----------
* ``guarded`` places a logical [rows, cols] matrix with row stride ``ld`` in the middle of ONE flat allocation that has at
  least GUARD_ROWS full rows in front of and behind it.  Everything outside the logical matrix -- the bands and the
  ``ld - cols`` pad columns of every row -- holds one bit pattern, and ``check()`` compares integer views against it.  The
  patterns are NaNs with a payload no arithmetic produces, so the same helper serves inputs: a result that depends on
  anything outside an operand's logical shape turns non-finite.
* ``assert_within`` takes a float64 reference computed by torch from the very (rounded) values the kernel reads, and a bound
  tensor built by the functions below.
* Unit roundoffs: bf16 2^-8, fp16 2^-11, f32 2^-24.  f32 ACCUMULATION is charged u = 2^-23 per operation: round-to-nearest
  with a factor 2 for a matrix core that truncates (which of the two it does is not measured here).
"""
import math

import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

GUARD_ROWS = 128
EPS = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}
U_ACC = 2.0 ** -23

_INT = {BF16: torch.int16, F16: torch.int16, F32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32,
        torch.int64: torch.int64}
# guard patterns (as the signed integer of the element's width).  SENTINEL: outputs; NAN_FILL: inputs.  Both are NaNs in
# every float format here, both differ from the canonical NaN a kernel could produce (0x7fc0 / 0x7e00 / 0x7fc00000).
SENTINEL = {BF16: 0x7FA5, F16: 0x7DA5, F32: 0x7FA5A5A5, torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A,
            torch.int64: 0x5A5A5A5A5A5A5A5A}
NAN_FILL = {BF16: 0x7FC1, F16: 0x7E01, F32: 0x7FC00001}


class Guarded:
    """view: the logical [rows, cols] tensor; flat: the whole allocation; check(): see ``guarded``."""

    def __init__(self, rows, cols, dtype, ld=None, offset=0, fill=None, device="cuda", init=None):
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.ld = max(cols, 1) if ld is None else ld
        if self.ld < cols:
            raise ValueError("ld < cols")
        self.fill = SENTINEL[dtype] if fill is None else fill
        self.start = GUARD_ROWS * self.ld + offset
        n = (2 * GUARD_ROWS + rows) * self.ld + offset
        n = (n + 7) // 8 * 8
        idt = _INT[dtype]
        bits = torch.full((n,), self.fill, dtype=idt, device=device)
        self.flat = bits.view(dtype)
        self.view = self.flat.as_strided((rows, cols), (self.ld, 1), self.start)
        if init is not None:
            self.view.copy_(init.to(dtype) if torch.is_tensor(init) else torch.full((rows, cols), init, dtype=dtype, device=device))
        elif dtype in (BF16, F16, F32):
            self.view.fill_(float("nan"))          # an output: a tile the kernel leaves out stays NaN

    def _inside(self, rows):
        m = torch.zeros(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        m.as_strided((rows, self.cols), (self.ld, 1), self.start).fill_(True)
        return m

    def check(self, tail_rows=0, tail_cols=0, expect=0, what="guard"):
        """Every byte outside the logical matrix is bit-identical to the fill.  ``tail_rows`` / ``tail_cols``: rows
        [rows, rows + tail_rows) x cols, and columns [cols, cols + tail_cols) of every logical row, belong to the kernel's
        documented contract instead and must hold the bit pattern ``expect`` exactly."""
        bits = self.flat.view(_INT[self.dtype])
        inside = self._inside(self.rows)
        contract = torch.zeros_like(inside)
        if tail_rows:
            contract.as_strided((tail_rows, self.cols), (self.ld, 1), self.start + self.rows * self.ld).fill_(True)
        if tail_cols:
            if self.cols + tail_cols > self.ld:
                raise ValueError("tail_cols past the row stride")
            contract.as_strided((self.rows, tail_cols), (self.ld, 1), self.start + self.cols).fill_(True)
        outside = ~(inside | contract)
        bad = outside & (bits != self.fill)
        if bool(bad.any()):
            at = int(torch.nonzero(bad)[0, 0]) - self.start
            raise AssertionError("%s: %d elements outside the logical [%d, %d] (ld %d) were written; first at row %d, column %d"
                                 % (what, int(bad.sum()), self.rows, self.cols, self.ld, math.floor(at / self.ld), at % self.ld))
        if tail_rows or tail_cols:
            badc = contract & (bits != expect)
            if bool(badc.any()):
                at = int(torch.nonzero(badc)[0, 0]) - self.start
                raise AssertionError("%s: %d elements of the documented tail differ from %#x; first at row %d, column %d"
                                     % (what, int(badc.sum()), expect, at // self.ld, at % self.ld))


def guarded(rows, cols, dtype, ld=None, offset=0, fill=None, device="cuda", init=None):
    """-> (view [rows, cols] with row stride ld, check).  The view sits ``offset`` elements (plus GUARD_ROWS rows) into one
    flat allocation with GUARD_ROWS full rows of guard before and after, all filled with the bit pattern ``fill``; ``init``
    (a tensor or a number) sets the logical elements, default NaN (an output)."""
    g = Guarded(rows, cols, dtype, ld, offset, fill, device, init)
    return g.view, g.check


def guarded_input(values, ld=None, offset=0, device="cuda"):
    """An operand: ``values`` [rows, cols] inside NaN bands and NaN pad columns."""
    return guarded(values.shape[0], values.shape[1], values.dtype, ld=ld, offset=offset, fill=NAN_FILL[values.dtype],
                   device=device, init=values.to(device))[0]


_PENDING = {}    # what -> worst ratio since the last report()


def assert_within(out, ref64, bound, what, verbose=True):
    """|out - ref| <= bound at EVERY element (float64, on the device of the reference; non-finite outputs fail).  Prints (or,
    with verbose=False, leaves to the next ``report``) and records the worst err / bound and where it is; returns it."""
    r = ref64.detach().to(torch.float64)
    o = out.detach().to(device=r.device, dtype=torch.float64)
    b = bound.detach().to(device=r.device, dtype=torch.float64) if torch.is_tensor(bound) else torch.full_like(r, float(bound))
    b = b.expand_as(r)
    assert o.shape == r.shape, (what, tuple(o.shape), tuple(r.shape))
    if r.numel() == 0:
        return 0.0
    err = (o - r).abs()
    err = torch.where(torch.isfinite(o), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    nan = torch.isnan(ratio).reshape(-1)
    flat = int(nan.int().argmax()) if bool(nan.any()) else int(ratio.argmax())
    worst = float(ratio.reshape(-1)[flat])
    if worst != worst:       # max() would drop a NaN that is not its first argument
        _PENDING[what] = worst
    else:
        _PENDING[what] = max(_PENDING.get(what, 0.0), worst)
    if verbose or not (worst <= 1):      # (a NaN ratio -- NaN in the reference or the bound, inf / inf -- fails too)
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        msg = "%-44s worst err/bound %.3f at %s (out %.6g ref %.6g bound %.3g)" % (
            what, worst, idx, float(o[idx]), float(r[idx]), float(b[idx]))
        print(msg)
        assert worst <= 1, "%s: %d of %d elements outside the bound" % (msg, int((~(ratio <= 1)).sum()), ratio.numel())
    return worst


def report(test):
    """Print the worst ratios recorded since the last report (one line per quantity) -- every test ends with it."""
    print()
    for what in sorted(_PENDING):
        print("RATIO %-40s %-34s %.3f" % (test, what, _PENDING[what]))
    _PENDING.clear()


# ------------------------------------------------------------------------------------------------------------- GEMM
GELU_ABS = 2.5e-4          # |gelu_f - gelu| where z < 1: asserted by tests/test_gelu_poly_cpu.py
GELU_REL = 1e-4            # |gelu_f - gelu| / |gelu| where z >= 1: asserted there too (Phi is a polynomial: its error of
                           # < 6e-5 is multiplied by z, so no absolute allowance can hold for large z)
DGELU_REL = 3e-4           # |dgelu_f - gelu'| (times |acc|): asserted by tests/test_gelu_poly_cpu.py
SIGMOID_ABS = TANH_ABS = 2.0 ** -12     # a REQUIREMENT on the device function: one eighth of a bf16 half-ulp at 1
LIP_GELU, LIP_SIGMOID = 1.13, 0.25      # max |gelu'| (1.129), max sigmoid'


def gemm_acc_bound(abs_prod, K, alpha=1.0, bias=None, bias2=None):
    """E = (K + 4) u (|alpha| (|A||B|)_ij + |bias_j| + |bias2_j|): error of z = alpha * acc + bias + bias2.

    A length-K f32 dot product of exact operand products, summed in ANY order (MFMA blocks, k-tiles, split-K atomics),
    is off by at most (K - 1) u (1 + O(Ku)) times the sum of the absolute products; the four extra u pay for the alpha
    multiply, the two bias adds and one fan-in add of the epilogue (each one rounding of a value no larger than the absolute
    sum they are charged on)."""
    t = abs(alpha) * abs_prod.double()
    if bias is not None:
        t = t + bias.double().abs()
    if bias2 is not None:
        t = t + bias2.double().abs()
    return (K + 4) * U_ACC * t


def gelu_prime64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def epilogue_bounds(epi, z, E, aux=None):
    """Error of the UNROUNDED epilogue value(s) given z (float64 reference of alpha*acc+bias+bias2) and its error E.
    -> (err_main, err_out2 or None).  epi is the name: NONE GELU DGELU ADD GATE TANH RELU ADD_RELU.

    f(z + e) - f(z) <= L |e| for an L-Lipschitz f, plus the approximation allowance of the device function:
      GELU   1.13 E + (2.5e-4 where z < 1, 1e-4 |gelu(z)| where z >= 1; the larger of the two where z is within E of 1)
             out2 = z: E
      DGELU  |gelu'(aux)| E + 3e-4 |z|   (aux is read exactly; the allowance is relative to the accumulator it multiplies)
      ADD / ADD_RELU / RELU / NONE  E    (max(., 0) is 1-Lipschitz; the add of aux is one of the four extra roundings of E,
                                          charged here on |aux| too: + u |aux|)
      GATE   g = sigmoid(z): E / 4 + 2^-12 = err_g (out2);  main = g * aux: |aux| err_g + u |g aux|
      TANH   E + 2^-12"""
    z = z.double()
    if epi == "GELU":
        rel = GELU_REL * (0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))).abs()
        allow = torch.where(z < 1 - E, torch.full_like(z, GELU_ABS), torch.where(z >= 1 + E, rel, rel.clamp_min(GELU_ABS)))
        return LIP_GELU * E + allow, E
    if epi == "DGELU":
        return gelu_prime64(aux).abs() * E + DGELU_REL * z.abs() + U_ACC * (z * gelu_prime64(aux)).abs(), None
    if epi in ("ADD", "ADD_RELU"):
        return E + U_ACC * aux.double().abs(), None
    if epi == "GATE":
        eg = LIP_SIGMOID * E + SIGMOID_ABS
        return aux.double().abs() * eg + U_ACC * (torch.sigmoid(z) * aux.double()).abs(), eg
    if epi == "TANH":
        return E + TANH_ABS, None
    if epi in ("NONE", "RELU"):
        return E, None
    raise ValueError(epi)


def epilogue_ref(epi, z, aux=None):
    """float64 reference of the epilogue -> (main, out2 or None)"""
    z = z.double()
    if epi == "GELU":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))), z
    if epi == "DGELU":
        return z * gelu_prime64(aux), None
    if epi == "ADD":
        return z + aux.double(), None
    if epi == "GATE":
        g = torch.sigmoid(z)
        return g * aux.double(), g
    if epi == "TANH":
        return torch.tanh(z), None
    if epi == "RELU":
        return z.clamp_min(0), None
    if epi == "ADD_RELU":
        return (z + aux.double()).clamp_min(0), None
    return z, None


TINY = {BF16: 2.0 ** -126, F32: 2.0 ** -126, F16: 2.0 ** -25}


def stored(err, ref, dtype):
    """A value with error ``err`` rounded to ``dtype``: err + eps_fmt (|ref| + err) + underflow.  Underflow: below the
    smallest normal number the relative roundoff no longer holds -- bf16 and f32 results may be flushed to zero (2^-126
    absolute), fp16 keeps subnormals with a spacing of 2^-24 (half of it)."""
    return err + EPS[dtype] * (ref.double().abs() + err) + TINY[dtype]


def with_beta(err, ref_new, beta, c_old):
    """C = new + beta * C_old evaluated in f32: |beta| |C_old| enters exactly (C_old is an input), the multiply-add costs one
    more rounding of each term: + u (|new| + |beta C_old|).  -> (reference, error) of the sum before it is stored."""
    t = beta * c_old.double()
    return ref_new.double() + t, err + U_ACC * (ref_new.double().abs() + t.abs())


# -------------------------------------------------------------------------------------------------------- attention
def attn_delta(q, k, scale, s, weight):
    """Delta_i = max over the keys that carry weight of ((64 + 2) u scale sum_d |q_id||k_kd| + 2^-22 |s_ik|).

    q [.., Sq, 64], k [.., Skv, 64] float64, s the float64 scores INCLUDING the additive mask, ``weight`` a bool [.., Sq, Skv]:
    keys whose float64 probability is not zero (a key at -10000 under a live one has none; in a fully masked sample every
    key has, and f32 scores near -10000 are then really that coarse).  First term: the 64-long f32 dot product (+2: scale multiply, mask add); second:
    the subtraction of the running maximum and the exp2 argument scaling, each one f32 rounding of a number no larger than
    |s| (2 u = 2^-22)."""
    ab = scale * (q.double().abs() @ k.double().abs().transpose(-1, -2))
    d = (64 + 2) * U_ACC * ab + 2.0 ** -22 * s.abs()
    d = torch.where(weight, d, torch.zeros_like(d))
    return d.amax(-1)


def attn_fwd_bound(p, v, delta, dtype=BF16):
    """(2^-7 + 4 Delta_i) sum_k p_ik |v_kj|.

    Scores off by at most Delta move every p_ik by a factor within exp(+-2 Delta) (numerator and normaliser each by
    exp(+-Delta)), i.e. 2 Delta (1 + Delta) relative; the second 2 Delta pays the exp2 / reciprocal device functions and the
    f32 row sums of the normaliser, which are relative errors of the same size class (a few u) and never exceed 2 Delta since
    Delta >= 66 u scale sum|q||k|.  P is rounded to bf16 before P.V (2^-8 of sum p|v|) and O is rounded to bf16 (2^-8 of |o| <=
    sum p|v|; an fp16 copy rounds finer); below the smallest normal of ``dtype`` the underflow term of ``stored`` applies.  ``p`` is the probability that
    multiplies v: with dropout, the kept and rescaled one."""
    return (2.0 ** -7 + 4.0 * delta[..., None]) * (p.double() @ v.double().abs()) + TINY[dtype]


def attn_lse_bound(lse, delta):
    """|lse error| <= 2 Delta_i + 2^-22 |lse|: a score error Delta moves log-sum-exp by at most Delta, the second Delta pays
    the log / exp2 device functions and the row sum; the result is max + log(sum), one f32 add and one rounding (2 u |lse|)."""
    return 2.0 * delta + 2.0 ** -22 * lse.double().abs()


# -------------------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd_bounds(t_abs, s, gamma, beta, eps, y_dtype=BF16):
    """Bounds of (y, xhat, rstd) for s = dropout(x + bias) + residual -> mean, centred two-pass variance, rstd, xhat, y.

    t_abs [M, H] = (|x| + |bias|) m + |residual|, the absolute terms of s (float64); s [M, H] float64.
      e_s    = 3 u t_abs                      (bias add, mask multiply, residual add)
      e_mean = (H + 4) u mean(t_abs)          (f32 sum of length H over the wave, then * 1/H)
      e_c    = e_s + e_mean + u |c|,  c = s - mean
      e_var  = (H + 4) u var + 2 mean(|c| e_c)          (f32 sum of squares; d(c^2) = 2 |c| e_c)
      r_rstd = e_var / (2 (var + eps)) + 2^-22          (relative; sqrt and the division are one rounding each: 2 u)
      e_xhat = rstd e_c + |xhat| (r_rstd + u)           (before rounding; stored in bf16)
      e_y    = |gamma| e_xhat + 2 u (|gamma xhat| + |beta|)   (before rounding; stored in y_dtype)
    An all-zero row has every term zero: y == beta exactly (after its rounding).

    Known limit: e_mean grows with H mean(t_abs), so for rows whose mean is large against their deviation the bound of y
    passes the bar of the existing test (1e-2 of the largest reference) as H grows: for f32 rows of mean 100 and deviation 1
    it is 0.84 of that bar at H = 520 (the case the GPU test runs) and 2.1 times the bar at H = 2048.  That is what an f32
    sum of H terms of size 100 can lose against a deviation of 1, not slack; for rows of mean 0 the bound stays under the
    bar at every H here (tests/test_kernel_check_cpu.py asserts both)."""
    H = s.shape[-1]
    s = s.double()
    mean = s.mean(-1, keepdim=True)
    c = s - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = c * rstd
    e_s = 3 * U_ACC * t_abs
    e_mean = (H + 4) * U_ACC * t_abs.mean(-1, keepdim=True)
    e_c = e_s + e_mean + U_ACC * c.abs()
    e_var = (H + 4) * U_ACC * var + 2 * (c.abs() * e_c).mean(-1, keepdim=True)
    r_rstd = e_var / (2 * (var + eps)) + 2.0 ** -22
    e_xhat = rstd * e_c + xhat.abs() * (r_rstd + U_ACC)
    g, b = gamma.double(), beta.double()
    y = g * xhat + b
    e_y = g.abs() * e_xhat + 2 * U_ACC * ((g * xhat).abs() + b.abs())
    return {"y": (y, stored(e_y, y, y_dtype)), "y_raw": (y, e_y), "xhat": (xhat, stored(e_xhat, xhat, BF16)),
            "rstd": (rstd[..., 0], rstd[..., 0] * (r_rstd[..., 0] + EPS[F32]))}


def ln_bwd_bounds(dy, xhat, rstd, gamma, mask=None):
    """References and bounds of the LayerNorm backward.  Its inputs are dy (the sum of the bf16 gradients fed in, float64),
    the SAVED xhat (bf16) and rstd (f32) and gamma -- all exact as given -- so nothing of the forward's error enters:

      gd   = gamma dy                                  one rounding each for the dy + dy2 add and the product: 2 u |gd|
      c1   = mean(gd), c2 = mean(gd xhat)              f32 sums of length H: (H + 4) u mean|gd|, (H + 4) u mean|gd xhat| (+ the
                                                       2 u of gd inside each term, covered by the + 4)
      ds   = rstd (gd - c1 - xhat c2)                  rstd (2 u |gd| + e_c1 + |xhat| e_c2) + 3 u rstd (|gd| + |c1| + |xhat c2|)
      dres = bf16(ds);  dx = bf16(ds * mask)           the mask multiplier 1 / (1 - p) costs one more rounding: u |dx|
      dgamma_j = sum_rows dy xhat, dbeta_j = sum_rows dy        f32 sums of length M in any order: (M + 4) u sum|.|
    (dbias is the column sum of the STORED dx: the test bounds it against the kernel's own dx with (M + 4) u sum|dx|.)"""
    M, H = dy.shape
    dy, xh, g = dy.double(), xhat.double(), gamma.double()
    r = rstd.double()[:, None]
    gd = g * dy
    c1 = gd.mean(-1, keepdim=True)
    c2 = (gd * xh).mean(-1, keepdim=True)
    e_c1 = (H + 4) * U_ACC * gd.abs().mean(-1, keepdim=True)
    e_c2 = (H + 4) * U_ACC * (gd * xh).abs().mean(-1, keepdim=True)
    ds = r * (gd - c1 - xh * c2)
    e_ds = r * (2 * U_ACC * gd.abs() + e_c1 + xh.abs() * e_c2) + 3 * U_ACC * r * (gd.abs() + c1.abs() + (xh * c2).abs())
    out = {"dres": (ds, stored(e_ds, ds, BF16)), "ds_raw": (ds, e_ds)}     # ds_raw: before any storage rounding
    m = torch.ones_like(ds) if mask is None else mask.double()
    dx = ds * m
    out["dx"] = (dx, stored(m * e_ds + U_ACC * dx.abs(), dx, BF16))
    dgam, dbet = (dy * xh).sum(0), dy.sum(0)
    out["dgamma"] = (dgam, stored((M + 4) * U_ACC * (dy * xh).abs().sum(0), dgam, F32))
    out["dbeta"] = (dbet, stored((M + 4) * U_ACC * dy.abs().sum(0), dbet, F32))
    return out


def attn_bwd_bounds(q, k, v, s, p, m, dout, lse, delta, scale):
    """References and bounds of (dq, dk, dv, delta) of one head batch; float64 tensors q / dout [.., Sq, 64], k / v
    [.., Skv, 64], s (scores incl. mask), p = softmax(s), m the dropout multiplier (0 or 1 / (1 - p_drop); ones without),
    lse the float64 log-sum-exp, delta = attn_delta(..).  What the kernels round (csrc/attention.hip): P and dS to bf16 as
    matrix operands; dP and dP - D stay f32 (that is where the cancellation is), and D is rowsum(P m dP) from the recomputed
    f32 P, not rowsum(dO O) of the rounded output.

      P   is recomputed as exp(s - lse) from f32 scores (error Delta_i) and the SAVED lse (error L_i = attn_lse_bound):
          relative error rho_i = expm1(Delta_i + L_i) + 2^-22 (exp2 and its argument scaling); where it is used as a bf16
          value: rho_op_i = rho_i + 2^-8 (1 + rho_i).
      dV  = (P m)^T dO: sum_i rho_op_i P m |dO| + (Sq + 4) u sum_i P m |dO|, stored in bf16.
      dP  = dO V^T: e_dP = (64 + 4) u sum_j |dO||V|.
      D   = rowsum(P m dP) -- the ``delta`` output: sum_k (rho_i P m |dP| + P m e_dP) + (Skv + 4) u sum_k P m |dP|, f32.
      dS  = bf16(P) (m dP - D): rho_op_i P (|m dP| + |D|) + P (m e_dP + e_D), then rounded to bf16 as matrix operand.
      dQ  = scale dS K: scale (e_dS |K| + (Skv + 4) u |dS| |K|);  dK = scale dS^T Q likewise with Sq; stored in bf16.

    Known limit: the bounds of dq / dk are no looser than the bar of the existing test (3e-2 of the largest reference) at plain
    scores only.  With q and k scaled by 4 the softmax is nearly one-hot, so dS = P (dP - D) is nearly zero and so are dq / dk
    and their largest element, while e_D keeps the term rho P |dP| with rho ~ 3 Delta_i from the score error Delta_i that
    the forward bound grants (Delta_i grows with scale sum|q||k|, 16 times larger there).  Measured against the bar, the dq / dk
    bounds are 1.2 - 2.6 times it at 130 x 257, 3 - 4 times at 65 x 129 and orders of magnitude at 5 x 7, where the reference
    itself is almost zero.  At 4x scores a shifted dropout mask is therefore certain to leave the bound only on dv; dv and
    the forward outputs stay sharp there (tests/test_kernel_check_cpu.py asserts what holds at each scale)."""
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    T = lambda x: x.transpose(-1, -2)
    Sq, Skv = q.shape[-2], k.shape[-2]
    pd = p * m
    L = attn_lse_bound(lse, delta)
    rho = (torch.expm1(delta + L) + 2.0 ** -22)[..., None]
    rho_op = rho + 2.0 ** -8 * (1 + rho)
    dv = T(pd) @ dout
    e_dv = T(rho_op * pd) @ dout.abs() + (Sq + 4) * U_ACC * (T(pd) @ dout.abs())
    dP = dout @ T(v)
    e_dP = (64 + 4) * U_ACC * (dout.abs() @ T(v.abs()))
    D = (pd * dP).sum(-1)
    e_D = ((rho * pd) * dP.abs() + pd * e_dP).sum(-1) + (Skv + 4) * U_ACC * (pd * dP.abs()).sum(-1)
    dS = p * (m * dP - D[..., None])
    e_dS = rho_op * p * ((m * dP).abs() + D.abs()[..., None]) + p * (m * e_dP + e_D[..., None])
    e_dS = e_dS + 2.0 ** -8 * (dS.abs() + e_dS)
    dq = scale * (dS @ k)
    e_dq = scale * (e_dS @ k.abs() + (Skv + 4) * U_ACC * (dS.abs() @ k.abs()))
    dk = scale * (T(dS) @ q)
    e_dk = scale * (T(e_dS) @ q.abs() + (Sq + 4) * U_ACC * (T(dS.abs()) @ q.abs()))
    return {"dq": (dq, stored(e_dq, dq, BF16)), "dk": (dk, stored(e_dk, dk, BF16)), "dv": (dv, stored(e_dv, dv, BF16)),
            "delta": (D, stored(e_D, D, F32))}
