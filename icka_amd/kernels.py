"""Tensor-level launchers over the C-ABI (include/icka_hip.h).

PyTorch is used here only for device memory and the current HIP stream: each function checks device / dtype /
contiguity on the host, then hands raw device pointers + sizes + the stream to libicka_hip.so.  Tensors must live
on a ROCm device; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_ADD, EPI_ADD_RELU, EPI_DGELU, EPI_GATE, EPI_GELU, EPI_NONE, EPI_RELU, EPI_TANH, GEMM_NN, GEMM_NT, GEMM_TN,
                   GemmDesc, check)

BF16 = torch.bfloat16
F32 = torch.float32
F16 = torch.float16


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_CUR_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of torch's current HIP stream.  (torch.cuda.current_stream().cuda_stream builds a Stream object per call:
    ~10 us of host time, i.e. ~2 ms of an eager c2 step's ~230 launches -- tools/eager_profile.py.)"""
    if _RAW_STREAM is not None and _CUR_DEVICE is not None:
        return _RAW_STREAM(_CUR_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise TypeError("%s must be a ROCm device tensor (icka_amd has no CPU path), got %s" % (name, t.device))


def _mat(t: torch.Tensor, name: str, dtype=BF16) -> None:
    # one-expression fast path (this runs ~700 times per eager c2 step); the slow path below words the error
    if t.is_cuda and t.dtype is dtype and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1):
        return
    _dev(t, name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s must be a 2-D row-major view (stride(1)==1), got shape %s strides %s"
                         % (name, tuple(t.shape), t.stride()))


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ld(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.stride(0)


# ------------------------------------------------------------------------------------------------------- GEMM
_PROF = None   # None, or the list of GEMM launches recorded while profile_gemm(True) is active


def profile_gemm(enable: bool, reps: int = 5):
    """bench.py roofline leg.  profile_gemm(True): start recording every GEMM launch (descriptor + operand tensors,
    kept alive).  profile_gemm(False): re-issue the recorded launches back to back, ``reps`` times, between ONE pair
    of HIP events on the launch stream (so no host gap or per-launch event cost is inside the bracket) and return
    (algorithmic FLOPs, elapsed ms, launches, algorithmic bytes) of what ran inside the bracket."""
    global _PROF
    if enable:
        _PROF = []
        return None
    rec, _PROF = _PROF or [], None
    lib = _lib.load()
    global last_fused_profile
    last_fused_profile = None
    if not rec:
        return 0.0, 0.0, 0, 0.0
    plain = [r for r in rec if r[0] < 2]
    fused = [r for r in rec if r[0] == 2]      # icka_gemm_ln launches: a GEMM with its LayerNorm phase in the same kernel
    fused_qa = [r for r in rec if r[0] == 3]   # icka_gemm_qkv_attn launches: the QKV projection with its attention in the same kernel

    def replay(which):
        for kind, payload, n, _keep in which:
            if kind == 0 and isinstance(n, torch.Tensor):
                check(lib.icka_gemm_live(C.byref(payload), n.data_ptr(), _stream()), "icka_gemm_live")
            elif kind == 0:
                check(lib.icka_gemm(C.byref(payload), _stream()), "icka_gemm")
            elif kind == 1:
                check(lib.icka_gemm_grouped(payload, n, _stream()), "icka_gemm_grouped")
            elif kind == 2:
                check(lib.icka_gemm_ln(*payload), "icka_gemm_ln")
            else:
                check(lib.icka_gemm_qkv_attn(*payload), "icka_gemm_qkv_attn")

    def timed(which):
        replay(which)   # warm
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            replay(which)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fl = lambda which: reps * sum(2.0 * d.M * d.N * d.K for _, _, _, ds in which for d in ds)
    if fused:
        # the fused launches are timed in a bracket of their own: their duration contains the HBM-bound LayerNorm phase, so they
        # are reported beside the MFMA-bound class, not inside it
        last_fused_profile = {"flops": fl(fused), "ms": timed(fused), "launches": reps * len(fused)}
    global last_fused_qkv_profile
    last_fused_qkv_profile = None
    if fused_qa:    # likewise: the launch contains the whole-head attention of its tiles (GEMM FLOPs only are counted)
        last_fused_qkv_profile = {"flops": fl(fused_qa), "ms": timed(fused_qa), "launches": reps * len(fused_qa)}
    ms = timed(plain) if plain else 0.0
    nbytes = reps * sum(_gemm_bytes(d) for _, _, _, ds in plain for d in ds)
    return fl(plain), ms, reps * len(plain), nbytes


last_fused_qkv_profile = None   # the same for the recorded icka_gemm_qkv_attn launches
last_fused_profile = None     # profile_gemm(False): {"flops", "ms", "launches"} of the recorded icka_gemm_ln launches, or None


def _gemm_bytes(d) -> float:
    """algorithmic HBM bytes of one GEMM: both operands once + the output once (bf16 in, bf16/f32 out)"""
    return 2.0 * (d.M * d.K + d.N * d.K) + d.M * d.N * (4.0 if d.c_is_f32 == 1 else 2.0) + (2.0 * d.M * d.N if d.C3 else 0.0)


def gemm_desc(op: int, A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
              epilogue: int = EPI_NONE, aux: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None,
              alpha: float = 1.0, beta: float = 0.0, A2: Optional[torch.Tensor] = None,
              B2: Optional[torch.Tensor] = None, bias2: Optional[torch.Tensor] = None,
              colsum_out: Optional[torch.Tensor] = None, colsum_accumulate: bool = False,
              out3: Optional[torch.Tensor] = None, out3_only: bool = False, tune: int = 0) -> GemmDesc:
    """Validate the operands and fill an ``icka_gemm_desc`` (the tensors must stay alive until it is launched).
    Operands are bf16, or -- op NT only, the "mixed16" forward GEMMs -- both fp16; ``out`` may then be fp16 too, with
    ``out3`` an optional bf16 copy of it.  With an f32 ``out``, ``out3`` is the data-parallel wire copy (bf16 of the final,
    beta-accumulated value) the weight-gradient GEMMs write for dp.GradReducer: op TN only.  ``tune``: per-call overrides of
    the launch heuristics (``gemm_tune(...)``; 0 = the library's choice) -- results do not depend on it."""
    odt = A.dtype if A.dtype == F16 else BF16     # operand dtype of this launch
    if odt == F16 and op != GEMM_NT:
        raise ValueError("fp16 operands: NT (forward) GEMMs only")
    _mat(A, "A", odt); _mat(B, "B", odt)
    if op == GEMM_NT:
        M, K = A.shape; N, Kb = B.shape
    elif op == GEMM_NN:
        M, K = A.shape; Kb, N = B.shape
    elif op == GEMM_TN:
        K, M = A.shape; Kb, N = B.shape
    else:
        raise ValueError("bad op")
    if K != Kb:
        raise ValueError("reduction mismatch: %s vs %s" % (tuple(A.shape), tuple(B.shape)))
    K1 = 0
    if A2 is not None or B2 is not None:
        if A2 is None or B2 is None:
            raise ValueError("A2 and B2 go together")
        _mat(A2, "A2", odt); _mat(B2, "B2", odt)
        K2 = A2.shape[0] if op == GEMM_TN else A2.shape[1]
        K1, K = K, K + K2
    _dev(out, "out")
    if out.dtype not in (BF16, F32, F16) or out.dim() != 2 or tuple(out.shape) != (M, N) or (N > 1 and out.stride(1) != 1):
        raise ValueError("out must be [%d,%d] bf16/f32/fp16 row-major, got %s %s" % (M, N, tuple(out.shape), out.dtype))
    if out.dtype == F16 and (beta != 0.0 or colsum_out is not None):
        raise ValueError("fp16 outputs are plain forward outputs (no accumulate, no fused column sums)")
    if out3 is not None:
        if out.dtype not in (F16, F32):
            raise ValueError("out3 is the bf16 copy of an fp16 main output, or the data-parallel wire copy of an f32 one")
        _mat(out3, "out3")
        if tuple(out3.shape) != (M, N):
            raise ValueError("out3 must be [%d,%d]" % (M, N))
        if out.dtype == F32 and op != GEMM_TN:
            raise ValueError("out3 beside an f32 output (the data-parallel wire copy) exists on weight-gradient (TN) GEMMs only")
    d = GemmDesc()
    d.op, d.M, d.N, d.K, d.K1 = op, M, N, K, K1
    d.A, d.lda, d.B, d.ldb = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0)
    if A2 is not None:       # (ctypes zero-initialises the struct: optional fields are only written when present)
        d.A2, d.lda2, d.B2, d.ldb2 = A2.data_ptr(), A2.stride(0), B2.data_ptr(), B2.stride(0)
    d.C, d.ldc, d.c_is_f32 = out.data_ptr(), out.stride(0), {BF16: 0, F32: 1, F16: 2}[out.dtype]
    if odt == F16:
        d.ab_f16 = 1
    if out3 is not None:
        d.C3, d.ldc3 = out3.data_ptr(), out3.stride(0)
    if out3_only:
        if not (out3 is not None and out.dtype == F32 and beta == 0.0 and epilogue == EPI_NONE):
            raise ValueError("out3_only: an f32 output with a wire copy, beta == 0, no epilogue")
        d.c3_only = 1
    if out2 is not None:
        _mat(out2, "out2")
        d.C2, d.ldc2 = out2.data_ptr(), out2.stride(0)
    if aux is not None:
        _mat(aux, "aux", F16 if aux.dtype == F16 else BF16)
        d.aux, d.ldaux = aux.data_ptr(), aux.stride(0)
        if aux.dtype == F16:
            d.aux_f16 = 1
    if bias is not None:
        if not bias.is_cuda or bias.dtype != F32 or bias.numel() != N or not bias.is_contiguous():
            _dev(bias, "bias")
            raise ValueError("bias must be contiguous f32 [N]")
        d.bias = bias.data_ptr()
    if bias2 is not None:
        if bias2.dtype != F32 or bias2.numel() != N or not bias2.is_contiguous() or not bias2.is_cuda:
            raise ValueError("bias2 must be contiguous device f32 [N]")
        d.bias2 = bias2.data_ptr()
    d.alpha, d.beta, d.epilogue = alpha, beta, epilogue
    if tune:
        d.tune = int(tune)
    if colsum_out is not None:
        if op != GEMM_TN or colsum_out.dtype != F32 or colsum_out.numel() != M or not colsum_out.is_contiguous():
            raise ValueError("colsum_out: contiguous f32 [M] with op TN")
        if M % 128 or N % 128 or K % 64:
            raise ValueError("fused column sums need the aligned fast path (M, N % 128 == 0, K % 64 == 0)")
        d.colsum_out, d.colsum_accumulate = colsum_out.data_ptr(), int(colsum_accumulate)
    if _PROF is not None:   # the recorded launch is re-issued later: its operands must outlive the step
        d._keep = (A, B, out, bias, aux, out2, A2, B2, bias2, colsum_out, out3)
    return d


def gemm_tune(*, ring: Optional[int] = None, tile_n: Optional[int] = None, wide_tiles: Optional[bool] = None,
              direct_epilogue: Optional[bool] = None, warp_specialized: Optional[int] = None, w3_grid: Optional[int] = None,
              big_tiles: Optional[int] = None, ablation: Optional[int] = None) -> int:
    """The ``icka_gemm_desc.tune`` word (include/icka_hip.h, ICKA_TUNE_*): per-call overrides of single launch heuristics, for
    tests of the alternative kernels and for probes.  There is no process-wide setter; the same fields can be given to a whole
    process through the ICKA_TUNE_GEMM_* environment (read once when the library loads)."""
    t = 0
    if ring is not None:
        if ring not in (2, 3, 4, 5):
            raise ValueError("ring: 2 .. 5")
        t |= ring
    if tile_n is not None:
        if tile_n not in (96, 128):
            raise ValueError("tile_n: 96 or 128")
        t |= (1 if tile_n == 96 else 2) << 4
    if wide_tiles is not None:
        t |= (2 if wide_tiles else 1) << 8
    if direct_epilogue is not None:
        t |= (2 if direct_epilogue else 1) << 12
    if warp_specialized is not None:
        if warp_specialized not in (0, 1, 2, 3):
            raise ValueError("warp_specialized: 0 .. 3")
        t |= (warp_specialized + 1) << 16
    if w3_grid is not None:
        if w3_grid not in (1, 2, 4, 8):
            raise ValueError("w3_grid: 1, 2, 4 or 8")
        t |= w3_grid << 20
    if big_tiles is not None:
        if big_tiles not in (0, 1, 2):
            raise ValueError("big_tiles: 0 .. 2")
        t |= (big_tiles + 1) << 24
    if ablation is not None:
        if ablation not in (1, 2, 3):
            raise ValueError("ablation: 1 .. 3 (diagnostic builds)")
        t |= ablation << 28
    return t


def gemm(op: int, A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, *, a_live: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """out[M,N] = epilogue(alpha * op(A,B) [+ op(A2,B2)] + bias) + beta*out.   op: GEMM_NT / GEMM_NN / GEMM_TN.
    ``a_live`` (op NN / NT): uint8 [M] row-liveness flags of A (icka_gemm_live): byte t may be 0 only if row t of A is all zero;
    the launches that have a LIVE instance then do not fetch the 8-row pieces of A without a live row.  Bitwise the plain call."""
    lib = _lib.load()
    d = gemm_desc(op, A, B, out, **kw)
    if a_live is not None:
        _dev(a_live, "a_live")
        if op not in (GEMM_NN, GEMM_NT):
            raise ValueError("gemm: a_live flags the rows of a row-major A (op NN or NT)")
        if a_live.dtype != torch.uint8 or not a_live.is_contiguous() or a_live.numel() != d.M:
            raise ValueError("gemm: a_live must be a contiguous uint8 [M] tensor")
    if _PROF is not None:   # (a live launch is recorded, and replayed, with its flags: same descriptor, same FLOPs)
        _PROF.append((0, d, a_live if a_live is not None else 1, [d]))
    if a_live is not None:
        check(lib.icka_gemm_live(C.byref(d), a_live.data_ptr(), _stream()), "icka_gemm_live")
    else:
        check(lib.icka_gemm(C.byref(d), _stream()), "icka_gemm")
    return out


def slab_reduction(partials: torch.Tensor, nslab: int, H: int, outs, accumulate: bool, slab_stride: int = 0,
                   offset: int = 0):
    """Descriptor of  outs[slot][c] (+)= sum_b partials[offset + b*slab_stride + slot*H + c]  (c < H); rides on a
    gemm_grouped launch (``reductions=``).  Default stride: the LayerNorm slab layout left by ln_bwd_slabs."""
    r = _lib.SlabReduction()
    if slab_stride == 0:
        slab_stride = _lib.load().icka_ln_slab_slots() * H
    r.partials, r.slab_stride, r.nslab, r.H = partials.data_ptr() + 4 * offset, slab_stride, nslab, H
    r.nslots, r.accumulate = len(outs), int(bool(accumulate))
    for i, o in enumerate(outs):
        _dev(o, "reduction output")
        if o.dtype != F32 or o.numel() != H or not o.is_contiguous():
            raise ValueError("reduction outputs must be contiguous f32 with %d elements" % H)
        r.out[i] = o.data_ptr()
    r._keep = (partials,) + tuple(outs)
    return r


def cls_head_fwd(seq, gated, W, bias, logits):
    """logits f32 [M,C] = [seq | gated] . W^T + bias (W [C, 2H]); seq, gated and W all bf16, or all fp16 (mixed16)."""
    dt = seq.dtype if seq.dtype == F16 else BF16
    _mat(seq, "seq", dt); _mat(gated, "gated", dt)
    M, H = seq.shape
    Cn = W.shape[0]
    if not (seq.is_contiguous() and gated.is_contiguous() and W.is_contiguous() and logits.is_contiguous()):
        raise ValueError("cls_head_fwd: contiguous operands")
    if W.dtype != dt or tuple(W.shape) != (Cn, 2 * H) or logits.dtype != F32 or tuple(logits.shape) != (M, Cn):
        raise ValueError("cls_head_fwd: W %s [C,2H], logits f32 [M,C]" % dt)
    if H % 8 or 2 * H // 8 > 256:
        raise ValueError("cls_head_fwd: H must be a multiple of 8 with 2H/8 <= 256 (H <= 1024), got H=%d" % H)
    lib = _lib.load()
    fn = lib.icka_cls_head_fwd_h if dt == F16 else lib.icka_cls_head_fwd
    check(fn(seq.data_ptr(), gated.data_ptr(), W.data_ptr(), _ptr(bias), logits.data_ptr(), M, H, Cn, _stream()),
          "icka_cls_head_fwd")
    return logits


def cls_head_bwd(dl, seq, gated, gate, cross, W, dseq, du, dcross, partials):
    """Returns the number of slabs written to ``partials`` (see icka_cls_head_bwd)."""
    M, H = seq.shape
    Cn = W.shape[0]
    for n, t in (("seq", seq), ("gated", gated), ("gate", gate), ("cross", cross), ("dseq", dseq), ("du", du),
                 ("dcross", dcross)):
        _mat(t, n)
        if not t.is_contiguous() or tuple(t.shape) != (M, H):
            raise ValueError("%s must be contiguous bf16 [M,H]" % n)
    _mat(dl, "dl")
    lib = _lib.load()
    check(lib.icka_cls_head_bwd(dl.data_ptr(), dl.stride(0), seq.data_ptr(), gated.data_ptr(), gate.data_ptr(),
                                cross.data_ptr(), W.data_ptr(), dseq.data_ptr(), du.data_ptr(), dcross.data_ptr(),
                                partials.data_ptr(), M, H, Cn, _stream()), "icka_cls_head_bwd")
    return lib.icka_cls_head_bwd_slabs(M)


def gemm_grouped(descs, reductions=None, k_live=None) -> None:
    """Launch several GEMMs (gemm_desc results) at once; same-layout fast-path problems share one launch.
    ``reductions``: slab_reduction descriptors (at most 4) summed by extra blocks of the same launch.
    ``k_live``: per problem None or a uint8 [K] tensor of row-liveness flags (icka_gemm_grouped_live): byte t may be 0 only
    if row t of one of the problem's operands is all zero; the 12-wave weight-gradient launch then skips dead k-tiles."""
    reductions = reductions or []
    if not descs and not reductions:
        return
    lib = _lib.load()
    arr = (GemmDesc * max(len(descs), 1))(*descs)
    if _PROF is not None and descs:
        _PROF.append((1, arr, len(descs), list(descs)))
    if k_live is not None and any(f is not None for f in k_live):
        if len(k_live) != len(descs) or len(reductions) > 4:
            raise ValueError("gemm_grouped: one k_live entry per problem, at most 4 reductions")
        for f, dsc in zip(k_live, descs):
            if f is not None and (f.dtype != torch.uint8 or not f.is_contiguous() or f.numel() != dsc.K):
                raise ValueError("gemm_grouped: k_live must be a contiguous uint8 [K] tensor")
        larr = (C.c_void_p * len(descs))(*[None if f is None else f.data_ptr() for f in k_live])
        rarr = (_lib.SlabReduction * max(len(reductions), 1))(*reductions)
        check(lib.icka_gemm_grouped_live(arr, len(descs), rarr if reductions else None, len(reductions), larr, _stream()),
              "icka_gemm_grouped_live")
        return
    if not reductions:
        check(lib.icka_gemm_grouped(arr, len(descs), _stream()), "icka_gemm_grouped")
        return
    for i in range(0, len(reductions), 4):   # the ABI takes 4 per call; GEMMs go with the first chunk
        chunk = reductions[i:i + 4]
        rarr = (_lib.SlabReduction * len(chunk))(*chunk)
        check(lib.icka_gemm_grouped_ex(arr if i == 0 else None, len(descs) if i == 0 else 0, rarr, len(chunk),
                                       _stream()), "icka_gemm_grouped_ex")


# ------------------------------------------------------------------------------------------------- LayerNorm
def _kind(t: torch.Tensor) -> int:
    """element-type code of the LayerNorm launchers: 0 bf16, 1 f32, 2 fp16"""
    return {BF16: 0, F32: 1, F16: 2}[t.dtype]


def ln_fwd(x, bias, residual, gamma, beta, y, *, y2=None, y_f32=None, y_f16=None, xhat=None, rstd=None, eps=1e-12,
           p_drop=0.0, seed=0):
    """x / residual may be bf16, f32 or fp16 [M,H] row-major; y (and y2) bf16; twin copy of the output: y_f32 (contiguous
    f32) or y_f16 (contiguous fp16, the "mixed16" forward operand + residual) -- at most one of the two."""
    lib = _lib.load()
    _mat(x, "x", x.dtype if x.dtype in (BF16, F32, F16) else BF16); _mat(y, "y")
    if residual is not None:
        _mat(residual, "residual", residual.dtype if residual.dtype in (BF16, F32, F16) else BF16)
    if y_f32 is not None and y_f16 is not None:
        raise ValueError("one twin copy: y_f32 or y_f16")
    M, H = x.shape
    twin = y_f16 if y_f16 is not None else y_f32
    if twin is not None and (twin.dtype != (F16 if y_f16 is not None else F32) or not twin.is_contiguous()
                             or tuple(twin.shape) != (M, H)):
        raise ValueError("twin output must be contiguous [M,H] f32 (y_f32) / fp16 (y_f16)")
    fn = lib.icka_ln_fwd_h if y_f16 is not None else lib.icka_ln_fwd
    check(fn(x.data_ptr(), x.stride(0), _kind(x), _ptr(bias), _ptr(residual), _ld(residual),
             0 if residual is None else _kind(residual), gamma.data_ptr(), beta.data_ptr(),
             y.data_ptr(), y.stride(0), _ptr(y2), _ld(y2), _ptr(twin), _ptr(xhat), _ptr(rstd),
             M, H, eps, p_drop, seed, _stream()), "icka_ln_fwd")
    return y


class GemmLnHandoffError(RuntimeError):
    """A stripe wait of a fused dense + LayerNorm launch gave up: the rows it finished are NaN."""


_GEMM_LN_ERR = None      # one pinned (host-mapped) error word for the process: polled by the host without a device sync
_GEMM_LN_ERR_NP = None   # numpy view of it (a host read through it costs ~0.1 us: it sits in front of every fused launch)
_GEMM_LN_ERR_PTR = 0


def _gemm_ln_err_word() -> int:
    """Device-visible address of the pinned error word (allocated on first use: never under stream capture -- a model's first
    forward, and every capture's warm-up, run eagerly)."""
    global _GEMM_LN_ERR, _GEMM_LN_ERR_NP, _GEMM_LN_ERR_PTR
    if _GEMM_LN_ERR is None:
        _GEMM_LN_ERR = torch.zeros(16, dtype=torch.int32).pin_memory()
        _GEMM_LN_ERR_NP = _GEMM_LN_ERR.numpy()
        _GEMM_LN_ERR_PTR = _GEMM_LN_ERR.data_ptr()
    return _GEMM_LN_ERR_PTR


def gemm_ln_sync(device) -> torch.Tensor:
    """Zeroed counter words for ``gemm_ln`` (icka_gemm_ln_sync_words; the launches leave them zero: one buffer per stream)."""
    return torch.zeros(_lib.load().icka_gemm_ln_sync_words(), dtype=torch.int32, device=device)


def gemm_ln(h, w, o, bias, residual, gamma, beta, y, sync, *, y_f32=None, y_f16=None, xhat=None, rstd=None, eps=1e-12,
            p_drop=0.0, seed=0) -> bool:
    """dense (h @ w^T -> o, f32) + bias + dropout + residual + LayerNorm -> y (and twin / xhat / rstd) as ONE launch
    (icka_gemm_ln) -- bitwise ``gemm(NT, h, w, o)`` followed by ``ln_fwd(o, bias, residual, gamma, beta, y, ...)``.  Returns False
    (nothing launched) when the shape is not eligible: the caller then makes the two calls.  A stripe wait of an EARLIER fused
    launch that gave up is raised here (gemm_ln_check_error: a host read of a pinned word)."""
    gemm_ln_check_error("detected before the next fused launch")
    lib = _lib.load()
    d = gemm_desc(GEMM_NT, h, w, o)
    _mat(y, "y")
    if residual is not None:
        _mat(residual, "residual", residual.dtype if residual.dtype in (BF16, F32, F16) else BF16)
    twin = y_f16 if y_f16 is not None else y_f32
    M, N = o.shape
    if twin is not None and (twin.dtype != (F16 if y_f16 is not None else F32) or not twin.is_contiguous() or tuple(twin.shape) != (M, N)):
        raise ValueError("twin output must be contiguous [M,N] f32 (y_f32) / fp16 (y_f16)")
    args = (d, _ptr(bias), _ptr(residual), _ld(residual), 0 if residual is None else _kind(residual), gamma.data_ptr(),
            beta.data_ptr(), y.data_ptr(), y.stride(0), _ptr(twin), int(y_f16 is not None), _ptr(xhat), _ptr(rstd), eps,
            p_drop, seed, sync.data_ptr(), _gemm_ln_err_word(), _stream())
    rc = lib.icka_gemm_ln(*args)
    if rc == -1:        # ICKA_E_SHAPE: not a shape of the fused kernel
        return False
    check(rc, "icka_gemm_ln")
    if _PROF is not None:   # bench.py roofline leg: the launch is re-issued later, its operands must outlive the step
        d._keep = (h, w, o, bias, residual, gamma, beta, y, twin, xhat, rstd, sync)
        _PROF.append((2, args, 1, [d]))
    return True


def gemm_qkv_attn(x, w, bias, qkv, add_mask, ctx, lse, B, heads, S, *, p_drop=0.0, seed=0, scale=None, out16=None,
                  keepbits=None) -> bool:
    """QKV projection (x @ w^T + bias -> qkv, the stacked bf16 [q | k | v]; x / w bf16 or both fp16) and the whole-head
    self-attention of every (sample, head) as ONE launch (icka_gemm_qkv_attn) -- bitwise ``gemm(NT, x, w, qkv, bias=bias)``
    followed by ``attn_fwd`` on the three column blocks (``out16`` / ``keepbits`` as there).  Returns False (nothing launched)
    when the shape is not eligible: the caller then makes the two calls."""
    lib = _lib.load()
    d = gemm_desc(GEMM_NT, x, w, qkv, bias=bias)
    _mat(ctx, "ctx")
    H = heads * 64
    if tuple(qkv.shape) != (B * S, 3 * H) or tuple(ctx.shape) != (B * S, H):
        return False
    if add_mask.dtype != F32 or not add_mask.is_contiguous() or add_mask.numel() != B * S:
        raise ValueError("add_mask must be contiguous f32 [B, S]")
    if lse is not None and (lse.dtype != F32 or not lse.is_contiguous() or lse.numel() != B * heads * S):
        raise ValueError("lse must be contiguous f32 [B, heads, S]")
    if out16 is not None:
        _mat(out16, "out16", F16)
        if tuple(out16.shape) != tuple(ctx.shape) or out16.stride(0) != ctx.stride(0):
            raise ValueError("out16 must have the shape and row stride of ctx")
    if keepbits is not None and (not keepbits.is_cuda or keepbits.element_size() != 4 or not keepbits.is_contiguous()
                                 or keepbits.numel() < lib.icka_attn_keepbits_words(B, heads, S, S)):
        raise ValueError("keepbits: contiguous 32-bit device buffer of icka_attn_keepbits_words words (attn_keepbits)")
    args = (d, add_mask.data_ptr(), ctx.data_ptr(), _ptr(out16), ctx.stride(0), _ptr(lse), B, heads, S,
            (1.0 / 8.0) if scale is None else scale, p_drop, seed, _ptr(keepbits), _stream())
    rc = lib.icka_gemm_qkv_attn(*args)
    if rc == -1:        # ICKA_E_SHAPE
        return False
    check(rc, "icka_gemm_qkv_attn")
    if _PROF is not None:
        d._keep = (x, w, bias, qkv, add_mask, ctx, lse, out16, keepbits)
        _PROF.append((3, args, 1, [d]))
    return True


def gemm_ln_check_error(where: str = "") -> None:
    """Raise if a fused dense + LayerNorm launch ever reported a stripe wait that gave up.  The word is pinned host memory the
    kernel writes with a system-scope store: the check is a plain host read, no device synchronisation, so it runs at every host
    touch-point (the next fused launch, GraphedStep / GraphedModule replays).  The word is cleared when the error is raised."""
    if _GEMM_LN_ERR_NP is not None and _GEMM_LN_ERR_NP[0] != 0:
        _GEMM_LN_ERR_NP[0] = 0
        raise GemmLnHandoffError(
            "icka_amd fused dense + LayerNorm%s: a block gave up waiting for the other blocks of its 128-row stripe -- the grid "
            "was not co-resident (another kernel held CUs: a collective on another stream, a second model, a partitioned GPU).  "
            "The rows it finished are NaN.  Reserve CUs (icka_lstm_set_reserved_cus) or set ICKA_FUSE_DENSE_LN=0."
            % ((" (" + where + ")") if where else ""))


def ln_bwd_slabs(dy, xhat, rstd, gamma, partials, *, dy2=None, dres=None, dx=None, p_drop=0.0, seed=0) -> int:
    """LayerNorm backward without the parameter-gradient finalize; returns the number of slabs left in ``partials``
    (slot 0 -> dgamma, slot 1 -> dbeta) for a slab_reduction."""
    lib = _lib.load()
    _mat(dy, "dy"); _mat(xhat, "xhat")
    M, H = dy.shape
    check(lib.icka_ln_bwd_slabs(dy.data_ptr(), dy.stride(0), _ptr(dy2), _ld(dy2), xhat.data_ptr(), rstd.data_ptr(),
                                gamma.data_ptr(), _ptr(dres), _ld(dres), _ptr(dx), _ld(dx), partials.data_ptr(), M, H,
                                p_drop, seed, _stream()), "icka_ln_bwd_slabs")
    return lib.icka_ln_bwd_nslab(M)


def ln_bwd_slabs_live(dy, xhat, rstd, gamma, partials, row_live, *, row_live_kv=None, add_mask=None, dy2=None, dres=None,
                      dx=None, p_drop=0.0, seed=0) -> int:
    """ln_bwd_slabs that also writes the row-liveness bytes (uint8 [M]) of the gradient rows it produced: ``row_live`` (some
    element of dres is non-zero) and optionally ``row_live_kv`` (... or the row is a key the additive mask f32 [B,S] leaves
    open): the k_live flags of the weight gradients downstream (gemm_grouped)."""
    lib = _lib.load()
    _mat(dy, "dy"); _mat(xhat, "xhat")
    M, H = dy.shape
    for f in (row_live, row_live_kv):
        if f is not None and (f.dtype != torch.uint8 or not f.is_contiguous() or f.numel() != M):
            raise ValueError("ln_bwd_slabs_live: the flags are contiguous uint8 [M] tensors")
    S = 0
    if row_live_kv is not None:
        if add_mask is None or add_mask.dtype != F32 or not add_mask.is_contiguous() or add_mask.numel() != M:
            raise ValueError("ln_bwd_slabs_live: row_live_kv needs the contiguous f32 additive mask [B,S] with B*S == M")
        S = add_mask.shape[-1]
    check(lib.icka_ln_bwd_slabs_live(dy.data_ptr(), dy.stride(0), _ptr(dy2), _ld(dy2), xhat.data_ptr(), rstd.data_ptr(),
                                     gamma.data_ptr(), _ptr(dres), _ld(dres), _ptr(dx), _ld(dx), partials.data_ptr(),
                                     row_live.data_ptr(), _ptr(row_live_kv), _ptr(add_mask) if S else None, S, M, H,
                                     p_drop, seed, _stream()), "icka_ln_bwd_slabs_live")
    return lib.icka_ln_bwd_nslab(M)


def ln_bwd_workspace(H: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().icka_ln_bwd_workspace_floats(H), dtype=F32, device=device)


def ln_bwd(dy, xhat, rstd, gamma, *, dy2=None, dres=None, dx=None, dgamma=None, dbeta=None, dbias=None,
           partials=None, p_drop=0.0, seed=0, accumulate=True):
    lib = _lib.load()
    _mat(dy, "dy"); _mat(xhat, "xhat")
    M, H = dy.shape
    check(lib.icka_ln_bwd(dy.data_ptr(), dy.stride(0), _ptr(dy2), _ld(dy2), xhat.data_ptr(), rstd.data_ptr(),
                          gamma.data_ptr(), _ptr(dres), _ld(dres), _ptr(dx), _ld(dx), _ptr(dgamma), _ptr(dbeta),
                          _ptr(dbias), partials.data_ptr(), M, H, p_drop, seed, int(accumulate), _stream()),
          "icka_ln_bwd")


# ------------------------------------------------------------------------------------------------- embeddings
def embed_fwd(ids, token_type, word, pos, typ, gamma, beta, y, *, y_f32=None, y_f16=None, xhat=None, rstd=None, eps=1e-12,
              p_drop=0.0, seed=0):
    lib = _lib.load()
    _dev(ids, "ids")
    B, S = ids.shape
    H = word.shape[1]
    if y_f32 is not None and y_f16 is not None:
        raise ValueError("one twin copy: y_f32 or y_f16")
    twin = y_f16 if y_f16 is not None else y_f32
    if twin is not None and (twin.dtype != (F16 if y_f16 is not None else F32) or not twin.is_contiguous()):
        raise ValueError("twin output must be contiguous f32 (y_f32) / fp16 (y_f16)")
    fn = lib.icka_embed_fwd_h if y_f16 is not None else lib.icka_embed_fwd
    check(fn(ids.data_ptr(), _ptr(token_type), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
             gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(twin), _ptr(xhat), _ptr(rstd),
             B, S, H, word.shape[0], typ.shape[0], eps, p_drop, seed, _stream()), "icka_embed_fwd")
    return y


def embed_bwd(dy, ids, token_type, xhat, rstd, gamma, dword, dpos, dtype_, dgamma, dbeta, partials, *,
              padding_idx=0, p_drop=0.0, seed=0, accumulate=True):
    lib = _lib.load()
    B, S = ids.shape
    H = dword.shape[1]
    check(lib.icka_embed_bwd(dy.data_ptr(), ids.data_ptr(), _ptr(token_type), xhat.data_ptr(), rstd.data_ptr(),
                             gamma.data_ptr(), dword.data_ptr(), dpos.data_ptr(), dtype_.data_ptr(),
                             dgamma.data_ptr(), dbeta.data_ptr(), partials.data_ptr(), B, S, H, dword.shape[0],
                             dtype_.shape[0], padding_idx, p_drop, seed, int(accumulate), _stream()),
          "icka_embed_bwd")


def embed_bwd_rows(dy, ids, token_type, xhat, rstd, gamma, dtok, dpos, dtype_, dgamma, dbeta, partials, *, vocab,
                   padding_idx=0, p_drop=0.0, seed=0, accumulate=True):
    """embed_bwd with the word-table gradient left as per-token rows ``dtok`` f32 [B*S, H] (row-sparse data-parallel exchange)."""
    lib = _lib.load()
    B, S = ids.shape
    H = dtok.shape[1]
    if dtok.dtype != F32 or tuple(dtok.shape) != (B * S, H) or not dtok.is_contiguous():
        raise ValueError("dtok must be contiguous f32 [B*S, H]")
    check(lib.icka_embed_bwd_rows(dy.data_ptr(), ids.data_ptr(), _ptr(token_type), xhat.data_ptr(), rstd.data_ptr(),
                                  gamma.data_ptr(), dtok.data_ptr(), dpos.data_ptr(), dtype_.data_ptr(), dgamma.data_ptr(),
                                  dbeta.data_ptr(), partials.data_ptr(), B, S, H, int(vocab), dtype_.shape[0], padding_idx, p_drop,
                                  seed, int(accumulate), _stream()), "icka_embed_bwd_rows")


def embed_scatter_rows(rows, ids, dword, *, padding_idx=0, scale=1.0):
    """dword[ids[t]] += scale * rows[t]  (rows f32 or bf16 [T, H] contiguous, ids int64 [T], dword f32 [vocab, H])."""
    _dev(rows, "rows"); _dev(ids, "ids"); _dev(dword, "dword")
    if rows.dtype not in (F32, BF16) or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows must be contiguous f32 / bf16 [T, H]")
    if ids.dtype != torch.int64 or ids.numel() != rows.shape[0] or not ids.is_contiguous():
        raise ValueError("ids must be contiguous int64 with one entry per row")
    if dword.dtype != F32 or dword.dim() != 2 or dword.shape[1] != rows.shape[1] or not dword.is_contiguous():
        raise ValueError("dword must be contiguous f32 [vocab, H]")
    check(_lib.load().icka_embed_scatter_rows(rows.data_ptr(), int(rows.dtype == BF16), ids.data_ptr(), dword.data_ptr(),
                                              rows.shape[0], rows.shape[1], dword.shape[0], padding_idx, float(scale), _stream()),
          "icka_embed_scatter_rows")


# ------------------------------------------------------------------------------------------ adversarial training
ADV_MAX_H, ADV_MAX_S = 2048, 1024           # limits of icka_adv_ascend / icka_adv_init_uniform (icka_hip.h)


def embed_fwd_adv(ids, token_type, word, pos, typ, gamma, beta, delta, y, *, y_f32=None, y_f16=None, xhat=None, rstd=None,
                  eps=1e-12, p_drop=0.0, seed=0):
    """embed_fwd with the perturbation ``delta`` (f32 [B, S, H] / [B*S, H] contiguous, or None: embed_fwd itself) added to the
    word rows (icka_hip.h: icka_embed_fwd_adv / _h)."""
    lib = _lib.load()
    _dev(ids, "ids")
    B, S = ids.shape
    H = word.shape[1]
    if y_f32 is not None and y_f16 is not None:
        raise ValueError("one twin copy: y_f32 or y_f16")
    twin = y_f16 if y_f16 is not None else y_f32
    if twin is not None and (twin.dtype != (F16 if y_f16 is not None else F32) or not twin.is_contiguous()):
        raise ValueError("twin output must be contiguous f32 (y_f32) / fp16 (y_f16)")
    if delta is not None:
        _dev(delta, "delta")
        if delta.dtype != F32 or delta.numel() != B * S * H or not delta.is_contiguous():
            raise ValueError("delta must be contiguous f32 [B, S, H]")
    fn = lib.icka_embed_fwd_adv_h if y_f16 is not None else lib.icka_embed_fwd_adv
    check(fn(ids.data_ptr(), _ptr(token_type), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
             gamma.data_ptr(), beta.data_ptr(), _ptr(delta), y.data_ptr(), _ptr(twin), _ptr(xhat), _ptr(rstd),
             B, S, H, word.shape[0], typ.shape[0], eps, p_drop, seed, _stream()), "icka_embed_fwd_adv")
    return y


def _adv_operands(delta, input_mask):
    _dev(delta, "delta"); _dev(input_mask, "input_mask")
    if delta.dtype != F32 or delta.dim() != 3 or not delta.is_contiguous():
        raise ValueError("delta must be contiguous f32 [B, S, H]")
    B, S, H = delta.shape
    if input_mask.dtype != torch.int64 or tuple(input_mask.shape) != (B, S) or not input_mask.is_contiguous():
        raise ValueError("input_mask must be contiguous int64 [B, S] = %s, got %s %s" % ((B, S), input_mask.dtype, tuple(input_mask.shape)))
    return B, S, H


def adv_workspace_floats(B: int, S: int, H: int) -> int:
    return int(_lib.load().icka_adv_workspace_floats(B, S, H))


def adv_ascend(delta, grad, input_mask, norms, workspace, *, alpha, epsilon):
    """One ascent step in place on ``delta`` (icka_hip.h: icka_adv_ascend): delta, grad f32 [B, S, H], input_mask int64 [B, S],
    norms f32 [B, 2], workspace f32 with adv_workspace_floats(B, S, H) elements."""
    B, S, H = _adv_operands(delta, input_mask)
    _dev(grad, "grad"); _dev(norms, "norms"); _dev(workspace, "workspace")
    if grad.dtype != F32 or grad.numel() != delta.numel() or not grad.is_contiguous():
        raise ValueError("grad must be contiguous f32 with the elements of delta")
    if norms.dtype != F32 or tuple(norms.shape) != (B, 2) or not norms.is_contiguous():
        raise ValueError("norms must be contiguous f32 [B, 2]")
    need = adv_workspace_floats(B, S, H)
    if need <= 0:
        raise ValueError("icka_adv_ascend takes H %% 8 == 0, H <= %d, S <= %d; got S = %d, H = %d" % (ADV_MAX_H, ADV_MAX_S, S, H))
    if workspace.dtype != F32 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError("workspace must be contiguous f32 with at least %d elements" % need)
    check(_lib.load().icka_adv_ascend(delta.data_ptr(), grad.data_ptr(), input_mask.data_ptr(), norms.data_ptr(), B, S, H,
                                      float(alpha), float(epsilon), workspace.data_ptr(), _stream()), "icka_adv_ascend")
    return delta


def adv_init_uniform(delta, input_mask, *, epsilon, seed, counter=None):
    """The uniform start of FreeLB (icka_hip.h: icka_adv_init_uniform); ``counter``: device int64 [1] added to ``seed``, or None."""
    B, S, H = _adv_operands(delta, input_mask)
    if counter is not None:
        _dev(counter, "counter")
        if counter.dtype != torch.int64 or counter.numel() != 1:
            raise ValueError("counter must be one device int64")
    check(_lib.load().icka_adv_init_uniform(delta.data_ptr(), input_mask.data_ptr(), B, S, H, float(epsilon),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(counter), _stream()), "icka_adv_init_uniform")
    return delta


def adv_bump(counter):
    """counter[0] += 1 as a one-thread launch (a graph node: every replay of a captured step draws a fresh uniform start)."""
    _dev(counter, "counter")
    if counter.dtype != torch.int64 or counter.numel() != 1:
        raise ValueError("counter must be one device int64")
    check(_lib.load().icka_adv_bump(counter.data_ptr(), _stream()), "icka_adv_bump")


def embed_prompt_fwd(ids, src, prompt, word, pos, typ, gamma, beta, y, *, y_f32=None, xhat=None, rstd=None,
                     pos_offset=0, eps=1e-5, p_drop=0.0, seed=0):
    """Prompt-spliced embeddings + LayerNorm + dropout (icka_hip.h: icka_embed_prompt_fwd).  ids int64 [B,S_in],
    src int32 [S], prompt bf16 [B,P,H] contiguous, y bf16 [B*S,H]."""
    lib = _lib.load()
    _dev(ids, "ids"); _dev(src, "src"); _dev(prompt, "prompt")
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.dim() != 2:
        raise ValueError("ids must be contiguous int64 [B,S_in]")
    if src.dtype != torch.int32 or src.dim() != 1 or not src.is_contiguous():
        raise ValueError("src must be contiguous int32 [S]")
    B, S_in = ids.shape
    S, H = src.shape[0], word.shape[1]
    if prompt.dtype != BF16 or prompt.dim() != 3 or prompt.shape[0] != B or prompt.shape[2] != H or not prompt.is_contiguous():
        raise ValueError("prompt must be contiguous bf16 [B,P,H]")
    if pos.shape[0] < S + pos_offset:
        raise ValueError("position table has %d rows, the spliced sequence needs %d" % (pos.shape[0], S + pos_offset))
    if tuple(y.shape) != (B * S, H):
        raise ValueError("y must be [B*S,H]")
    check(lib.icka_embed_prompt_fwd(ids.data_ptr(), src.data_ptr(), prompt.data_ptr(), word.data_ptr(), pos.data_ptr(),
                                    typ.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(y_f32),
                                    _ptr(xhat), _ptr(rstd), B, S_in, S, prompt.shape[1], H, word.shape[0], pos_offset,
                                    eps, p_drop, seed, _stream()), "icka_embed_prompt_fwd")
    return y


def embed_prompt_bwd(dy, ids, src, xhat, rstd, gamma, dword, dpos, dtype_, dgamma, dbeta, dprompt, partials, *,
                     pos_offset=0, padding_idx=1, p_drop=0.0, seed=0, accumulate=True):
    lib = _lib.load()
    B, S_in = ids.shape
    S, H = src.shape[0], dword.shape[1]
    if dprompt.dtype != BF16 or not dprompt.is_contiguous() or dprompt.shape[0] != B or dprompt.shape[2] != H:
        raise ValueError("dprompt must be contiguous bf16 [B,P,H]")
    if partials.numel() < S * lib.icka_ln_slab_slots() * H:
        raise ValueError("partials too small")
    check(lib.icka_embed_prompt_bwd(dy.data_ptr(), ids.data_ptr(), src.data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
                                    gamma.data_ptr(), dword.data_ptr(), dpos.data_ptr(), dtype_.data_ptr(),
                                    dgamma.data_ptr(), dbeta.data_ptr(), dprompt.data_ptr(), partials.data_ptr(), B,
                                    S_in, S, dprompt.shape[1], H, dword.shape[0], pos_offset, padding_idx, p_drop, seed,
                                    int(accumulate), _stream()), "icka_embed_prompt_bwd")


def tanh_bwd(dy, y, dx):
    """dx = dy * (1 - y^2), contiguous bf16."""
    for n, t in (("dy", dy), ("y", y), ("dx", dx)):
        _dev(t, n)
        if t.dtype != BF16 or not t.is_contiguous():
            raise ValueError("%s must be contiguous bf16" % n)
    if dy.numel() != y.numel() or dx.numel() != y.numel():
        raise ValueError("tanh_bwd: size mismatch")
    check(_lib.load().icka_tanh_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.numel(), _stream()), "icka_tanh_bwd")
    return dx


def dgelu(dg, z, dz):
    """dz = dg * gelu'(z), contiguous bf16."""
    for n, t in (("dg", dg), ("z", z), ("dz", dz)):
        _dev(t, n)
        if t.dtype != BF16 or not t.is_contiguous() or t.numel() != z.numel():
            raise ValueError("%s must be contiguous bf16 with %d elements" % (n, z.numel()))
    check(_lib.load().icka_dgelu_bf16(dg.data_ptr(), z.data_ptr(), dz.data_ptr(), z.numel(), _stream()), "icka_dgelu_bf16")
    return dz


# ------------------------------------------------------------------------------------------------- attention
def attn_keepbits(B, heads, Sq, Skv, device) -> torch.Tensor:
    """Buffer for the keep bits of an attention-probability dropout site (attn_fwd fills it, attn_bwd reads it)."""
    return torch.empty(_lib.load().icka_attn_keepbits_words(B, heads, Sq, Skv), dtype=torch.int32, device=device)


def attn_fwd(q, k, v, add_mask, out, lse, B, heads, Sq, Skv, *, p_drop=0.0, seed=0, scale=None, fp8=False, out16=None,
             keepbits=None, tiled=False):
    """q/k/v/out: 2-D row-major bf16 views [B*S, >=heads*64] (may be column slices of a fused projection).
    fp8=True: QK^T and PV on the fp8 matrix cores (Sq, Skv <= 128 only).  out16: optional fp16 copy of the context with
    the strides of ``out`` (the "mixed16" operand of the out-proj GEMM).  tiled=True takes the tiled flash-style kernels
    also where the head would fit the whole-head kernels (per call: tests exercise both paths)."""
    lib = _lib.load()
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _mat(t, n)
    if scale is None:
        scale = 1.0 / math.sqrt(64.0)
    if out16 is not None or keepbits is not None or tiled:
        if out16 is not None:
            _mat(out16, "out16", F16)
            if tuple(out16.shape) != tuple(out.shape) or out16.stride(0) != out.stride(0):
                raise ValueError("out16 must have the shape and row stride of out")
        if keepbits is not None and (not keepbits.is_cuda or keepbits.element_size() != 4 or not keepbits.is_contiguous()
                                     or keepbits.numel() < lib.icka_attn_keepbits_words(B, heads, Sq, Skv)):
            raise ValueError("keepbits: contiguous 32-bit device buffer of icka_attn_keepbits_words words (attn_keepbits)")
        check(lib.icka_attn_fwd_ex(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                   add_mask.data_ptr(), out.data_ptr(), _ptr(out16), out.stride(0), _ptr(lse), B, heads,
                                   Sq, Skv, scale, p_drop, seed, (_lib.ATTN_FP8 if fp8 else 0) | (_lib.ATTN_TILED if tiled else 0),
                                   _ptr(keepbits), _stream()), "icka_attn_fwd_ex")
        return out
    fn = lib.icka_attn_fwd_fp8 if fp8 else lib.icka_attn_fwd
    check(fn(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), add_mask.data_ptr(),
             out.data_ptr(), out.stride(0), _ptr(lse), B, heads, Sq, Skv, scale, p_drop, seed, _stream()),
          "icka_attn_fwd_fp8" if fp8 else "icka_attn_fwd")
    return out


def attn_bwd(q, k, v, add_mask, out, dout, lse, delta, dq, dk, dv, B, heads, Sq, Skv, *, p_drop=0.0, seed=0,
             scale=None, keepbits=None, tiled=False):
    lib = _lib.load()
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out), ("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        _mat(t, n)
    if scale is None:
        scale = 1.0 / math.sqrt(64.0)
    check(lib.icka_attn_bwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                            add_mask.data_ptr(), out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0),
                            lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dq.stride(0), dk.data_ptr(),
                            dk.stride(0), dv.data_ptr(), dv.stride(0), B, heads, Sq, Skv, scale, p_drop, seed,
                            _ptr(keepbits), _lib.ATTN_TILED if tiled else 0, _stream()), "icka_attn_bwd")


ATTN_PROBS_MAX_KEYS = 512   # icka_attn_probs keeps every score of a query row in registers: BERT's position limit


def attn_probs(q, k, add_mask, B, heads, Sq, Skv, *, head_mean=False, scale=None, out=None) -> torch.Tensor:
    """Attention maps (icka_attn_probs): softmax(scale * q.k^T + add_mask) BEFORE dropout, f32 [B,heads,Sq,Skv] or, with
    ``head_mean``, the mean over heads [B,Sq,Skv].  q / k: the 2-D row-major bf16 views attn_fwd takes ([>= B*Sq, >= heads*64]
    and [>= B*Skv, >= heads*64], head size 64), add_mask: contiguous f32 [B,Skv].  ``out``: a contiguous f32 device tensor
    of exactly that many elements to write into (else a new one).  One launch; 1 <= Skv <= 512."""
    for n, t in (("q", q), ("k", k)):
        _mat(t, n)
    for n, v in (("B", B), ("heads", heads), ("Sq", Sq), ("Skv", Skv)):
        if int(v) != v or v < 1:
            raise ValueError("%s must be a positive integer, got %r" % (n, v))
    if Skv > ATTN_PROBS_MAX_KEYS:
        raise ValueError("attn_probs holds a query's scores in registers: Skv <= %d, got %d" % (ATTN_PROBS_MAX_KEYS, Skv))
    for n, t, rows in (("q", q, B * Sq), ("k", k, B * Skv)):
        if t.shape[0] < rows or t.shape[1] < heads * 64:
            raise ValueError("%s must hold at least %d rows and heads * 64 = %d columns, got %s" % (n, rows, heads * 64, tuple(t.shape)))
    _dev(add_mask, "add_mask")
    if add_mask.dtype != F32 or not add_mask.is_contiguous() or add_mask.numel() != B * Skv:
        raise ValueError("add_mask must be contiguous f32 [B, Skv] = [%d, %d]" % (B, Skv))
    shape = (B, Sq, Skv) if head_mean else (B, heads, Sq, Skv)
    if out is None:
        out = torch.empty(shape, dtype=F32, device=q.device)
    else:
        _dev(out, "out")
        if out.dtype != F32 or not out.is_contiguous() or out.numel() != math.prod(shape):
            raise ValueError("out must be a contiguous f32 tensor of %d elements" % math.prod(shape))
    if not (q.device == k.device == add_mask.device == out.device):
        raise ValueError("attn_probs: q, k, add_mask and out must live on one device")
    check(_lib.load().icka_attn_probs(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), add_mask.data_ptr(), out.data_ptr(),
                                      B, heads, Sq, Skv, (1.0 / 8.0) if scale is None else scale,
                                      _lib.ATTN_PROBS_HEAD_MEAN if head_mean else 0, _stream()), "icka_attn_probs")
    return out


# ------------------------------------------------------------------------------------------------- packed batches
def _i32vec(t: torch.Tensor, n: int, name: str) -> None:
    _dev(t, name)
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError("%s must be a contiguous int32 device tensor of at least %d elements" % (name, n))


def pack_plan(mask: torch.Tensor, max_tokens: int, plan, err_word: int = 0) -> None:
    """icka_pack_plan: input_mask (int64 [B,S]) -> the row maps of ``plan`` (packing.Plan: lens, cu, p2p, pad2pack, cls_of,
    status).  ``err_word``: address of a host-mapped uint32[2] that receives {tokens, flags} on overflow (0: none)."""
    _dev(mask, "mask")
    if mask.dtype != torch.int64 or mask.dim() != 2 or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous int64 [B, S] tensor")
    B, S = mask.shape
    _i32vec(plan.lens, B, "lens")
    _i32vec(plan.cu, B + 1, "cu_seqlens")
    _i32vec(plan.p2p, max_tokens, "packed_to_padded")
    _i32vec(plan.pad2pack, B * S, "padded_to_packed")
    _i32vec(plan.cls_of, max_tokens, "cls_of")
    if plan.status is not None:
        _i32vec(plan.status, 2, "status")
    check(_lib.load().icka_pack_plan(mask.data_ptr(), B, S, max_tokens, plan.lens.data_ptr(), plan.cu.data_ptr(),
                                     plan.p2p.data_ptr(), plan.pad2pack.data_ptr(), plan.cls_of.data_ptr(), _ptr(plan.status),
                                     err_word or None, _stream()), "icka_pack_plan")


def rows_gather(src: torch.Tensor, dst: torch.Tensor, row_map: torch.Tensor, map_stride: int = 1, fill: int = 0) -> torch.Tensor:
    """dst[r] = src[row_map[r * map_stride]] (-1: zeros, -2: every 32-bit word = ``fill``).  src / dst: 2-D row-major views of
    one dtype whose rows are whole 32-bit words (bf16 with an even width, f32)."""
    _dev(src, "src")
    _dev(dst, "dst")
    if src.dtype != dst.dtype or src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1]:
        raise ValueError("rows_gather: src and dst must be 2-D of one dtype and width")
    es = src.element_size()
    if (src.shape[1] * es) % 4 or src.stride(1) != 1 or dst.stride(1) != 1 or (src.stride(0) * es) % 4 or (dst.stride(0) * es) % 4:
        raise ValueError("rows_gather: rows must be whole 32-bit words of a row-major view")
    _dev(row_map, "row_map")
    if row_map.dtype != torch.int32 or not row_map.is_contiguous() or row_map.numel() < (dst.shape[0] - 1) * map_stride + 1:
        raise ValueError("rows_gather: row_map must be a contiguous int32 tensor covering every destination row")
    words = src.shape[1] * es // 4
    ld_s = src.stride(0) * es // 4
    ld_d = dst.stride(0) * es // 4
    check(_lib.load().icka_rows_gather(src.data_ptr(), ld_s, src.shape[0], dst.data_ptr(), ld_d, dst.shape[0], words,
                                       row_map.data_ptr(), map_stride, fill, _stream()), "icka_rows_gather")
    return dst


def _f32vec(t, n: int, name: str) -> None:
    if t is None:
        return
    _dev(t, name)
    if t.dtype != F32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError("%s must be a contiguous f32 device tensor of at least %d elements" % (name, n))


def _packed_checks(B, heads, Sq, Skv, M, kv_packed, add_mask, cu, **mats) -> None:
    """Row counts and widths of the operands of the packed attention calls: the query-side matrices (and the key-side ones when
    ``kv_packed``) hold at least Mrows rows, the key-side ones of a cross-attention at least B * Skv; every one at least
    heads * 64 columns; add_mask is contiguous f32 [B, Skv]."""
    _i32vec(cu, B + 1, "cu_seqlens")
    if not (0 < Sq <= 128 and 0 < Skv <= 128) or (kv_packed and Skv != Sq) or M <= 0:
        raise ValueError("packed attention: Sq, Skv in [1, 128] (equal for self-attention) and at least one packed row")
    _dev(add_mask, "add_mask")
    if add_mask.dtype != F32 or not add_mask.is_contiguous() or add_mask.numel() != B * Skv:
        raise ValueError("add_mask must be contiguous f32 [B, Skv] = [%d, %d]" % (B, Skv))
    for n, t in mats.items():
        key_side = n in ("k", "v", "dk", "dv")
        rows = B * Skv if (key_side and not kv_packed) else M
        if t.shape[0] < rows:
            raise ValueError("%s must hold at least %d rows, got %d" % (n, rows, t.shape[0]))
        if t.shape[1] < heads * 64:
            raise ValueError("%s must hold at least heads * 64 = %d columns, got %d" % (n, heads * 64, t.shape[1]))


def attn_fwd_packed(q, k, v, add_mask, out, lse, cu, kv_packed: bool, B, heads, Sq, Skv, *, p_drop=0.0, seed=0, scale=None,
                    keepbits=None):
    """attn_fwd for packed queries (icka_attn_fwd_packed): q / out rows are the packed rows [cu[b], cu[b+1]) of sample b; k / v
    too when ``kv_packed`` (self-attention), else at b * Skv.  Sq / Skv are the PADDED lengths (<= 128)."""
    lib = _lib.load()
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _mat(t, n)
    M = out.shape[0]        # Mrows: the kernel clamps cu_seqlens to it and reads / writes packed rows below it only
    _packed_checks(B, heads, Sq, Skv, M, kv_packed, add_mask, cu, q=q, out=out, k=k, v=v)
    _f32vec(lse, B * heads * Sq, "lse")
    if keepbits is not None and (not keepbits.is_cuda or keepbits.element_size() != 4 or not keepbits.is_contiguous()
                                 or keepbits.numel() < lib.icka_attn_keepbits_words(B, heads, Sq, Skv)):
        raise ValueError("keepbits: contiguous 32-bit device buffer of icka_attn_keepbits_words words (attn_keepbits)")
    check(lib.icka_attn_fwd_packed(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                   add_mask.data_ptr(), out.data_ptr(), out.stride(0), _ptr(lse), cu.data_ptr(), int(kv_packed),
                                   out.shape[0], B, heads, Sq, Skv, (1.0 / 8.0) if scale is None else scale, p_drop, seed,
                                   _ptr(keepbits), _stream()), "icka_attn_fwd_packed")
    return out


def attn_bwd_packed(q, k, v, add_mask, dout, lse, delta, dq, dk, dv, cu, kv_packed: bool, B, heads, Sq, Skv, *, p_drop=0.0,
                    seed=0, scale=None, keepbits=None):
    lib = _lib.load()
    for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        _mat(t, n)
    M = dq.shape[0]         # Mrows (see attn_fwd_packed)
    _packed_checks(B, heads, Sq, Skv, M, kv_packed, add_mask, cu, q=q, dout=dout, dq=dq, k=k, v=v, dk=dk, dv=dv)
    _f32vec(lse, B * heads * Sq, "lse")
    _f32vec(delta, B * heads * Sq, "delta")
    if keepbits is not None and (not keepbits.is_cuda or keepbits.element_size() != 4 or not keepbits.is_contiguous()
                                 or keepbits.numel() < lib.icka_attn_keepbits_words(B, heads, Sq, Skv)):
        raise ValueError("keepbits: contiguous 32-bit device buffer of icka_attn_keepbits_words words (attn_keepbits)")
    check(lib.icka_attn_bwd_packed(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                   add_mask.data_ptr(), dout.data_ptr(), dout.stride(0), lse.data_ptr(), delta.data_ptr(),
                                   dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0),
                                   cu.data_ptr(), int(kv_packed), dq.shape[0], B, heads, Sq, Skv,
                                   (1.0 / 8.0) if scale is None else scale, p_drop, seed, _ptr(keepbits), _stream()),
          "icka_attn_bwd_packed")


# ------------------------------------------------------------------------------------------------- LSTM
def _lstm_lens(lens, B, like):
    """``lens`` of the variable-length LSTM entries: int32 [B], contiguous, on the device of the other operands."""
    _dev(lens, "lens")
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or not lens.is_contiguous() or lens.device != like.device:
        raise ValueError("lens must be a contiguous int32 [B] tensor on %s" % like.device)
    return lens.data_ptr()


def lstm_fwd(gates_x, w_hh, y, c_all, act, hprev, B, S, H, flags=0, lens=None):
    """gates_x f32 [B*S, 8H]; w_hh bf16 [8H, H] (= [2][4H][H]); y bf16 [B*S, 2H]; c_all f32 [B*S, 2H];
    act bf16 [B*S, 8H]; hprev bf16 [B*S, 2H] or None.  ``lens`` (int32 [B] on the device): positions t >= lens[b] are pads
    (icka_hip.h: icka_lstm_fwd_varlen); None is the fixed-length entry."""
    _dev(gates_x, "gates_x")
    if gates_x.dtype != F32 or gates_x.stride(1) != 1 or tuple(gates_x.shape) != (B * S, 8 * H):
        raise ValueError("gates_x must be f32 [B*S, 8H]")
    for n, t, shp, dt in (("w_hh", w_hh, (8 * H, H), BF16), ("y", y, (B * S, 2 * H), BF16),
                          ("c_all", c_all, (B * S, 2 * H), F32), ("act", act, (B * S, 8 * H), BF16)):
        _dev(t, n)
        if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError("%s must be contiguous %s %s" % (n, dt, shp))
    if lens is not None:
        check(_lib.load().icka_lstm_fwd_varlen(gates_x.data_ptr(), gates_x.stride(0), w_hh.data_ptr(), y.data_ptr(),
                                               c_all.data_ptr(), act.data_ptr(), _ptr(hprev), _lstm_lens(lens, B, gates_x),
                                               B, S, H, int(flags), _stream()), "icka_lstm_fwd_varlen")
        return
    check(_lib.load().icka_lstm_fwd(gates_x.data_ptr(), gates_x.stride(0), w_hh.data_ptr(), y.data_ptr(),
                                    c_all.data_ptr(), act.data_ptr(), _ptr(hprev), B, S, H, int(flags), _stream()), "icka_lstm_fwd")


def lstm_mask_gates(gates_x, lens, B, S, H):
    """In place: the i and f pre-activations of both directions of an f32 gate buffer [B*S, 8H] := -1e4 at every t >= lens[b]
    (icka_hip.h: icka_lstm_mask_gates; the fp32 mode's form of the pad mask)."""
    _dev(gates_x, "gates_x")
    if gates_x.dtype != F32 or gates_x.stride(1) != 1 or tuple(gates_x.shape) != (B * S, 8 * H):
        raise ValueError("gates_x must be f32 [B*S, 8H]")
    check(_lib.load().icka_lstm_mask_gates(gates_x.data_ptr(), gates_x.stride(0), _lstm_lens(lens, B, gates_x), B, S, H,
                                           _stream()), "icka_lstm_mask_gates")
    return gates_x


def lstm_bwd(dy, w_hh_t, act, c_all, dgates, dc_carry, B, S, H, flags=0, lens=None):
    for n, t, shp, dt in (("dy", dy, (B * S, 2 * H), BF16), ("w_hh_t", w_hh_t, (2 * H, 4 * H), BF16),
                          ("act", act, (B * S, 8 * H), BF16), ("c_all", c_all, (B * S, 2 * H), F32),
                          ("dgates", dgates, (B * S, 8 * H), BF16), ("dc_carry", dc_carry, (2 * B, H), F32)):
        _dev(t, n)
        if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError("%s must be contiguous %s %s" % (n, dt, shp))
    if lens is not None:
        check(_lib.load().icka_lstm_bwd_varlen(dy.data_ptr(), w_hh_t.data_ptr(), act.data_ptr(), c_all.data_ptr(),
                                               dgates.data_ptr(), dgates.stride(0), dc_carry.data_ptr(),
                                               _lstm_lens(lens, B, dy), B, S, H, int(flags), _stream()), "icka_lstm_bwd_varlen")
        return
    check(_lib.load().icka_lstm_bwd(dy.data_ptr(), w_hh_t.data_ptr(), act.data_ptr(), c_all.data_ptr(),
                                    dgates.data_ptr(), dgates.stride(0), dc_carry.data_ptr(), B, S, H, int(flags), _stream()),
          "icka_lstm_bwd")


class LstmHandoffError(RuntimeError):
    """A hand-off wait of a persistent LSTM launch gave up: the outputs of that call are NaN-poisoned."""


def lstm_check_error(where: str = "") -> None:
    """Raise if a persistent LSTM launch ever reported a failed hand-off (icka_hip.h: icka_lstm_barrier_error).  The error
    word is host-mapped memory: the check is a plain host read, no device synchronisation, so it runs at every host
    touch-point (BiLSTM.forward, GraphedStep / SegmentedStep replays).  The word is cleared when the error is raised."""
    lib = _lib.load()
    rc = lib.icka_lstm_barrier_error()
    if rc != 0:
        lib.icka_lstm_clear_error()
        raise LstmHandoffError(
            "icka_amd BiLSTM%s: a block of a persistent LSTM launch gave up waiting for another block's words (status %d): "
            "the grid was not co-resident (another kernel held its CUs, e.g. a collective on the communication stream, or "
            "the GPU is partitioned / shared).  The outputs and gradients of that call are NaN.  Reserve CUs "
            "(icka_lstm_set_reserved_cus) or take the per-step launches (BiLSTM.recurrence_flags = LSTM_PER_STEP)."
            % ((" (" + where + ")") if where else "", rc))


def copy_many(srcs, dsts) -> None:
    """dsts[i] <- srcs[i] (contiguous device tensors of equal byte size, at most 8) in one launch."""
    import ctypes as C
    n = len(srcs)
    if n != len(dsts) or n > 8:
        raise ValueError("copy_many: up to 8 (source, destination) pairs")
    sp = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dp = (C.c_void_p * n)(*[t.data_ptr() for t in dsts])
    for a, b in zip(srcs, dsts):
        if a.numel() * a.element_size() != b.numel() * b.element_size() or not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("copy_many: contiguous tensors of equal byte size")
    nb = (C.c_int64 * n)(*[t.numel() * t.element_size() for t in srcs])
    check(_lib.load().icka_copy_many(sp, dp, nb, n, _stream()), "icka_copy_many")


_LSTM_RESERVED = [0]


def lstm_set_reserved_cus(n: int) -> int:
    """Set the CUs kept free of persistent BiLSTM blocks (process-global); returns the previous value so that the caller can
    restore it (dp.GradReducer.close)."""
    check(_lib.load().icka_lstm_set_reserved_cus(int(n)), "icka_lstm_set_reserved_cus")
    prev, _LSTM_RESERVED[0] = _LSTM_RESERVED[0], int(n)
    return prev


def linear_small_m(x, W, bias, y, act: int = 0):
    """y bf16 [M<=64, N] = act(x . W^T + bias); x may be a strided row view (the pooler's first-token rows)."""
    _mat(x, "x"); _mat(W, "W"); _mat(y, "y")
    M, Kd = x.shape
    N = W.shape[0]
    if W.shape[1] != Kd or tuple(y.shape) != (M, N) or not W.is_contiguous():
        raise ValueError("linear_small_m: W [N,K] contiguous, y [M,N]")
    check(_lib.load().icka_linear_small_m(x.data_ptr(), x.stride(0), W.data_ptr(), _ptr(bias), y.data_ptr(), y.stride(0),
                                          M, N, Kd, act, _stream()), "icka_linear_small_m")
    return y


def transpose_bf16(src, dst, batch, R, Cn):
    _dev(src, "src"); _dev(dst, "dst")
    if src.dtype != BF16 or dst.dtype != BF16 or src.numel() != batch * R * Cn or dst.numel() != src.numel() \
            or not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("transpose_bf16: contiguous bf16 [batch, R, C] -> [batch, C, R]")
    check(_lib.load().icka_transpose_bf16(src.data_ptr(), dst.data_ptr(), batch, R, Cn, _stream()), "icka_transpose_bf16")
    return dst


# ------------------------------------------------------------------------------------------------- CRF
def _crf_check(emissions, start, end, trans):
    for n, t in (("emissions", emissions), ("start", start), ("end", end), ("trans", trans)):
        _dev(t, n)
        if t.dtype != F32 or not t.is_contiguous():
            raise ValueError("%s must be contiguous f32" % n)
    if emissions.dim() != 3:
        raise ValueError("emissions must be [B,S,C]")
    B, S, Cn = emissions.shape
    if start.numel() != Cn or end.numel() != Cn or tuple(trans.shape) != (Cn, Cn):
        raise ValueError("transition parameters do not match num_tags = %d" % Cn)
    return B, S, Cn


def _i64(t, name, shape):
    if t is None:
        return None
    _dev(t, name)
    if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError("%s must be contiguous int64 %s" % (name, shape))
    return t


def crf_llh(emissions, tags, mask, start, end, trans, llh):
    B, S, Cn = _crf_check(emissions, start, end, trans)
    _i64(tags, "tags", (B, S)); _i64(mask, "mask", (B, S))
    check(_lib.load().icka_crf_llh(emissions.data_ptr(), Cn, tags.data_ptr(), _ptr(mask), start.data_ptr(),
                                   end.data_ptr(), trans.data_ptr(), llh.data_ptr(), B, S, Cn, _stream()),
          "icka_crf_llh")
    return llh


def crf_grad(emissions, tags, mask, start, end, trans, gllh, d_emissions, d_start, d_end, d_trans):
    B, S, Cn = _crf_check(emissions, start, end, trans)
    _i64(tags, "tags", (B, S)); _i64(mask, "mask", (B, S))
    check(_lib.load().icka_crf_grad(emissions.data_ptr(), Cn, tags.data_ptr(), _ptr(mask), start.data_ptr(),
                                    end.data_ptr(), trans.data_ptr(), gllh.data_ptr(), d_emissions.data_ptr(), Cn,
                                    d_start.data_ptr(), d_end.data_ptr(), d_trans.data_ptr(), B, S, Cn, _stream()),
          "icka_crf_grad")


def crf_decode(emissions, mask, start, end, trans, best_tags, best_score=None):
    B, S, Cn = _crf_check(emissions, start, end, trans)
    _i64(mask, "mask", (B, S)); _i64(best_tags, "best_tags", (B, S))
    check(_lib.load().icka_crf_decode(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(),
                                      trans.data_ptr(), best_tags.data_ptr(), _ptr(best_score), B, S, Cn, _stream()),
          "icka_crf_decode")
    return best_tags


CRF_FLAT_MAX_B = 2048   # icka_crf_score_decode: the batch size up to which the kernel computes the path offsets itself


def crf_score_decode(emissions, tags, mask, start, end, trans, llh, lens, tags_flat):
    """Viterbi paths of all samples into ``tags_flat`` (int32, back to back) with their lengths in ``lens`` (int32 [B]) and,
    when ``tags`` is given, the gold-path log-likelihood into ``llh`` (f32 [B]) -- one launch, no host sync."""
    B, S, Cn = _crf_check(emissions, start, end, trans)
    _i64(tags, "tags", (B, S)); _i64(mask, "mask", (B, S))
    check_flat_tags(lens, tags_flat, B, S)
    if (tags is None) != (llh is None):
        raise ValueError("crf_score_decode: tags and llh go together")
    if llh is not None:
        _dev(llh, "llh")
        if llh.dtype != F32 or tuple(llh.shape) != (B,) or not llh.is_contiguous():
            raise ValueError("llh must be contiguous f32 [%d]" % B)
    _dev(lens, "lens"); _dev(tags_flat, "tags_flat")
    if B > CRF_FLAT_MAX_B:
        raise ValueError("crf_score_decode: B = %d > %d" % (B, CRF_FLAT_MAX_B))
    check(_lib.load().icka_crf_score_decode(emissions.data_ptr(), Cn, _ptr(tags), _ptr(mask), start.data_ptr(),
                                            end.data_ptr(), trans.data_ptr(), _ptr(llh), lens.data_ptr(),
                                            tags_flat.data_ptr(), tags_flat.numel(), B, S, Cn, _stream()),
          "icka_crf_score_decode")


def check_flat_tags(lens, tags_flat, B, S):
    """Host-side checks of the outputs of crf_score_decode (no device access): int32, 1-D, contiguous, ``lens`` [B] and room
    for B * S tags."""
    for n, t in (("lens", lens), ("tags_flat", tags_flat)):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous 1-D int32 tensor, got %s %s" % (n, t.dtype, tuple(t.shape)))
    if lens.numel() != B:
        raise ValueError("lens holds %d entries for a batch of %d" % (lens.numel(), B))
    if tags_flat.numel() < B * S:
        raise ValueError("tags_flat holds %d tags, a batch of %d x %d needs up to %d" % (tags_flat.numel(), B, S, B * S))


CRF_MAX_SC, CRF_POSTERIOR_MAX_S, CRF_POSTERIOR_MAX_IDS = 12288, 512, 64
CRF_NBEST_MAX_C, CRF_NBEST_MAX_K, CRF_NBEST_MAX_S, CRF_NBEST_MAX_SCK = 16, 8, 512, 49152


class _CrfOperands(object):
    """The host-side checks of crf_posterior, crf_nbest and the crf_constrained_* entries, in the one order they all keep: the
    four f32 parameters, ``emissions`` [B,S,C] and the transition shapes (the constructor); then the entry's own limits and its
    operands (``vec`` / ``opt``) in the order the entry states them; the devices last (``same_device``).  ValueError for dtype /
    shape / contiguity / a limit, then TypeError for an operand that is not on the device, before anything is launched."""

    def __init__(self, who, emissions, start, end, trans):
        for n, t in (("emissions", emissions), ("start", start), ("end", end), ("trans", trans)):
            if not isinstance(t, torch.Tensor) or t.dtype != F32 or not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous f32" % (who, n))
        if emissions.dim() != 3:
            raise ValueError("%s: emissions must be [B,S,C], got %s" % (who, tuple(emissions.shape)))
        Cn = emissions.shape[2]
        if start.numel() != Cn or end.numel() != Cn or tuple(trans.shape) != (Cn, Cn):
            raise ValueError("%s: transition parameters do not match num_tags = %d" % (who, Cn))
        self.who, self.shape, self.used = who, tuple(emissions.shape), [emissions, start, end, trans]

    def vec(self, t, name, dtype, shape=None, least=None, fits=None, what=None):
        """``t`` must be a contiguous ``dtype`` tensor of exactly ``shape``, or of at least ``least[0]`` rows of the trailing
        shape ``least[1:]``, or one that ``fits(t)``, worded by ``what``; it joins the operands of the device check."""
        ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()
        if ok and shape is not None:
            ok = tuple(t.shape) == shape
        if ok and least is not None:
            ok = t.dim() == len(least) and t.shape[0] >= least[0] and tuple(t.shape[1:]) == tuple(least[1:])
        if ok and fits is not None:
            ok = fits(t)
        if not ok:
            if what is None:
                want = shape if shape is not None else (">= %d" % least[0],) + tuple(least[1:])
                what = "a contiguous %s tensor of shape %s" % (dtype, want)
            raise ValueError("%s: %s must be %s, got %s %s"
                             % (self.who, name, what, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))
        self.used.append(t)
        return t

    def opt(self, t, *args, **kw):
        """``vec`` of an operand that may be None."""
        return None if t is None else self.vec(t, *args, **kw)

    def same_device(self):
        dev = self.used[0].device
        for t in self.used:
            _dev(t, "%s operand" % self.who)
            if t.device != dev:
                raise ValueError("%s: operands on %s and %s" % (self.who, dev, t.device))


def crf_posterior(emissions, mask, start, end, trans, log_z, bad, *, lens=None, tags_flat=None, seq_logp=None,
                  token_conf=None, marginals=None, label_table=None, ent=None, ent_conf=None, n_ent=None):
    """log Z, token marginals and -- for the paths ``lens`` + ``tags_flat`` (a ``crf.DeviceTags``) -- the path's
    log-probability, the marginal of every path tag and, with a ``label_table``, the path's chunks with their posteriors
    (icka_crf_posterior, include/icka_hip.h): one launch, no host sync.  ``bad`` (int32 [1]) is ADDED to: zero it first.
    Every operand is checked on the host (dtype, shape, contiguity, the kernel's limits: ValueError; then the device:
    TypeError) before anything is launched."""
    ops = _CrfOperands("crf_posterior", emissions, start, end, trans)
    B, S, Cn = ops.shape
    if B < 1 or S < 1 or not 1 <= Cn <= 64 or S * Cn > CRF_MAX_SC or B > CRF_FLAT_MAX_B:
        raise ValueError("crf_posterior: B <= %d, C <= 64 and S * C <= %d, got [%d, %d, %d]"
                         % (CRF_FLAT_MAX_B, CRF_MAX_SC, B, S, Cn))
    ops.vec(log_z, "log_z", F32, (B,))
    ops.vec(bad, "bad", torch.int32, (1,))
    ops.opt(mask, "mask", torch.int64, (B, S))
    ops.opt(marginals, "marginals", F32, (B, S, Cn))
    if (lens is None) != (tags_flat is None):
        raise ValueError("crf_posterior: lens and tags_flat go together")
    cap, L_ids = 0, 0
    if lens is not None:
        ops.vec(lens, "lens", torch.int32, (B,))
        cap = ops.vec(tags_flat, "tags_flat", torch.int32, least=(0,)).numel()
        ops.vec(seq_logp, "seq_logp", F32, (B,))
        ops.vec(token_conf, "token_conf", F32, least=(cap,))
    elif seq_logp is not None or token_conf is not None or label_table is not None:
        raise ValueError("crf_posterior: seq_logp, token_conf and label_table need the paths (lens + tags_flat)")
    if label_table is not None:
        L_ids = ops.vec(label_table, "label_table", torch.int32, least=(1,)).numel()
        if L_ids > CRF_POSTERIOR_MAX_IDS or S > CRF_POSTERIOR_MAX_S:
            raise ValueError("crf_posterior: with a label table at most %d words and S <= %d, got %d words, S = %d"
                             % (CRF_POSTERIOR_MAX_IDS, CRF_POSTERIOR_MAX_S, L_ids, S))
        ops.vec(ent, "ent", torch.int32, least=(cap, 3))
        ops.vec(ent_conf, "ent_conf", F32, least=(cap,))
        ops.vec(n_ent, "n_ent", torch.int32, (B,))
    elif ent is not None or ent_conf is not None or n_ent is not None:
        raise ValueError("crf_posterior: ent, ent_conf and n_ent need a label_table")
    ops.same_device()
    check(_lib.load().icka_crf_posterior(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(),
                                         trans.data_ptr(), _ptr(lens), _ptr(tags_flat), cap, _ptr(label_table), L_ids,
                                         log_z.data_ptr(), _ptr(seq_logp), _ptr(token_conf), _ptr(marginals), _ptr(ent),
                                         _ptr(ent_conf), _ptr(n_ent), bad.data_ptr(), B, S, Cn, _stream()),
          "icka_crf_posterior")


def crf_nbest(emissions, mask, start, end, trans, nbest, lens, n_paths, scores, tags_flat):
    """The ``nbest`` best tag paths of every sample (icka_crf_nbest, include/icka_hip.h): ``lens`` and ``n_paths`` int32 [B],
    ``scores`` f32 [B, nbest], ``tags_flat`` int32 [nbest, capacity >= B*S] (row r: rank r in the layout of
    ``crf_score_decode``).  One launch, no host sync.  Every operand is checked on the host (dtype, shape, contiguity, the
    kernel's limits: ValueError; then the device: TypeError) before anything is launched."""
    ops = _CrfOperands("crf_nbest", emissions, start, end, trans)
    B, S, Cn = ops.shape
    if isinstance(nbest, bool) or not isinstance(nbest, int):
        raise ValueError("crf_nbest: nbest must be an int, got %s" % type(nbest).__name__)
    if not 1 <= Cn <= CRF_NBEST_MAX_C:
        raise ValueError("crf_nbest: 1 <= num_tags <= %d, got %d" % (CRF_NBEST_MAX_C, Cn))
    if not 1 <= nbest <= CRF_NBEST_MAX_K:
        raise ValueError("crf_nbest: 1 <= nbest <= %d, got %d" % (CRF_NBEST_MAX_K, nbest))
    if B < 1 or S < 1 or S > CRF_NBEST_MAX_S or B > CRF_FLAT_MAX_B:
        raise ValueError("crf_nbest: 1 <= B <= %d and 1 <= S <= %d, got [%d, %d, %d]"
                         % (CRF_FLAT_MAX_B, CRF_NBEST_MAX_S, B, S, Cn))
    if S * Cn * nbest > CRF_NBEST_MAX_SCK:
        raise ValueError("crf_nbest: S * num_tags * nbest <= %d (one back-pointer byte each), got %d * %d * %d = %d"
                         % (CRF_NBEST_MAX_SCK, S, Cn, nbest, S * Cn * nbest))
    ops.vec(lens, "lens", torch.int32, (B,))
    ops.vec(n_paths, "n_paths", torch.int32, (B,))
    ops.vec(scores, "scores", F32, (B, nbest))
    ops.opt(mask, "mask", torch.int64, (B, S))
    ops.vec(tags_flat, "tags_flat", torch.int32,
            fits=lambda t: t.dim() == 2 and t.shape[0] == nbest and t.shape[1] >= B * S,
            what="a contiguous int32 tensor of shape (%d, >= %d)" % (nbest, B * S))
    ops.same_device()
    check(_lib.load().icka_crf_nbest(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(),
                                     trans.data_ptr(), nbest, lens.data_ptr(), n_paths.data_ptr(), scores.data_ptr(),
                                     tags_flat.data_ptr(), tags_flat.shape[1], B, S, Cn, _stream()),
          "icka_crf_nbest")


CRF_SAMPLE_MAX_K = 64


def crf_sample(emissions, mask, start, end, trans, num_samples, seed, seed_dev, lens, log_z, scores, tags_flat):
    """``num_samples`` exact draws from the CRF distribution of every sample (icka_crf_sample, include/icka_hip.h): ``lens``
    int32 [B], ``log_z`` f32 [B], ``scores`` f32 [B, num_samples], ``tags_flat`` int32 [num_samples, capacity >= B*S] (row k:
    draw k in the layout of ``crf_nbest``).  ``seed``: an int in [0, 2^64); ``seed_dev``: None or a device int64 [1] / int32 [2]
    tensor whose two 32-bit words are XORed into the halves of the seed.  One launch, no host sync.  Every operand is checked
    on the host (ValueError, then TypeError for the device) before anything is launched."""
    ops = _CrfOperands("crf_sample", emissions, start, end, trans)
    B, S, Cn = ops.shape
    if isinstance(num_samples, bool) or not isinstance(num_samples, int):
        raise ValueError("crf_sample: num_samples must be an int, got %s" % type(num_samples).__name__)
    if not 1 <= num_samples <= CRF_SAMPLE_MAX_K:
        raise ValueError("crf_sample: 1 <= num_samples <= %d, got %d" % (CRF_SAMPLE_MAX_K, num_samples))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError("crf_sample: seed must be an int in [0, 2^64), got %r" % (seed,))
    if B < 1 or S < 1 or not 1 <= Cn <= 64 or S * Cn > CRF_MAX_SC or B > CRF_FLAT_MAX_B:
        raise ValueError("crf_sample: 1 <= B <= %d, 1 <= num_tags <= 64 and S * num_tags <= %d, got [%d, %d, %d]"
                         % (CRF_FLAT_MAX_B, CRF_MAX_SC, B, S, Cn))
    ops.vec(lens, "lens", torch.int32, (B,))
    ops.vec(log_z, "log_z", F32, (B,))
    ops.vec(scores, "scores", F32, (B, num_samples))
    ops.opt(mask, "mask", torch.int64, (B, S))
    ops.vec(tags_flat, "tags_flat", torch.int32,
            fits=lambda t: t.dim() == 2 and t.shape[0] == num_samples and t.shape[1] >= B * S,
            what="a contiguous int32 tensor of shape (%d, >= %d)" % (num_samples, B * S))
    if seed_dev is not None:
        ok = isinstance(seed_dev, torch.Tensor) and seed_dev.is_contiguous() and (
            (seed_dev.dtype == torch.int64 and seed_dev.numel() == 1) or (seed_dev.dtype == torch.int32 and seed_dev.numel() == 2))
        if not ok:
            raise ValueError("crf_sample: seed_dev must be a contiguous int64 [1] or int32 [2] tensor, got %s %s"
                             % (getattr(seed_dev, "dtype", type(seed_dev).__name__), tuple(getattr(seed_dev, "shape", ()))))
        ops.used.append(seed_dev)
    ops.same_device()
    check(_lib.load().icka_crf_sample(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(),
                                      trans.data_ptr(), num_samples, seed, _ptr(seed_dev), lens.data_ptr(), log_z.data_ptr(),
                                      scores.data_ptr(), tags_flat.data_ptr(), tags_flat.shape[1], B, S, Cn, _stream()),
          "icka_crf_sample")


def _crf_constrained_operands(who, emissions, mask, allowed, start, end, trans, flat_b=False):
    """What the three constrained-CRF entries check before their own operands: the limits, ``allowed`` and ``mask``."""
    ops = _CrfOperands(who, emissions, start, end, trans)
    B, S, Cn = ops.shape
    if not 1 <= Cn <= 64:
        raise ValueError("%s: 1 <= num_tags <= 64 (one lane and one bit per tag), got %d" % (who, Cn))
    if B < 1 or S < 1:
        raise ValueError("%s: empty batch [%d, %d, %d]" % (who, B, S, Cn))
    if S * Cn > CRF_MAX_SC:
        raise ValueError("%s: S * num_tags <= %d, got %d * %d = %d" % (who, CRF_MAX_SC, S, Cn, S * Cn))
    if flat_b and B > CRF_FLAT_MAX_B:
        raise ValueError("%s: B <= %d (the kernel sums the path offsets itself), got %d" % (who, CRF_FLAT_MAX_B, B))
    ops.vec(allowed, "allowed", torch.int64, (B, S))
    ops.opt(mask, "mask", torch.int64, (B, S))
    return ops


def crf_constrained_llh(emissions, mask, allowed, start, end, trans, llh, log_z, log_za, infeasible=None):
    """``llh = log Z_A - log Z`` of the paths inside the per-position allowed sets (``allowed`` int64 [B,S] bit sets), with
    ``log_za`` and ``log_z`` (icka_crf_constrained_llh, include/icka_hip.h).  ``infeasible`` (int32 [1] or None) is ADDED to:
    zero it first.  One launch, no host sync."""
    who = "crf_constrained_llh"
    ops = _crf_constrained_operands(who, emissions, mask, allowed, start, end, trans)
    B, S, Cn = ops.shape
    for t, name in ((llh, "llh"), (log_z, "log_z"), (log_za, "log_za")):
        ops.opt(t, name, F32, (B,))
    ops.opt(infeasible, "infeasible", torch.int32, (1,))
    ops.same_device()
    if llh is None or log_z is None or log_za is None:
        raise ValueError("%s: llh, log_z and log_za are all written" % who)
    check(_lib.load().icka_crf_constrained_llh(emissions.data_ptr(), Cn, _ptr(mask), allowed.data_ptr(), start.data_ptr(),
                                               end.data_ptr(), trans.data_ptr(), llh.data_ptr(), log_z.data_ptr(),
                                               log_za.data_ptr(), _ptr(infeasible), B, S, Cn, _stream()),
          "icka_crf_constrained_llh")
    return llh


def crf_constrained_grad(emissions, mask, allowed, start, end, trans, gllh, d_emissions, d_start, d_end, d_trans):
    """``gllh[b] * d llh[b] / d(.)`` of ``crf_constrained_llh``: ``d_emissions`` [B,S,C] is written, ``d_start``, ``d_end`` and
    ``d_trans`` are ADDED to with atomics (the contract of ``crf_grad``).  One launch, no host sync."""
    who = "crf_constrained_grad"
    ops = _crf_constrained_operands(who, emissions, mask, allowed, start, end, trans)
    B, S, Cn = ops.shape
    for t, name, shape in ((gllh, "gllh", (B,)), (d_emissions, "d_emissions", (B, S, Cn)), (d_start, "d_start", (Cn,)),
                           (d_end, "d_end", (Cn,)), (d_trans, "d_trans", (Cn, Cn))):
        ops.opt(t, name, F32, shape)
    ops.same_device()
    if any(t is None for t in (gllh, d_emissions, d_start, d_end, d_trans)):
        raise ValueError("%s: gllh and the four gradients are all needed" % who)
    check(_lib.load().icka_crf_constrained_grad(emissions.data_ptr(), Cn, _ptr(mask), allowed.data_ptr(), start.data_ptr(),
                                                end.data_ptr(), trans.data_ptr(), gllh.data_ptr(), d_emissions.data_ptr(), Cn,
                                                d_start.data_ptr(), d_end.data_ptr(), d_trans.data_ptr(), B, S, Cn, _stream()),
          "icka_crf_constrained_grad")


def crf_constrained_decode(emissions, mask, allowed, start, end, trans, lens, tags_flat, scores, infeasible=None):
    """The best path inside the allowed sets of every sample (icka_crf_constrained_decode, include/icka_hip.h): ``lens`` int32
    [B], ``tags_flat`` int32 [>= B*S] in the layout of ``crf_score_decode``, ``scores`` f32 [B]; an infeasible sample holds -1
    tags and a -inf score and adds 1 to ``infeasible`` (int32 [1] or None; zero it first).  One launch, no host sync."""
    who = "crf_constrained_decode"
    ops = _crf_constrained_operands(who, emissions, mask, allowed, start, end, trans, flat_b=True)
    B, S, Cn = ops.shape
    ops.opt(lens, "lens", torch.int32, (B,))
    ops.opt(tags_flat, "tags_flat", torch.int32, fits=lambda t: t.dim() == 1 and t.numel() >= B * S,
            what="a contiguous 1-D %s tensor of at least %d entries" % (torch.int32, B * S))
    ops.opt(scores, "scores", F32, (B,))
    ops.opt(infeasible, "infeasible", torch.int32, (1,))
    ops.same_device()
    if lens is None or scores is None or tags_flat is None:
        raise ValueError("%s: lens, tags_flat and scores are all written" % who)
    check(_lib.load().icka_crf_constrained_decode(emissions.data_ptr(), Cn, _ptr(mask), allowed.data_ptr(), start.data_ptr(),
                                                  end.data_ptr(), trans.data_ptr(), lens.data_ptr(), tags_flat.data_ptr(),
                                                  tags_flat.numel(), scores.data_ptr(), _ptr(infeasible), B, S, Cn,
                                                  _stream()),
          "icka_crf_constrained_decode")


CRF_EXPECT_MAX_SC = 4096


def _crf_expect_operands(who, emissions, mask, start, end, trans, second, second_start, second_end, second_trans, relative):
    """What the two expectation entries check before their own operands: the limits, the mask, the second lattice, the mode."""
    ops = _CrfOperands(who, emissions, start, end, trans)
    B, S, Cn = ops.shape
    if not 1 <= Cn <= 64:
        raise ValueError("%s: 1 <= num_tags <= 64 (one lane per tag), got %d" % (who, Cn))
    if B < 1 or S < 1:
        raise ValueError("%s: empty batch [%d, %d, %d]" % (who, B, S, Cn))
    if S * Cn > CRF_EXPECT_MAX_SC:
        raise ValueError("%s: S * num_tags <= %d, got %d * %d = %d" % (who, CRF_EXPECT_MAX_SC, S, Cn, S * Cn))
    if not isinstance(relative, bool):
        raise ValueError("%s: relative must be a bool, got %s" % (who, type(relative).__name__))
    ops.opt(mask, "mask", torch.int64, (B, S))
    ops.opt(second, "second", F32, (B, S, Cn))
    ops.opt(second_start, "second_start", F32, (Cn,))
    ops.opt(second_end, "second_end", F32, (Cn,))
    ops.opt(second_trans, "second_trans", F32, (Cn, Cn))
    return ops


def crf_expect(emissions, mask, start, end, trans, log_z, expect=None, *, second=None, second_start=None, second_end=None,
               second_trans=None, relative=False):
    """``log_z`` = log Z_p and ``expect`` = E_p[r(y)] per sample (icka_crf_expect, include/icka_hip.h): the payoff ``r`` is the
    path score of the second lattice (every part nullable = zeros) or, with ``relative``, p's own score minus it.
    ``expect=None`` computes ``log_z`` only.  One launch, no host sync.  Every operand is checked on the host (ValueError, then
    TypeError for a wrong device) before anything is launched."""
    who = "crf_expect"
    ops = _crf_expect_operands(who, emissions, mask, start, end, trans, second, second_start, second_end, second_trans, relative)
    B, S, Cn = ops.shape
    ops.opt(log_z, "log_z", F32, (B,))
    ops.opt(expect, "expect", F32, (B,))
    ops.same_device()
    if log_z is None:
        raise ValueError("%s: log_z is always written" % who)
    check(_lib.load().icka_crf_expect(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(), trans.data_ptr(),
                                      _ptr(second), Cn, _ptr(second_start), _ptr(second_end), _ptr(second_trans),
                                      int(relative), log_z.data_ptr(), _ptr(expect), B, S, Cn, _stream()),
          "icka_crf_expect")
    return log_z


def crf_expect_grad(emissions, mask, start, end, trans, g_logz, g_expect, d_emissions, d_start, d_end, d_trans, *, second=None,
                    second_start=None, second_end=None, second_trans=None, relative=False, d_second=None,
                    d_second_start=None, d_second_end=None, d_second_trans=None):
    """``g_logz[b] * d log_z[b] / d(.) + g_expect[b] * d expect[b] / d(.)`` of ``crf_expect`` for both lattices
    (icka_crf_expect_grad): ``d_emissions`` and ``d_second`` [B,S,C] are written, the six parameter gradients are ADDED to with
    atomics (the contract of ``crf_grad``).  Every one of the two upstream vectors and the eight outputs may be None: not
    given / not wanted, its work is skipped.  One launch, no host sync."""
    who = "crf_expect_grad"
    ops = _crf_expect_operands(who, emissions, mask, start, end, trans, second, second_start, second_end, second_trans, relative)
    B, S, Cn = ops.shape
    for t, name, shape in ((g_logz, "g_logz", (B,)), (g_expect, "g_expect", (B,)),
                           (d_emissions, "d_emissions", (B, S, Cn)), (d_start, "d_start", (Cn,)), (d_end, "d_end", (Cn,)),
                           (d_trans, "d_trans", (Cn, Cn)), (d_second, "d_second", (B, S, Cn)),
                           (d_second_start, "d_second_start", (Cn,)), (d_second_end, "d_second_end", (Cn,)),
                           (d_second_trans, "d_second_trans", (Cn, Cn))):
        ops.opt(t, name, F32, shape)
    ops.same_device()
    check(_lib.load().icka_crf_expect_grad(emissions.data_ptr(), Cn, _ptr(mask), start.data_ptr(), end.data_ptr(),
                                           trans.data_ptr(), _ptr(second), Cn, _ptr(second_start), _ptr(second_end),
                                           _ptr(second_trans), int(relative), _ptr(g_logz), _ptr(g_expect),
                                           _ptr(d_emissions), Cn, _ptr(d_start), _ptr(d_end), _ptr(d_trans), _ptr(d_second),
                                           Cn, _ptr(d_second_start), _ptr(d_second_end), _ptr(d_second_trans), B, S, Cn,
                                           _stream()),
          "icka_crf_expect_grad")


# ------------------------------------------------------------------------------------------------- chunk metrics
CHUNK_EVAL_MAX_S, CHUNK_EVAL_MAX_IDS, CHUNK_EVAL_MAX_TYPES, CHUNK_EVAL_HEAD = 512, 64, 32, 6


def chunk_eval(labels, output_mask, label_table, counters, ntypes, *, lens=None, tags_flat=None, pred=None):
    """Add the chunk-level counts of one batch into ``counters`` (icka_chunk_eval, include/icka_hip.h): one launch, no host
    sync.  Predictions either as ``lens`` + ``tags_flat`` (a ``crf.DeviceTags``) or as ``pred`` int64 [B, S]."""
    _dev(labels, "labels")
    if labels.dim() != 2:
        raise ValueError("labels must be [B, S], got %s" % (tuple(labels.shape),))
    B, S = labels.shape
    _i64(labels, "labels", (B, S)); _i64(output_mask, "output_mask", (B, S))
    if not 1 <= S <= CHUNK_EVAL_MAX_S or B < 1:
        raise ValueError("chunk_eval: B >= 1 and 1 <= S <= %d, got [%d, %d]" % (CHUNK_EVAL_MAX_S, B, S))
    _dev(label_table, "label_table"); _dev(counters, "counters")
    L = label_table.numel()
    if label_table.dtype != torch.int32 or label_table.dim() != 1 or not label_table.is_contiguous() \
            or not 1 <= L <= CHUNK_EVAL_MAX_IDS:
        raise ValueError("label_table must be a contiguous int32 vector of 1 .. %d words" % CHUNK_EVAL_MAX_IDS)
    if not 1 <= ntypes <= CHUNK_EVAL_MAX_TYPES:
        raise ValueError("chunk_eval: 1 <= ntypes <= %d, got %d" % (CHUNK_EVAL_MAX_TYPES, ntypes))
    if counters.dtype != torch.int64 or counters.dim() != 1 or not counters.is_contiguous() \
            or counters.numel() < CHUNK_EVAL_HEAD + 3 * ntypes:
        raise ValueError("counters must be a contiguous int64 vector of at least %d entries" % (CHUNK_EVAL_HEAD + 3 * ntypes))
    if (lens is None) != (tags_flat is None) or (lens is None) == (pred is None):
        raise ValueError("chunk_eval: predictions as lens + tags_flat or as pred, not both")
    cap = 0
    if lens is not None:
        check_flat_tags(lens, tags_flat, B, 0)
        _dev(lens, "lens"); _dev(tags_flat, "tags_flat")
        cap = tags_flat.numel()
    else:
        _dev(pred, "pred")
        if pred.dtype != torch.int64 or tuple(pred.shape) != (B, S) or (S > 1 and pred.stride(1) != 1) or pred.stride(0) < S:
            raise ValueError("pred must be int64 [%d, %d] with unit column stride" % (B, S))
    check(_lib.load().icka_chunk_eval(_ptr(lens), _ptr(tags_flat), cap, _ptr(pred), _ld(pred), labels.data_ptr(),
                                      output_mask.data_ptr(), label_table.data_ptr(), counters.data_ptr(), B, S, L,
                                      int(ntypes), _stream()), "icka_chunk_eval")


CHUNK_COUNTS_MAX_R = 64


def chunk_counts(lens, tags, labels, output_mask, label_table, counts, ntypes):
    """Write the chunk counts of every (path row, sample) into ``counts`` int32 [R, B, 4] = (correct_preds, total_preds,
    total_correct, bad) (icka_chunk_counts, include/icka_hip.h): ``lens`` int32 [B], ``tags`` int32 [R, capacity] with unit
    column stride (the rows of ``crf_nbest`` / ``crf_sample``, or one ``tags_flat`` as [1, capacity]).  One launch, no host
    sync."""
    _dev(labels, "labels")
    if labels.dim() != 2:
        raise ValueError("labels must be [B, S], got %s" % (tuple(labels.shape),))
    B, S = labels.shape
    _i64(labels, "labels", (B, S)); _i64(output_mask, "output_mask", (B, S))
    if not 1 <= S <= CHUNK_EVAL_MAX_S or not 1 <= B <= CRF_FLAT_MAX_B:
        raise ValueError("chunk_counts: 1 <= B <= %d and 1 <= S <= %d, got [%d, %d]" % (CRF_FLAT_MAX_B, CHUNK_EVAL_MAX_S, B, S))
    _dev(label_table, "label_table"); _dev(counts, "counts"); _dev(lens, "lens"); _dev(tags, "tags")
    L = label_table.numel()
    if label_table.dtype != torch.int32 or label_table.dim() != 1 or not label_table.is_contiguous() \
            or not 1 <= L <= CHUNK_EVAL_MAX_IDS:
        raise ValueError("label_table must be a contiguous int32 vector of 1 .. %d words" % CHUNK_EVAL_MAX_IDS)
    if not 1 <= ntypes <= CHUNK_EVAL_MAX_TYPES:
        raise ValueError("chunk_counts: 1 <= ntypes <= %d, got %d" % (CHUNK_EVAL_MAX_TYPES, ntypes))
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or not lens.is_contiguous():
        raise ValueError("lens must be a contiguous int32 tensor of shape (%d,), got %s %s" % (B, lens.dtype, tuple(lens.shape)))
    if tags.dtype != torch.int32 or tags.dim() != 2 or not 1 <= tags.shape[0] <= CHUNK_COUNTS_MAX_R \
            or (tags.shape[1] > 1 and tags.stride(1) != 1) or (tags.shape[0] > 1 and tags.stride(0) < tags.shape[1]):
        raise ValueError("tags must be int32 [1 .. %d, capacity] with unit column stride, got %s %s"
                         % (CHUNK_COUNTS_MAX_R, tags.dtype, tuple(tags.shape)))
    R, cap = tags.shape
    if counts.dtype != torch.int32 or tuple(counts.shape) != (R, B, 4) or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 tensor of shape %s, got %s %s"
                         % ((R, B, 4), counts.dtype, tuple(counts.shape)))
    check(_lib.load().icka_chunk_counts(lens.data_ptr(), tags.data_ptr(), cap, tags.stride(0) if R > 1 else cap, R,
                                        labels.data_ptr(), output_mask.data_ptr(), label_table.data_ptr(), counts.data_ptr(),
                                        B, S, L, int(ntypes), _stream()), "icka_chunk_counts")
    return counts


def loss_accumulate(loss, acc):
    """acc[0] += loss, acc[1] += 1 on the device (icka_loss_accumulate): ``loss`` one f32 element, ``acc`` f64 [2]."""
    _dev(loss, "loss"); _dev(acc, "acc")
    if loss.dtype != F32 or loss.numel() != 1:
        raise ValueError("loss must hold one f32 element, got %s %s" % (loss.dtype, tuple(loss.shape)))
    if acc.dtype != torch.float64 or acc.numel() != 2 or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous f64 vector of 2")
    check(_lib.load().icka_loss_accumulate(loss.data_ptr(), acc.data_ptr(), _stream()), "icka_loss_accumulate")


# ------------------------------------------------------------------------------------------------- helpers
def cast_f32_to_bf16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _dev(src, "src"); _dev(dst, "dst")
    check(_lib.load().icka_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "icka_cast")
    return dst


def cast_f32_to_bf16_f16(src: torch.Tensor, dst: torch.Tensor, dsth: torch.Tensor) -> None:
    """both 16-bit shadows of an f32 range in one launch: dst bf16, dsth fp16"""
    _dev(src, "src"); _dev(dst, "dst"); _dev(dsth, "dsth")
    if src.dtype != F32 or dst.dtype != BF16 or dsth.dtype != F16 or dst.numel() != src.numel() or dsth.numel() != src.numel():
        raise TypeError("cast_f32_to_bf16_f16: f32 source, bf16 + fp16 destinations of the same length")
    check(_lib.load().icka_cast_f32_to_bf16_f16(src.data_ptr(), dst.data_ptr(), dsth.data_ptr(), src.numel(), _stream()),
          "icka_cast_f32_to_bf16_f16")


def cast_to_f16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """contiguous bf16 / f32 -> fp16 (saturating)"""
    _dev(src, "src"); _dev(dst, "dst")
    if src.dtype not in (BF16, F32) or dst.dtype != F16 or not src.is_contiguous() or not dst.is_contiguous() \
            or src.numel() != dst.numel():
        raise TypeError("cast_to_f16: contiguous bf16/f32 source, contiguous fp16 destination of the same size")
    check(_lib.load().icka_cast_to_f16(src.data_ptr(), int(src.dtype == F32), dst.data_ptr(), src.numel(), _stream()),
          "icka_cast_to_f16")
    return dst


def cast_bf16_to_f32(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _dev(src, "src"); _dev(dst, "dst")
    check(_lib.load().icka_cast_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "icka_cast")
    return dst


def cast_pad_f32_to_bf16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst bf16 [M, ldd>=N]: dst[:, :N] = src f32 [M,N]; pad columns zeroed."""
    _dev(src, "src"); _dev(dst, "dst")
    if src.dtype != F32 or src.dim() != 2 or src.stride(1) != 1 or dst.dtype != BF16 or not dst.is_contiguous():
        raise TypeError("cast_pad: src f32 [M,N] row-major, dst contiguous bf16 [M,ldd]")
    M, N = src.shape
    check(_lib.load().icka_cast_pad_f32_to_bf16(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.shape[1], M, N,
                                                _stream()), "icka_cast_pad_f32_to_bf16")
    return dst


def additive_mask(mask: torch.Tensor, T: int, out: torch.Tensor) -> torch.Tensor:
    """mask int64 [B, >=T] (row-major) -> out f32 [B,T] = (1 - mask[:, :T]) * -10000."""
    _dev(mask, "mask")
    if mask.dtype != torch.int64 or mask.stride(1) != 1:
        raise TypeError("mask must be int64 row-major")
    check(_lib.load().icka_additive_mask(mask.data_ptr(), mask.stride(0), out.data_ptr(), mask.shape[0], T,
                                         _stream()), "icka_additive_mask")
    return out


def dropout(x, y, *, y2=None, p_drop=0.0, seed=0):
    _mat(x, "x"); _mat(y, "y")
    M, H = x.shape
    check(_lib.load().icka_dropout(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _ptr(y2), _ld(y2), M, H,
                                   p_drop, seed, _stream()), "icka_dropout")
    return y


def dropout_mask(n: int, p_drop: float, seed: int, device) -> torch.Tensor:
    out = torch.empty(n, dtype=F32, device=device)
    check(_lib.load().icka_dropout_mask(out.data_ptr(), n, p_drop, seed, _stream()), "icka_dropout_mask")
    return out


def attn_dropout_mask(rows: int, Skv: int, p_drop: float, seed: int, device) -> torch.Tensor:
    """The keep-multiplier [rows, Skv] the attention kernels apply to the probabilities (two decisions per hash: NOT
    dropout_mask of the flat index); rows = (batch * heads + head) * Sq + query."""
    out = torch.empty(rows, Skv, dtype=F32, device=device)
    check(_lib.load().icka_attn_dropout_mask(out.data_ptr(), rows, Skv, p_drop, seed, _stream()), "icka_attn_dropout_mask")
    return out


def regions_to_tokens(src: torch.Tensor, dst: torch.Tensor, B: int, R: int, Cc: int, layout: int) -> torch.Tensor:
    _dev(src, "src")
    if src.dtype != F32 or not src.is_contiguous():
        raise TypeError("region features must be contiguous f32")
    check(_lib.load().icka_regions_to_tokens(src.data_ptr(), dst.data_ptr(), B, R, Cc, layout, _stream()),
          "icka_regions_to_tokens")
    return dst


def regions_to_tokens_h(src: torch.Tensor, dst: torch.Tensor, dst16: torch.Tensor, B: int, R: int, Cc: int, layout: int) -> None:
    """regions_to_tokens with an fp16 twin of the tokens (the "mixed16" operand of the region projection)."""
    _dev(src, "src"); _dev(dst, "dst"); _dev(dst16, "dst16")
    if src.dtype != F32 or not src.is_contiguous() or dst.dtype != BF16 or dst16.dtype != F16:
        raise TypeError("regions_to_tokens_h: contiguous f32 features, bf16 + fp16 token buffers")
    check(_lib.load().icka_regions_to_tokens_h(src.data_ptr(), dst.data_ptr(), dst16.data_ptr(), B, R, Cc, layout, _stream()),
          "icka_regions_to_tokens_h")


def colsum_workspace(N: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().icka_colsum_workspace_floats(N), dtype=F32, device=device)


def colsum(x, out, partials, accumulate=True):
    _mat(x, "x")
    M, N = x.shape
    check(_lib.load().icka_colsum(x.data_ptr(), x.stride(0), out.data_ptr(), partials.data_ptr(), M, N,
                                  int(accumulate), _stream()), "icka_colsum")
    return out


def gate_bwd(dout, g, cross, du, dcross, dcross_in=None):
    _mat(dout, "dout"); _mat(cross, "cross")
    M, H = dout.shape
    check(_lib.load().icka_gate_bwd(dout.data_ptr(), dout.stride(0), g.data_ptr(), cross.data_ptr(), cross.stride(0),
                                    _ptr(dcross_in), _ld(dcross_in), du.data_ptr(), dcross.data_ptr(),
                                    dcross.stride(0), M, H, _stream()), "icka_gate_bwd")


def add_bf16(a, b, out):
    check(_lib.load().icka_add_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "icka_add")
    return out


def token_ce(logits, labels, mask, loss_sum, count, dlogits):
    """logits f32 [M,C]; labels/mask int64 [M]; dlogits bf16 [M, ldd>=C] (unscaled, see scale_by_ratio)."""
    M, Cn = logits.shape
    check(_lib.load().icka_token_ce(logits.data_ptr(), logits.stride(0), labels.data_ptr(), mask.data_ptr(),
                                    loss_sum.data_ptr(), count.data_ptr(), dlogits.data_ptr(), dlogits.stride(0),
                                    M, Cn, _stream()), "icka_token_ce")


def token_ce_fused(logits, labels, mask, stats, dlogits):
    """Token CE without accumulator fill / atomics: stats f32[3] <- (loss sum, #valid, mean loss); dlogits bf16 or f32
    [M, ldd>=C] unscaled."""
    M, Cn = logits.shape
    lib = _lib.load()
    part = torch.empty(lib.icka_token_ce_workspace_floats(M), dtype=F32, device=logits.device)
    check(lib.icka_token_ce_fused(logits.data_ptr(), logits.stride(0), labels.data_ptr(), mask.data_ptr(),
                                  stats.data_ptr(), part.data_ptr(), dlogits.data_ptr(), dlogits.stride(0),
                                  int(dlogits.dtype == F32), M, Cn, _stream()), "icka_token_ce_fused")


def zero_(t: torch.Tensor) -> torch.Tensor:
    """Clear a contiguous f32 device tensor with the library's fill kernel."""
    _dev(t, "t")
    if t.dtype != F32 or not t.is_contiguous():
        raise TypeError("zero_: contiguous f32 tensor")
    check(_lib.load().icka_zero_f32(t.data_ptr(), t.numel(), _stream()), "icka_zero_f32")
    return t


def zero_rows_(t: torch.Tensor, row0: int) -> None:
    """Clear rows [row0, end) of a contiguous 16-bit [rows, cols] matrix (the padding rows of a row-padded operand) with the
    library's fill kernel."""
    _dev(t, "t")
    if t.dim() != 2 or not t.is_contiguous() or t.element_size() != 2:
        raise TypeError("zero_rows_: contiguous 16-bit [rows, cols] matrix")
    n16 = (t.shape[0] - row0) * t.shape[1]
    if n16 <= 0:
        return
    if (row0 * t.shape[1]) % 2 or n16 % 2:
        raise ValueError("zero_rows_: the cleared range must be a whole number of 32-bit words")
    check(_lib.load().icka_zero_f32(t.data_ptr() + 2 * row0 * t.shape[1], n16 // 2, _stream()), "icka_zero_f32")


def scale_by_ratio(x, y, num=None, den=None):
    """y = x * num[0] / max(den[0], 1) with device scalars (None = 1)."""
    check(_lib.load().icka_scale_by_ratio(x.data_ptr(), y.data_ptr(), _ptr(num), _ptr(den), x.numel(), _stream()),
          "icka_scale_by_ratio")
    return y


def scalar_ratio(out, num, den):
    check(_lib.load().icka_scalar_ratio(out.data_ptr(), num.data_ptr(), den.data_ptr(), _stream()),
          "icka_scalar_ratio")
    return out


def set_dropout_nonce(words: Optional[torch.Tensor]) -> None:
    """Register (or clear) the 2 x int32 device tensor whose value every dropout kernel folds into its seed."""
    if words is not None and (not words.is_cuda or words.numel() < 2 or words.element_size() != 4):
        raise TypeError("nonce must be a device tensor of two 32-bit words")
    global _NONCE_PTR
    check(_lib.load().icka_set_dropout_nonce(_ptr(words)), "icka_set_dropout_nonce")
    _NONCE_PTR = _ptr(words)


_NONCE_PTR = None


def clear_dropout_nonce_if(words: torch.Tensor) -> None:
    """Unregister ``words`` if (and only if) it is the currently registered nonce (its owner is going away)."""
    if _NONCE_PTR is not None and words is not None and _NONCE_PTR == words.data_ptr():
        set_dropout_nonce(None)


def bump_dropout_nonce(words: torch.Tensor) -> None:
    check(_lib.load().icka_bump_dropout_nonce(words.data_ptr(), _stream()), "icka_bump_dropout_nonce")


# ------------------------------------------------------------------------------------------------- data parallel
class DpFlagError(RuntimeError):
    """A bucket-ready wait on the communication stream gave up: that step's all-reduce ran on unfinished gradients (the
    bucket was poisoned with a NaN)."""


def dp_chunk_table(ranges, device) -> torch.Tensor:
    """Chunk table for dp_cast_chunks: [(lo, hi)] element ranges (multiples of 8) -> int64 [n, 2] device tensor of
    (first element, count <= icka_dp_chunk_elems())."""
    ch = _lib.load().icka_dp_chunk_elems()
    rows = []
    for lo, hi in ranges:
        if lo % 8 or hi % 8:
            raise ValueError("chunk ranges must start and end on multiples of 8 elements")
        while lo < hi:
            n = min(ch, hi - lo)
            rows.append((lo, n))
            lo += n
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 2)


def dp_cast_chunks(src_f32: torch.Tensor, dst_bf16: torch.Tensor, table: torch.Tensor) -> None:
    """dst[i] = bf16(src[i]) over the chunks of ``table`` (dp_chunk_table); src / dst are the whole flat buffers."""
    _dev(src_f32, "src"); _dev(dst_bf16, "dst")
    if src_f32.dtype != F32 or dst_bf16.dtype != BF16 or src_f32.numel() != dst_bf16.numel():
        raise TypeError("dp_cast_chunks: f32 source and bf16 destination of the same length")
    if table.numel() == 0:
        return
    check(_lib.load().icka_dp_cast_chunks(src_f32.data_ptr(), dst_bf16.data_ptr(), table.data_ptr(), table.shape[0],
                                          _stream()), "icka_dp_cast_chunks")


def dp_cast_back_scaled(src_bf16: torch.Tensor, dst_f32: torch.Tensor, scale: float) -> None:
    _dev(src_bf16, "src"); _dev(dst_f32, "dst")
    if src_bf16.dtype != BF16 or dst_f32.dtype != F32 or src_bf16.numel() != dst_f32.numel():
        raise TypeError("dp_cast_back_scaled: bf16 source and f32 destination of the same length")
    check(_lib.load().icka_dp_cast_back_scaled(src_bf16.data_ptr(), dst_f32.data_ptr(), src_bf16.numel(), float(scale),
                                               _stream()), "icka_dp_cast_back_scaled")


def dp_check_error(where: str = "") -> None:
    lib = _lib.load()
    if lib.icka_dp_error() != 0:
        lib.icka_dp_clear_error()
        raise DpFlagError("icka_amd data-parallel step%s: a bucket-ready wait on the communication stream gave up (the "
                          "compute graph did not reach the bucket's flag in time); the first gradients of that bucket were "
                          "set to NaN after the exchange (icka_dp_poison_if / icka_dp_poison_final), so a global-norm clip or "
                          "an optimizer step that consumed them produced NaN" % ((" (" + where + ")") if where else ""))


# ------------------------------------------------------------------------------------------------- capturable parameter update
def optim_state_new(device) -> torch.Tensor:
    """A zeroed ``icka_optim_state`` block (include/icka_hip.h; mirror: _lib.OptimState) as a uint8 device tensor."""
    n = C.sizeof(_lib.OptimState)
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device).view(torch.uint8)[:n]


def optim_state_write(state: torch.Tensor, host: "_lib.OptimState", lo: int, hi: int) -> None:
    """Upload bytes [lo, hi) of ``host`` into the device block (outside a capture: a host-to-device copy)."""
    state[lo:hi].copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8)[lo:hi])


def optim_state_read(state: torch.Tensor) -> "_lib.OptimState":
    """The device block as a host structure (one device-to-host copy: synchronises)."""
    return _lib.OptimState.from_buffer_copy(bytes(state.cpu().tolist()))


def optim_chunk_table3(ranges_per_group, device) -> torch.Tensor:
    """Chunk table of icka_optim_adamw_dev: per group a list of [(lo, hi)] element ranges (multiples of 8) -> int64 [n, 3]
    device tensor of (first element, count <= icka_optim_chunk_elems(), group)."""
    if len(ranges_per_group) > _lib.OPTIM_MAX_GROUPS:
        raise ValueError("at most %d parameter groups" % _lib.OPTIM_MAX_GROUPS)
    ch = _lib.load().icka_optim_chunk_elems()
    rows = []
    for gi, ranges in enumerate(ranges_per_group):
        for lo, hi in ranges:
            if lo % 8 or hi % 8:
                raise ValueError("chunk ranges must start and end on multiples of 8 elements")
            while lo < hi:
                n = min(ch, hi - lo)
                rows.append((lo, n, gi))
                lo += n
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 3)


def optim_sqnorm(gflat: torch.Tensor, table: torch.Tensor, partials: torch.Tensor) -> None:
    check(_lib.load().icka_optim_sqnorm(gflat.data_ptr(), table.data_ptr(), table.shape[0], partials.data_ptr(), _stream()),
          "icka_optim_sqnorm")


def optim_prepare(partials: Optional[torch.Tensor], n: int, max_norm: float, state: torch.Tensor, dry: bool = False,
                  guard: bool = True) -> None:
    """Norm, non-finite test, clip coefficient and the values of the next update into the state block; advances t."""
    flags = (_lib.OPTIM_DRY if dry else 0) | (0 if guard else _lib.OPTIM_NO_GUARD)
    check(_lib.load().icka_optim_prepare(_ptr(partials), int(n), float(max_norm), flags, state.data_ptr(), _stream()),
          "icka_optim_prepare")


def optim_adamw_dev(flat, gflat, m, v, shadow, shadow16, table3: torch.Tensor, state: torch.Tensor) -> None:
    """AdamW over the chunks of all groups with the values of the state block (skipped when its skip word is set)."""
    for n, t in (("params", flat), ("grads", gflat), ("exp_avg", m), ("exp_avg_sq", v)):
        _dev(t, n)
        if t.dtype != F32 or t.numel() != flat.numel():
            raise TypeError("optim_adamw_dev: %s must be f32 of the parameters' length" % n)
    if table3.dtype != torch.int64 or table3.dim() != 2 or table3.shape[1] != 3 or not table3.is_contiguous():
        raise TypeError("optim_adamw_dev: the chunk table is a contiguous int64 [n, 3] tensor (optim_chunk_table3)")
    check(_lib.load().icka_optim_adamw_dev(flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(shadow),
                                           _ptr(shadow16), table3.data_ptr(), table3.shape[0], state.data_ptr(), _stream()),
          "icka_optim_adamw_dev")


# ------------------------------------------------------------------------------------------------- averaged weights (EMA / SWA)
def average_state_new(device) -> torch.Tensor:
    """A zeroed ``icka_average_state`` block (include/icka_hip.h; mirror: _lib.AverageState) as a uint8 device tensor."""
    n = C.sizeof(_lib.AverageState)
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device).view(torch.uint8)[:n]


def average_state_write(state: torch.Tensor, host: "_lib.AverageState", lo: int, hi: int) -> None:
    """Upload bytes [lo, hi) of ``host`` into the device block (outside a capture: a host-to-device copy)."""
    state[lo:hi].copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8)[lo:hi])


def average_state_read(state: torch.Tensor) -> "_lib.AverageState":
    """The device block as a host structure (one device-to-host copy: synchronises)."""
    return _lib.AverageState.from_buffer_copy(bytes(state.cpu().tolist()))


def _average_operands(what: str, flat, avg, table) -> None:
    for n, t in (("params", flat), ("avg", avg)):
        _dev(t, n)
        if t.dtype != F32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != flat.numel():
            raise TypeError("%s: %s must be a contiguous 1-D f32 tensor of the parameters' length" % (what, n))
    if flat.data_ptr() == avg.data_ptr():
        raise ValueError("%s: params and avg are the same buffer" % what)
    _dev(table, "table")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2 or not table.is_contiguous():
        raise TypeError("%s: the chunk table is a contiguous int64 [n, 2] tensor (dp_chunk_table)" % what)


def _state_operand(what: str, state: torch.Tensor, mirror) -> None:
    _dev(state, "state")
    if state.dtype != torch.uint8 or state.numel() != C.sizeof(mirror) or not state.is_contiguous():
        raise TypeError("%s: the state block is a uint8 tensor of %d bytes" % (what, C.sizeof(mirror)))


def optim_average(flat: torch.Tensor, avg: torch.Tensor, table: torch.Tensor, decay: float) -> None:
    """avg <- avg + (1 - decay) * (flat - avg) over the chunks of ``table`` (dp_chunk_table); decay == 0 copies."""
    _average_operands("optim_average", flat, avg, table)
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError("optim_average: decay in [0, 1), got %r" % (decay,))
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_optim_average(flat.data_ptr(), avg.data_ptr(), table.data_ptr(), table.shape[0], float(decay),
                                         _stream()), "icka_optim_average")


def optim_average_prepare(average_state: torch.Tensor, optim_state: torch.Tensor) -> None:
    """Behind optim_prepare: whether the update it admitted is averaged, and this update's decay, into the average block."""
    _state_operand("optim_average_prepare", average_state, _lib.AverageState)
    _state_operand("optim_average_prepare", optim_state, _lib.OptimState)
    check(_lib.load().icka_optim_average_prepare(average_state.data_ptr(), optim_state.data_ptr(), _stream()),
          "icka_optim_average_prepare")


def optim_average_dev(flat: torch.Tensor, avg: torch.Tensor, table: torch.Tensor, average_state: torch.Tensor) -> None:
    """optim_average with the decay of the average block (nothing is touched when its apply word is 0)."""
    _average_operands("optim_average_dev", flat, avg, table)
    _state_operand("optim_average_dev", average_state, _lib.AverageState)
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_optim_average_dev(flat.data_ptr(), avg.data_ptr(), table.data_ptr(), table.shape[0],
                                             average_state.data_ptr(), _stream()), "icka_optim_average_dev")


def optim_swap(flat: torch.Tensor, avg: torch.Tensor, shadow: Optional[torch.Tensor], shadow16: Optional[torch.Tensor],
               table: torch.Tensor) -> None:
    """Exchange flat and avg over the chunks of ``table`` and write the 16-bit shadows of the new flat (either may be None)."""
    _average_operands("optim_swap", flat, avg, table)
    for n, t, dt in (("shadow", shadow, BF16), ("shadow16", shadow16, F16)):
        if t is not None:
            _dev(t, n)
            if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() != flat.numel():
                raise TypeError("optim_swap: %s must be a contiguous 1-D %s tensor of the parameters' length" % (n, dt))
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_optim_swap(flat.data_ptr(), avg.data_ptr(), _ptr(shadow), _ptr(shadow16), table.data_ptr(),
                                      table.shape[0], _stream()), "icka_optim_swap")


# ------------------------------------------------------------------------------------------------- sharpness-aware minimisation
def sam_state_new(device) -> torch.Tensor:
    """A zeroed ``icka_sam_state`` block (include/icka_hip.h; mirror: _lib.SamState) as a uint8 device tensor."""
    n = C.sizeof(_lib.SamState)
    return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device).view(torch.uint8)[:n]


def sam_state_read(state: torch.Tensor) -> "_lib.SamState":
    """The device block as a host structure (one device-to-host copy: synchronises)."""
    return _lib.SamState.from_buffer_copy(bytes(state.cpu().tolist()))


def _sam_operands(what: str, flat, others, shadow, shadow16, table) -> None:
    """flat: the parameters; others: (name, f32 buffer of the same layout) pairs, none of them the same buffer as another."""
    bufs = [("params", flat)] + list(others)
    for n, t in bufs:
        _dev(t, n)
        if t.dtype != F32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != flat.numel():
            raise TypeError("%s: %s must be a contiguous 1-D f32 tensor of the parameters' length" % (what, n))
    if len({t.data_ptr() for _, t in bufs}) != len(bufs):
        raise ValueError("%s: %s must be separate buffers" % (what, ", ".join(n for n, _ in bufs)))
    for n, t, dt in (("shadow", shadow, BF16), ("shadow16", shadow16, F16)):
        if t is not None:
            _dev(t, n)
            if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() != flat.numel():
                raise TypeError("%s: %s must be a contiguous 1-D %s tensor of the parameters' length" % (what, n, dt))
    _dev(table, "table")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2 or not table.is_contiguous():
        raise TypeError("%s: the chunk table is a contiguous int64 [n, 2] tensor (dp_chunk_table)" % what)


def sam_sqnorm(flat: torch.Tensor, gflat: torch.Tensor, table: torch.Tensor, partials: torch.Tensor, adaptive: bool) -> None:
    """partials[b] = sum over chunk b of (t g)^2, t = 1 or (``adaptive``) |p|; not adaptive: icka_optim_sqnorm's bits."""
    _sam_operands("sam_sqnorm", flat, [("grads", gflat)], None, None, table)
    _dev(partials, "partials")
    if partials.dtype != F32 or not partials.is_contiguous() or partials.numel() < table.shape[0]:
        raise TypeError("sam_sqnorm: partials must be a contiguous f32 tensor of at least one element per chunk")
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_sam_sqnorm(flat.data_ptr(), gflat.data_ptr(), table.data_ptr(), table.shape[0], int(bool(adaptive)),
                                      partials.data_ptr(), _stream()), "icka_sam_sqnorm")


def sam_prepare(partials: Optional[torch.Tensor], n: int, rho: float, state: torch.Tensor, dry: bool = False) -> None:
    """Norm, step scale and the skip word of the ascent behind it into the state block; counts the ascent (``dry``: not)."""
    _state_operand("sam_prepare", state, _lib.SamState)
    if not float(rho) > 0.0:
        raise ValueError("sam_prepare: rho must be positive, got %r" % (rho,))
    if n > 0 and (partials is None or partials.numel() < n):
        raise ValueError("sam_prepare: %d partials asked for, %s given" % (n, None if partials is None else partials.numel()))
    check(_lib.load().icka_sam_prepare(_ptr(partials), int(n), float(rho), _lib.SAM_DRY if dry else 0, state.data_ptr(),
                                       _stream()), "icka_sam_prepare")


def sam_ascend(flat: torch.Tensor, gflat: torch.Tensor, backup: torch.Tensor, shadow: Optional[torch.Tensor],
               shadow16: Optional[torch.Tensor], table: torch.Tensor, state: torch.Tensor, adaptive: bool) -> None:
    """backup <- flat; flat <- flat + e over the chunks of ``table``, with the 16-bit shadows of the new flat (either may be
    None); nothing is touched when the block's skip word is set."""
    _sam_operands("sam_ascend", flat, [("grads", gflat), ("backup", backup)], shadow, shadow16, table)
    _state_operand("sam_ascend", state, _lib.SamState)
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_sam_ascend(flat.data_ptr(), gflat.data_ptr(), backup.data_ptr(), _ptr(shadow), _ptr(shadow16),
                                      table.data_ptr(), table.shape[0], int(bool(adaptive)), state.data_ptr(), _stream()),
          "icka_sam_ascend")


def sam_restore(flat: torch.Tensor, backup: torch.Tensor, shadow: Optional[torch.Tensor], shadow16: Optional[torch.Tensor],
                table: torch.Tensor, state: torch.Tensor) -> None:
    """flat <- backup over the chunks of ``table``, with the 16-bit shadows; nothing is touched when the skip word is set."""
    _sam_operands("sam_restore", flat, [("backup", backup)], shadow, shadow16, table)
    _state_operand("sam_restore", state, _lib.SamState)
    if table.shape[0] == 0:
        return
    check(_lib.load().icka_sam_restore(flat.data_ptr(), backup.data_ptr(), _ptr(shadow), _ptr(shadow16), table.data_ptr(),
                                       table.shape[0], state.data_ptr(), _stream()), "icka_sam_restore")


# ------------------------------------------------------------------------------------------------- per-sample gates
def sample_gate_fwd(a, c, gate, mode, out, B, S):
    _mat(a, "a"); _mat(out, "out")
    H = a.shape[1]
    check(_lib.load().icka_sample_gate_fwd(a.data_ptr(), a.stride(0), _ptr(c), _ld(c), gate.data_ptr(), mode,
                                           out.data_ptr(), out.stride(0), B, S, H, _stream()), "icka_sample_gate_fwd")
    return out


def sample_gate_fwd_h(a16, gate, mode, out, out16, B, S):
    """out (bf16) and out16 (fp16) = g(gate[b]) * a16 (fp16): the "mixed16" form of the gate without blend operand."""
    _mat(a16, "a16", F16); _mat(out, "out"); _mat(out16, "out16", F16)
    H = a16.shape[1]
    if out.stride(0) != out16.stride(0):
        raise ValueError("out and out16 share one row stride")
    check(_lib.load().icka_sample_gate_fwd_h(a16.data_ptr(), a16.stride(0), gate.data_ptr(), mode, out.data_ptr(),
                                             out16.data_ptr(), out.stride(0), B, S, H, _stream()), "icka_sample_gate_fwd_h")
    return out


def sample_gate_bwd(dout, a, c, gate, mode, da, dc, dgate, B, S):
    _mat(dout, "dout"); _mat(a, "a"); _mat(da, "da")
    H = a.shape[1]
    check(_lib.load().icka_sample_gate_bwd(dout.data_ptr(), dout.stride(0), a.data_ptr(), a.stride(0), _ptr(c), _ld(c),
                                           gate.data_ptr(), mode, da.data_ptr(), da.stride(0), _ptr(dc), _ld(dc),
                                           dgate.data_ptr(), B, S, H, _stream()), "icka_sample_gate_bwd")


def crs_fwd(seq, cross, W, bias, crs, B, S):
    _mat(seq, "seq"); _mat(cross, "cross")
    H = seq.shape[1]
    check(_lib.load().icka_crs_fwd(seq.data_ptr(), seq.stride(0), cross.data_ptr(), cross.stride(0), W.data_ptr(),
                                   _ptr(bias), crs.data_ptr(), B, S, H, _stream()), "icka_crs_fwd")
    return crs


def crs_bwd(dcrs, seq, cross, W, dseq, dcross, dW, dbias, B, S, accumulate):
    H = seq.shape[1]
    check(_lib.load().icka_crs_bwd(dcrs.data_ptr(), seq.data_ptr(), seq.stride(0), cross.data_ptr(), cross.stride(0),
                                   W.data_ptr(), dseq.data_ptr(), dcross.data_ptr(), dW.data_ptr(), _ptr(dbias), B, S, H,
                                   int(accumulate), _stream()), "icka_crs_bwd")


# ------------------------------------------------------------------------------------------------- auxiliary objective
_OBJ_DTYPE = {F32: 0, BF16: 1, F16: 2}


def _obj_rows(t, v):
    for n, x in (("t", t), ("v", v)):
        _dev(x, n)
        if x.dtype not in _OBJ_DTYPE or x.dim() != 2 or x.stride(1) != 1:
            raise ValueError("%s must be 2-D row-major f32 / bf16 / fp16" % n)
    if t.dtype != v.dtype or t.shape != v.shape:
        raise ValueError("t and v must have one dtype and shape, got %s %s / %s %s" % (t.dtype, tuple(t.shape), v.dtype,
                                                                                       tuple(v.shape)))
    B, D = t.shape
    if not (1 <= B <= 256) or D % 8 or not (8 <= D <= 4096):
        raise ValueError("contrastive loss: 1 <= B <= 256 and D a multiple of 8 in [8, 4096], got B=%d D=%d" % (B, D))
    return B, D


def contrastive_workspace(B: int, device) -> torch.Tensor:
    return torch.empty(int(_lib.load().icka_contrastive_workspace_floats(B)), dtype=F32, device=device)


def contrastive_fwd(t, v, temp: float, temp_lamb: float, stats, ws, crs=None, n_neg: int = 0):
    """stats f32[2] = (contrastive loss, relevance cross-entropy or 0); ws keeps what the backward reads."""
    B, D = _obj_rows(t, v)
    if crs is not None and (crs.dtype != F32 or tuple(crs.shape) != (B, 2) or not crs.is_contiguous()):
        raise ValueError("crs must be contiguous f32 [B, 2]")
    check(_lib.load().icka_contrastive_fwd(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), _OBJ_DTYPE[t.dtype], B, D,
                                           float(temp), float(temp_lamb), _ptr(crs), int(n_neg), stats.data_ptr(),
                                           ws.data_ptr(), _stream()), "icka_contrastive_fwd")
    return stats


def contrastive_bwd(t, v, temp: float, temp_lamb: float, ws, dcl, dt, dv, crs=None, n_neg: int = 0, dcrs=None, dcrs_loss=None):
    """dt, dv (contiguous f32, any input dtype) from the device-resident upstream gradient dcl (f32, one element) of the contrastive
    loss; with crs also dcrs f32 [B,2] from dcrs_loss, the upstream gradient of the relevance cross-entropy."""
    B, D = _obj_rows(t, v)
    for n, x in (("dt", dt), ("dv", dv)):
        if x.dtype != F32 or tuple(x.shape) != (B, D) or not x.is_contiguous():
            raise ValueError("%s must be contiguous f32 [%d, %d]" % (n, B, D))
    for n, x in (("dcl", dcl), ("dcrs_loss", dcrs_loss)):
        if x is not None and (x.dtype != F32 or x.numel() != 1):
            raise ValueError("%s must be one f32 element" % n)
    if crs is not None and (dcrs is None or dcrs_loss is None or dcrs.dtype != F32 or tuple(dcrs.shape) != (B, 2)
                            or not dcrs.is_contiguous()):
        raise ValueError("with crs: dcrs contiguous f32 [B, 2] and dcrs_loss")
    check(_lib.load().icka_contrastive_bwd(t.data_ptr(), t.stride(0), v.data_ptr(), v.stride(0), _OBJ_DTYPE[t.dtype], B, D,
                                           float(temp), float(temp_lamb), ws.data_ptr(), dcl.data_ptr(), _ptr(dcrs_loss), dt.data_ptr(),
                                           dv.data_ptr(), _ptr(crs), int(n_neg), _ptr(dcrs), _stream()),
          "icka_contrastive_bwd")


def relu_bwd(dy, y, dx):
    """dx = dy * [y > 0], contiguous bf16 or f32 (relu_bwd(x, x, out) = relu(x))."""
    for n, t in (("dy", dy), ("y", y), ("dx", dx)):
        _dev(t, n)
        if t.dtype not in (BF16, F32) or t.dtype != y.dtype or not t.is_contiguous():
            raise ValueError("%s must be contiguous bf16 or f32 (one dtype)" % n)
    if dy.numel() != y.numel() or dx.numel() != y.numel():
        raise ValueError("relu_bwd: size mismatch")
    check(_lib.load().icka_relu_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.numel(), int(y.dtype == F32), _stream()),
          "icka_relu_bwd")
    return dx


def sample_swap(x, y, B: int, n_neg: int):
    """y = x with the negative-sample pairs of the last n_neg of B samples exchanged (x, y contiguous, same shape)."""
    _dev(x, "x"); _dev(y, "y")
    if not (x.is_contiguous() and y.is_contiguous()) or x.dtype != y.dtype or x.shape != y.shape or x.numel() % B:
        raise ValueError("sample_swap: x and y contiguous, one dtype and shape, B samples")
    check(_lib.load().icka_sample_swap(x.data_ptr(), y.data_ptr(), B, x.numel() // B * x.element_size(), int(n_neg), _stream()),
          "icka_sample_swap")
    return y


# ---------------------------------------------------------------------------------------------------- train-mode BatchNorm
def gemm_bn_stats(a: torch.Tensor, w: torch.Tensor, rows_valid: int):
    """Convolution GEMM of a train-mode BatchNorm layer: raw bf16 [M, N] = a . w^T (a [M, K], w [N, K], NT; no bias, no
    activation) and the partial statistics f32 [3, M/128, N] = (count, mean, M2) of each 128-row tile and channel over the
    rows < rows_valid, from the f32 accumulators (icka_gemm_bn_stats)."""
    _mat(a, "a"); _mat(w, "w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("gemm_bn_stats: a [M, K], w [N, K]")
    raw = torch.empty(M, N, dtype=BF16, device=a.device)
    part = torch.empty(3, M // 128, N, dtype=F32, device=a.device)
    check(_lib.load().icka_gemm_bn_stats(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), raw.data_ptr(), N, M, N, K,
                                         rows_valid, part.data_ptr(), _stream()), "icka_gemm_bn_stats")
    return raw, part


def conv3x3_bn_stats(x: torch.Tensor, w: torch.Tensor, B: int, H: int, W: int, C: int, Cout: int, stride: int, rows_padded: int,
                     zeros: torch.Tensor):
    """The implicit 3x3 / pad 1 convolution of icka_conv3x3_gemm (x NHWC bf16 rows, w bf16 [Cout, 9 C]) for a train-mode
    BatchNorm layer: raw bf16 [rows_padded, Cout] + partials f32 [3, rows_padded/128, Cout] (icka_conv3x3_gemm_stats)."""
    _dev(x, "x")
    if x.dtype != BF16 or w.dtype != BF16 or not x.is_contiguous() or not w.is_contiguous():
        raise ValueError("conv3x3_bn_stats: contiguous bf16 operands")
    raw = torch.empty(rows_padded, Cout, dtype=BF16, device=x.device)
    part = torch.empty(3, rows_padded // 128, Cout, dtype=F32, device=x.device)
    check(_lib.load().icka_conv3x3_gemm_stats(x.data_ptr(), w.data_ptr(), raw.data_ptr(), B, H, W, C, Cout, stride, rows_padded,
                                              zeros.data_ptr(), part.data_ptr(), _stream()), "icka_conv3x3_gemm_stats")
    return raw, part


def bn_finalize(part: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: torch.Tensor,
                running_var: torch.Tensor, num_batches_tracked: torch.Tensor, momentum: Optional[float], eps: float):
    """Batch statistics from the partials of gemm_bn_stats / conv3x3_bn_stats -> (scale, shift) f32 [C], and the running
    statistics updated in place on the device (icka_bn_finalize).  momentum None = cumulative average."""
    _dev(part, "partials")
    _, tiles, Cn = part.shape
    for t, name in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t.dtype != F32 or t.numel() != Cn or not t.is_contiguous() or t.device != part.device:
            raise TypeError("bn_finalize: %s must be contiguous f32 [%d] on %s" % (name, Cn, part.device))
    if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.device != part.device:
        raise TypeError("bn_finalize: num_batches_tracked must be an int64 device tensor")
    scale = torch.empty(Cn, dtype=F32, device=part.device)
    shift = torch.empty(Cn, dtype=F32, device=part.device)
    check(_lib.load().icka_bn_finalize(part.data_ptr(), tiles, Cn, weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(),
                                       running_var.data_ptr(), num_batches_tracked.data_ptr(),
                                       -1.0 if momentum is None else float(momentum), float(eps), scale.data_ptr(),
                                       shift.data_ptr(), _stream()), "icka_bn_finalize")
    return scale, shift


def bn_apply(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, rows_valid: int, relu: bool = True,
             residual: Optional[torch.Tensor] = None, res_scale: Optional[torch.Tensor] = None,
             res_shift: Optional[torch.Tensor] = None, nbt=(), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = [relu](raw * scale + shift [+ residual (* res_scale + res_shift)]) on rows < rows_valid, zeros below; adds 1 to each
    num_batches_tracked tensor of ``nbt`` (at most two).  out defaults to raw (in place) (icka_bn_apply)."""
    _mat(raw, "raw")
    if residual is not None:
        _mat(residual, "residual")
        if residual.shape != raw.shape or not residual.is_contiguous():
            raise ValueError("bn_apply: residual must match raw")
    if not raw.is_contiguous() or len(nbt) > 2:
        raise ValueError("bn_apply: contiguous raw, at most two counters")
    out = raw if out is None else out
    p = [t.data_ptr() for t in nbt] + [None] * (2 - len(nbt))
    check(_lib.load().icka_bn_apply(raw.data_ptr(), scale.data_ptr(), shift.data_ptr(), _ptr(residual), _ptr(res_scale),
                                    _ptr(res_shift), out.data_ptr(), raw.shape[1], rows_valid, raw.shape[0], int(bool(relu)),
                                    p[0], p[1], _stream()), "icka_bn_apply")
    return out
