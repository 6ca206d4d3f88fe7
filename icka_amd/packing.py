"""Padding-free ("packed") token-budget batches for the MNER tagger.

``set_packed(model, max_tokens)`` switches a ``MTCCMBertForMMTokenClassificationCRF(variant="cl")`` to packed execution: the
embeddings still run on the padded ``[B, S]`` batch, then the valid tokens of every sample are gathered into ``max_tokens``
rows (sample b in rows ``[cu[b], cu[b+1])``, the rest are filler rows), the text encoder, the cross encoder and the gated head
run on those rows, and the logits are scattered back to ``[B, S, C]`` (exactly 0 at pad positions).  Every shape depends on
``max_tokens`` only, so one graph capture serves every batch; ``TokenBudgetBatchSampler`` picks batches that fill the budget.

A batch whose valid tokens exceed ``max_tokens`` is never written past the buffers: the samples that do not fit are left out
of the row maps, their logits (and so the loss) are NaN, and the plan kernel sets the model's host-mapped error word.  The
next ``forward`` (or the pre-replay check of a graphed step) raises ``PackOverflowError`` with the token count.
"""
from __future__ import annotations

import random
from typing import Iterator, List, Optional, Sequence

import torch

F32_NAN_WORD = 0x7FC00000


class PackOverflowError(RuntimeError):
    """A packed batch held more valid tokens than ``max_tokens`` (or a mask that is not a prefix mask)."""


class TokenBudgetBatchSampler(object):
    """Batches of sample indices whose summed ``lengths`` never exceed ``max_tokens`` (and at most ``max_batch`` samples):
    the ``batch_sampler`` of a ``torch.utils.data.DataLoader`` feeding a model under ``set_packed(model, max_tokens)``.

    Indices are taken in order (a seeded shuffle per epoch when ``shuffle``; ``set_epoch`` changes the order) and a batch is
    closed when the next sample would not fit.  ``drop_last`` drops the final batch when it is not full (it could still take
    the next sample of a longer epoch: fewer than ``max_batch`` samples and room for the shortest one).  A sample longer
    than ``max_tokens`` raises."""

    def __init__(self, lengths: Sequence[int], max_tokens: int, max_batch: int = 256, shuffle: bool = False, seed: int = 0,
                 drop_last: bool = False):
        lengths = [int(n) for n in lengths]
        if max_tokens <= 0 or max_batch <= 0:
            raise ValueError("max_tokens and max_batch must be positive")
        for i, n in enumerate(lengths):
            if n < 0:
                raise ValueError("lengths[%d] = %d is negative" % (i, n))
            if n > max_tokens:
                raise ValueError("sample %d has %d tokens, more than max_tokens=%d" % (i, n, max_tokens))
        self.lengths, self.max_tokens, self.max_batch = lengths, int(max_tokens), int(max_batch)
        self.shuffle, self.seed, self.drop_last, self.epoch = bool(shuffle), int(seed), bool(drop_last), 0
        self._min_len = min(lengths) if lengths else 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _order(self) -> List[int]:
        order = list(range(len(self.lengths)))
        if self.shuffle:
            random.Random(self.seed * 1000003 + self.epoch).shuffle(order)
        return order

    def __iter__(self) -> Iterator[List[int]]:
        batch, tokens = [], 0
        for i in self._order():
            n = self.lengths[i]
            if batch and (tokens + n > self.max_tokens or len(batch) == self.max_batch):
                yield batch
                batch, tokens = [], 0
            batch.append(i)
            tokens += n
        if batch:
            full = len(batch) == self.max_batch or tokens + self._min_len > self.max_tokens
            if full or not self.drop_last:
                yield batch

    def __len__(self) -> int:
        return sum(1 for _ in self)


def check_max_tokens(max_tokens) -> int:
    if isinstance(max_tokens, bool) or not isinstance(max_tokens, int):
        raise TypeError("max_tokens must be an int (a positive multiple of 128) or None, got %r" % (max_tokens,))
    if max_tokens <= 0 or max_tokens % 128:
        raise ValueError("max_tokens must be a positive multiple of 128, got %d" % max_tokens)
    return max_tokens


def plan_reference(input_mask: torch.Tensor, max_tokens: int):
    """CPU restatement of the plan kernel (icka_pack_plan): dict of lens [B], cu_seqlens [B+1], packed_to_padded
    [max_tokens], padded_to_packed [B*S], cls_of [max_tokens] (int32) and status (total tokens, flags)."""
    m = input_mask.detach().to("cpu", torch.int64) != 0
    B, S = m.shape
    first_zero = torch.where(~m, torch.arange(S).expand(B, S), torch.full((B, S), S)).min(dim=1).values
    lens = first_zero.to(torch.int32)
    nonprefix = bool((m.sum(dim=1) != first_zero).any())
    cu = torch.zeros(B + 1, dtype=torch.int32)
    kept, dropping = 0, False
    for b in range(B):
        cu[b] = kept
        n = int(lens[b])
        if not dropping and kept + n <= max_tokens:
            kept += n
        else:
            dropping = True
    cu[B] = kept
    p2p = torch.full((max_tokens,), -1, dtype=torch.int32)
    pad2pack = torch.where(m.reshape(-1), torch.tensor(-2, dtype=torch.int32), torch.tensor(-1, dtype=torch.int32))
    cls_of = torch.full((max_tokens,), -1, dtype=torch.int32)
    for b in range(B):
        c0, n = int(cu[b]), int(cu[b + 1]) - int(cu[b])
        if n:
            p2p[c0:c0 + n] = b * S + torch.arange(n, dtype=torch.int32)
            pad2pack[b * S:b * S + n] = c0 + torch.arange(n, dtype=torch.int32)
            cls_of[c0] = b
    total = int(lens.sum())
    flags = (1 if total > max_tokens else 0) | (2 if nonprefix else 0)
    return {"lens": lens, "cu_seqlens": cu, "packed_to_padded": p2p, "padded_to_packed": pad2pack, "cls_of": cls_of,
            "status": torch.tensor([total, flags], dtype=torch.int32)}


class Plan(object):
    """Device row maps of one packed forward (icka_pack_plan), handed to the kernels through ops.Dims.pack."""
    __slots__ = ("B", "S", "max_tokens", "lens", "cu", "p2p", "pad2pack", "cls_of", "status")

    def __init__(self, B, S, max_tokens, device):
        i32 = torch.int32
        self.B, self.S, self.max_tokens = B, S, max_tokens
        self.lens = torch.empty(B, dtype=i32, device=device)
        self.cu = torch.empty(B + 1, dtype=i32, device=device)
        self.p2p = torch.empty(max_tokens, dtype=i32, device=device)
        self.pad2pack = torch.empty(B * S, dtype=i32, device=device)
        self.cls_of = torch.empty(max_tokens, dtype=i32, device=device)
        self.status = torch.empty(2, dtype=i32, device=device)


class PackState(object):
    """Per-model packed configuration and its host-mapped error word (one per model)."""

    def __init__(self, max_tokens: int):
        self.max_tokens = max_tokens
        self._err = None        # pinned int32[2]: {tokens, flags}, written by the plan kernel with a system-scope store
        self._err_np = None

    def err_word(self) -> int:
        # first packed forward: eager (a capture's warm-up runs eagerly first).  A word that is not (or no longer) pinned host
        # memory is never handed to the device: it is made again
        if self._err is None or not self._err.is_pinned():
            self._err = torch.zeros(2, dtype=torch.int32).pin_memory()
            self._err_np = self._err.numpy()
        return self._err.data_ptr()

    # A copy of the model (copy.deepcopy, torch.save / torch.load) must not carry the word: a copied storage is ordinary
    # pageable memory and its numpy view no longer aliases it.  The copy makes its own pinned word at its first forward.
    def __getstate__(self):
        d = dict(self.__dict__)
        d["_err"] = d["_err_np"] = None
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def __deepcopy__(self, memo):
        c = PackState.__new__(PackState)
        c.__setstate__(self.__getstate__())
        memo[id(self)] = c
        return c

    def check_error(self, where: str = "") -> None:
        e = self._err_np
        if e is not None and e[1] != 0:
            tokens, flags = int(e[0]), int(e[1])
            e[0] = e[1] = 0
            what = []
            if flags & 1:
                what.append("%d valid tokens in a batch for max_tokens=%d" % (tokens, self.max_tokens))
            if flags & 2:
                what.append("an input_mask that is not a prefix mask (pos < len)")
            raise PackOverflowError("icka_amd packed batch%s: %s; the samples that did not fit were left out and that batch's "
                                    "logits and loss are NaN.  Pick batches with TokenBudgetBatchSampler(max_tokens=%d)."
                                    % ((" (" + where + ")") if where else "", " and ".join(what), self.max_tokens))

    def plan(self, input_mask: torch.Tensor) -> Plan:
        from . import kernels as K
        B, S = input_mask.shape
        mask = input_mask if input_mask.dtype == torch.int64 else input_mask.long()
        p = Plan(B, S, self.max_tokens, input_mask.device)
        K.pack_plan(mask.contiguous(), self.max_tokens, p, err_word=self.err_word())
        return p


def state_of(model) -> Optional[PackState]:
    return getattr(model, "_icka_packed", None)


def _unsupported(model) -> Optional[str]:
    from .modeling import MTCCMBertForMMTokenClassificationCRF, resolved_precision
    if type(model) is not MTCCMBertForMMTokenClassificationCRF:
        return ("packed batches are built for MTCCMBertForMMTokenClassificationCRF(variant='cl') only, not %s"
                % type(model).__name__)
    from .modeling import BertModel
    if not isinstance(model.bert, BertModel):
        return "packed batches need the model's own BertModel text encoder"
    if model.variant != "cl":
        return ("packed batches do not support variant='gate_cl': its crs_classifier reads the pad rows through "
                "cat(seq, cross).view(B, -1), so packing would change its result")
    prec = resolved_precision(model)
    if prec != "bf16":
        return "packed batches run in the bf16 precision mode only, not %s" % prec
    cfg = model.config
    if cfg.hidden_size // cfg.num_attention_heads != 64 or cfg.hidden_size % cfg.num_attention_heads:
        return "packed batches need head size 64, got %d" % (cfg.hidden_size // cfg.num_attention_heads)
    for layer in model.txt2img_attention.layer:
        if getattr(layer.attention.self, "fp8_scores", False):
            return "packed batches do not support the fp8 cross-attention (cross_attention_fp8=True)"
    return None


def validate(model, S: int) -> None:
    """Raise NotImplementedError for a model / mode / length the packed path does not take."""
    why = _unsupported(model)
    if why is None and S > 128:
        why = "packed batches take sequences of up to 128 tokens, got S=%d (the <4,16> attention instance of longer heads " \
              "is at the 512-register cap)" % S
    if why is not None:
        raise NotImplementedError(why)


def set_packed(model, max_tokens):
    """Switch ``model`` to packed token-budget batches of ``max_tokens`` rows (a positive multiple of 128), or back to the
    padded path with ``None``.  ``forward`` keeps the reference's signature and returns padded outputs.

    Empty samples (an all-zero ``input_mask``) occupy no packed row.  They are neutral only for the token-CE loss: the CRF
    (``use_crf``) scores position 0 of every sample and divides by B, and ``aux_losses`` takes every sample into the contrastive
    loss (an empty sample's pooler input is a zero row here, the encoder output at its position 0 in the padded path).  So
    bring batches to a fixed B with empty samples only under token-CE; with the CRF or ``aux_losses``, feed full batches."""
    if max_tokens is None:
        if hasattr(model, "_icka_packed"):
            del model._icka_packed
        return model
    max_tokens = check_max_tokens(max_tokens)
    why = _unsupported(model)
    if why is not None:
        raise NotImplementedError(why)
    model._icka_packed = PackState(max_tokens)
    return model


def refuse(model, what: str) -> None:
    """The data-parallel step forms do not take packed models (multi-GPU packing is out of scope)."""
    if model is not None and state_of(model) is not None:
        raise NotImplementedError("%s does not support packed models (set_packed): packed batches run on one GPU" % what)


def check_error(model, where: str = "") -> None:
    st = state_of(model)
    if st is not None:
        st.check_error(where)


class RowsGatherFn(torch.autograd.Function):
    """y = rows of x through ``fwd_map`` (icka_rows_gather); the backward gathers dy through ``bwd_map``, the inverse map.
    Both directions write every destination row (zeros where the map has no source row)."""

    @staticmethod
    def forward(ctx, x, fwd_map, fwd_stride: int, out_rows: int, bwd_map, bwd_stride: int, fill: int = 0):
        from . import kernels as K
        y = torch.empty(out_rows, x.shape[1], dtype=x.dtype, device=x.device)
        K.rows_gather(x, y, fwd_map, fwd_stride, fill)
        ctx.in_rows, ctx.bwd_stride = x.shape[0], bwd_stride
        ctx.save_for_backward(bwd_map)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import kernels as K
        bwd_map, = ctx.saved_tensors
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = torch.empty(ctx.in_rows, dy.shape[1], dtype=dy.dtype, device=dy.device)
        K.rows_gather(dy, dx, bwd_map, ctx.bwd_stride, 0)
        return dx, None, None, None, None, None, None
