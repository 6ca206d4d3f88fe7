"""Attention maps of a forward pass: the softmax probabilities the fused attention kernels never materialise.

    with icka_amd.attention_maps(model, heads="mean", select=None) as rec:   # heads: "mean" | "all"
        out = model(...)                  # any number of eager forward calls, eval or train mode, grad on or off
    rec.names                             # qualified names (model.named_modules()) of the recorded attention modules
    rec["txt2img_attention.layer.0.attention.self"]   # list, one f32 tensor per call: [B,Sq,Skv] or [B,heads,Sq,Skv]

The reference computes ``attention_probs`` in the open (BertSelfAttention.forward :478-506, BertCoAttention.forward :590-624); here
the forward keeps the row log-sum-exp only and the backward recomputes.  While a recorder is active on this thread,
``ops._attn_core_fwd`` -- the one place every attention of the 16-bit path goes through, the fused projection + attention launch
included -- follows its attention launch with ONE ``icka_attn_probs`` launch on the bf16 q / k it already holds (same additive
mask, same 1 / sqrt(d)) and appends the result to the recorder.

Definition: a map is ``softmax(q.k^T / sqrt(d) + mask)`` BEFORE dropout, in f32, from the bf16 q / k of the forward -- so train
mode is allowed and gives the same maps as eval mode; ``heads="mean"`` is the mean over heads, summed in head order inside the
kernel.  Nothing flows back through a map (they are made outside autograd and returned detached).  The forward itself is
untouched: outputs, saved tensors, dropout seeds and the launch sequence are those of a call without the recorder, plus the
probability launches.  With no recorder active the only new work is one thread-local read per attention call.

Limits (each refused with NotImplementedError):
  * head size 64 only (other head sizes take the generic f32 attention path) -- raised at the first recorded call;
  * the bf16 and mixed16 precision modes, not fp32 -- raised at the first recorded call;
  * at most 512 keys (``kernels.ATTN_PROBS_MAX_KEYS``, BERT's position limit);
  * not a packed model (``set_packed``) -- refused on entry;
  * eager calls only: ``GraphedModule`` / ``GraphedStep`` / ``TrainStep`` take their eager route while a recorder is active on
    the calling thread (no capture, no replay: the captured graphs hold no probability launch), and recording inside a stream
    capture raises.
A co-attention flagged ``fp8_scores`` is recorded, but its maps are the bf16 formulation above, NOT the fp8 QK^T its forward used.

The state is thread-local and re-entrant-safe like ``crf.device_decode()``: leaving a recorder restores the one that was active
before it; of nested recorders only the innermost records.
"""
from __future__ import annotations

import threading
from typing import Callable, Dict, Iterable, List, Optional, Union

import torch

from .kernels import ATTN_PROBS_MAX_KEYS as _MAX_KEYS

_state = threading.local()


def current():
    """The recorder active on this thread, or None (the one read ``ops._attn_core_fwd`` pays when nothing records)."""
    return getattr(_state, "rec", None)


def active() -> bool:
    return getattr(_state, "rec", None) is not None


class attention_maps(object):
    """Context manager and recorder (module docstring).  ``select``: None = every BertSelfAttention / BertCoAttention under
    ``model``; an iterable of qualified names (an unknown one raises KeyError on entry); or a predicate on the name."""

    def __init__(self, model, heads: str = "mean", select: Union[None, Iterable[str], Callable[[str], bool]] = None):
        if heads not in ("mean", "all"):
            raise ValueError('heads must be "mean" or "all", got %r' % (heads,))
        self.model = model
        self.heads = heads
        self._select = select
        self._by_module: Dict[int, str] = {}
        self._maps: Dict[str, List[torch.Tensor]] = {}
        self._prev = None
        self._entered = False

    # ---- the module -> name table, built on entry
    def _table(self) -> None:
        from .modeling import BertSelfAttention      # (BertCoAttention is a subclass)
        for m in self.model.modules():
            if getattr(m, "_icka_packed", None) is not None:
                raise NotImplementedError("attention_maps does not record a packed model (set_packed): its queries sit at "
                                          "packed rows; call set_packed(model, None) first")
        found = [(n, m) for n, m in self.model.named_modules() if isinstance(m, BertSelfAttention)]
        sel = self._select
        if sel is None:
            keep = found
        elif callable(sel):
            keep = [(n, m) for n, m in found if sel(n)]
        else:
            want = [sel] if isinstance(sel, str) else list(sel)
            known = dict(found)
            for n in want:
                if n not in known:
                    raise KeyError("attention_maps: %r names no BertSelfAttention / BertCoAttention under the model (known: %s)"
                                   % (n, ", ".join(sorted(known)) or "none"))
            keep = [(n, m) for n, m in found if n in set(want)]
        self._by_module = {id(m): n for n, m in keep}
        self._modules = [m for _n, m in keep]         # keeps the ids above alive and unique
        self._maps = {n: [] for n, _m in keep}

    def __enter__(self):
        if self._entered:
            raise RuntimeError("this attention_maps recorder is already active")
        self._table()
        self._prev = getattr(_state, "rec", None)
        _state.rec = self
        self._entered = True
        return self

    def __exit__(self, *exc):
        _state.rec = self._prev
        self._prev = None
        self._entered = False
        return False

    # ---- results
    @property
    def names(self) -> List[str]:
        return list(self._maps)

    def __getitem__(self, name: str) -> List[torch.Tensor]:
        return self._maps[name]

    def __contains__(self, name: str) -> bool:
        return name in self._maps

    def __len__(self) -> int:
        return len(self._maps)

    def items(self):
        return self._maps.items()

    # ---- called by the attention cores
    def wants(self, sa, head_size: int, Skv: int) -> Optional[str]:
        """Name under which ``sa``'s call is recorded, or None when it is not selected.  Called BEFORE the attention core
        launches anything, so that a refusal leaves no half-made forward."""
        name = self._by_module.get(id(sa))
        if name is None:
            return None
        if head_size != 64:
            raise NotImplementedError("attention_maps: %s has head size %d; the probability kernel is built for head size 64 "
                                      "(other head sizes run the generic f32 attention path)" % (name, head_size))
        if Skv > _MAX_KEYS:
            raise NotImplementedError("attention_maps: %s attends over %d keys; the probability kernel takes up to %d"
                                      % (name, Skv, _MAX_KEYS))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attention_maps records eager calls only: %s was called inside a stream capture" % name)
        return name

    def refuse_fp32(self, sa) -> None:
        name = self._by_module.get(id(sa))
        if name is not None:
            raise NotImplementedError("attention_maps: %s runs in the fp32 precision mode; maps are recorded in the bf16 and "
                                      "mixed16 modes only (set_precision)" % name)

    def record(self, name: str, q, k, add_mask, B: int, heads: int, Sq: int, Skv: int) -> None:
        from . import kernels as K
        P = K.attn_probs(q, k, add_mask, B, heads, Sq, Skv, head_mean=self.heads == "mean")
        self._maps[name].append(P.detach())
