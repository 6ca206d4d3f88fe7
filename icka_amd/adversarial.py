"""Adversarial training on the word embeddings: FGM and FreeLB as a per-token perturbation.

    adv = icka_amd.Adversary(model, epsilon=1.0, recipe="fgm")                                              # or
    adv = icka_amd.Adversary(model, epsilon=1.0, recipe="freelb", steps=3, alpha=0.3, init="uniform", seed=0)

    def step_fn(ids, seg, mask, added, vmean, vatt, labels):       # GraphedStep / TrainStep contract: forward + backward inside
        return adv.run(lambda: model(ids, seg, mask, added, vmean, vatt, labels=labels) / k, input_mask=mask)

The textbook form perturbs the embedding WEIGHT, backs it up and restores it.  Here the table is a view of the arena's flat f32
buffer that the captured optimizer and the averaging launches own, so the perturbation is a tensor of its own: ``delta``
f32 [B, S, H], one row per token position, added to the word row inside the embedding kernel (``icka_embed_fwd_adv``; the
definitions are in include/icka_hip.h).  The gradient with respect to it is the per-token row ``icka_embed_bwd_rows`` leaves;
``icka_adv_ascend`` turns it into the next perturbation on the device (per-sample norm over the valid positions, step,
projection onto the epsilon-ball, zeros at the non-valid positions).  Nothing here synchronises the host or reads a value
back, so a whole recipe -- clean pass, ascent, adversarial pass -- is legal inside one stream capture.

Recipes (``run(closure, input_mask)``; ``closure`` runs the forward and returns the loss, ``run`` calls ``backward()``):
  * ``"fgm"`` (Miyato et al. 2017): a clean pass (no perturbation; its gradient rows are recorded), ONE ascent from
    delta = 0 with alpha = epsilon -- delta_b = epsilon g_b / ||g_b|| -- and one perturbed pass whose parameter gradients
    accumulate onto the clean ones.  Returns the clean loss.
  * ``"freelb"`` (Zhu et al. 2020): delta_0 = 0 or uniform (``init``), then ``steps`` perturbed passes of
    ``(closure() / steps).backward()`` with an ascent of size ``alpha`` between consecutive passes (steps - 1 ascents); the
    parameter gradients of all passes accumulate.  Returns the sum of the scaled losses.
Other schedules are built from ``clean()`` / ``perturbed()`` (contexts that open a pass), ``ascend``, ``init_uniform``,
``reset`` and the read-only views ``delta`` / ``grad`` / ``norms``.

Inside a pass ``BertEmbeddings.forward`` routes through ``ops.EmbeddingsAdvFn``; outside, the code path is the plain one (the
only new work is one attribute read).  While a pass is open on its model a ``GraphedModule`` call takes its eager route (its
captured forwards hold no perturbation), the rule ``attention_maps`` follows.

Limits, each refused with NotImplementedError on construction or on pass entry: the fp32-exact precision mode; a packed model
(``set_packed``); an arena with a ``GradReducer`` attached (its sparse-row branch owns the per-token rows); hidden sizes
outside ``H % 8 == 0, H <= 2048``; more than 1024 positions.  Token ids must lie inside the table (the row scatter skips ids
outside it, where the plain backward clamps them).  Out of scope: Madry-style PGD (its intermediate passes discard their
parameter gradients), perturbing the region features or the prompt embeddings (``PromptRobertaEmbeddings`` is not a target),
virtual adversarial (KL) losses (``CRF.kl_divergence`` and the building blocks allow them by hand), data parallel, packed
batches.  One pass at a time per embeddings module; the state is not thread-safe.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch

from . import kernels as K

_open = []      # the adversaries with an open pass (GraphedModule asks ``pass_open``)


def pass_open(model) -> bool:
    """Is an adversarial pass open on an embeddings module under ``model``?  (One list test when none is.)"""
    if not _open:
        return False
    mods = None
    for adv in _open:
        if adv.model is model:
            return True
        if mods is None:
            mods = {id(m) for m in model.modules()}
        if id(adv.embeddings) in mods:
            return True
    return False


class _Pass(object):
    def __init__(self, adv, perturbed: bool):
        self.adv, self.perturbed_ = adv, perturbed

    def __enter__(self):
        self.adv._enter(self.perturbed_)
        return self.adv

    def __exit__(self, *exc):
        self.adv._exit()
        return False


class Adversary(object):
    """Module docstring.  ``embeddings``: the ``modeling.BertEmbeddings`` to perturb; None = the single one under ``model``
    (none or several: ValueError).  ``alpha``: ascent step size (default: epsilon for "fgm", epsilon / steps for "freelb")."""

    def __init__(self, model, embeddings=None, *, epsilon: float = 1.0, recipe: str = "fgm", steps: Optional[int] = None,
                 alpha: Optional[float] = None, init: str = "zero", seed: int = 0):
        from .modeling import BertEmbeddings
        if recipe not in ("fgm", "freelb"):
            raise ValueError('recipe must be "fgm" or "freelb", got %r' % (recipe,))
        if init not in ("zero", "uniform"):
            raise ValueError('init must be "zero" or "uniform", got %r' % (init,))
        if not epsilon > 0:
            raise ValueError("epsilon must be positive")
        if embeddings is None:
            found = [m for m in model.modules() if isinstance(m, BertEmbeddings)]
            if len(found) != 1:
                raise ValueError("Adversary: %d BertEmbeddings under the model; name the one to perturb with embeddings="
                                 % len(found))
            embeddings = found[0]
        elif not isinstance(embeddings, BertEmbeddings):
            raise TypeError("embeddings must be a modeling.BertEmbeddings (PromptRobertaEmbeddings is not a target), got %s"
                            % type(embeddings).__name__)
        self.model, self.embeddings = model, embeddings
        self.epsilon, self.recipe, self.init, self.seed = float(epsilon), recipe, init, int(seed)
        self.steps = 1 if recipe == "fgm" else int(3 if steps is None else steps)
        if self.steps < 1:
            raise ValueError("steps must be >= 1")
        if recipe == "fgm" and steps not in (None, 1):
            raise ValueError("fgm is one ascent step; use recipe='freelb' for more")
        self.alpha = float(alpha) if alpha is not None else (self.epsilon if recipe == "fgm" else self.epsilon / self.steps)
        self.H = int(embeddings.word_embeddings.weight.shape[1])
        if self.H % 8 or self.H > K.ADV_MAX_H:
            raise NotImplementedError("Adversary: hidden size %d is outside the kernel limits (H %% 8 == 0, H <= %d)"
                                      % (self.H, K.ADV_MAX_H))
        self._refuse_modes()
        self._bufs: Dict[Tuple[int, int], dict] = {}
        self._cur = None            # the buffers of the shape last initialised / ascended / passed
        self._counter = None        # device int64: uniform starts drawn so far (advanced by a launch: fresh per replay)
        self._mode = None           # None | "clean" | "perturbed"
        self._ids_shape = None      # [B, S] of the ids of the last pass

    # ---- refusals
    def _refuse_modes(self) -> None:
        from .modeling import _is_exact
        from .packing import state_of
        if _is_exact(self.embeddings):
            raise NotImplementedError("Adversary: the fp32-exact precision mode is not supported (bf16 and mixed16 are)")
        if state_of(self.model) is not None:
            raise NotImplementedError("Adversary: a packed model (set_packed) is not supported: its token rows are packed rows; "
                                      "call set_packed(model, None) first")
        arena = getattr(self.model, "_icka_arena", None)
        if arena is not None and arena.reducer is not None:
            raise NotImplementedError("Adversary: this model's arena has a GradReducer attached (its sparse-row exchange owns "
                                      "the per-token gradient rows); data parallel is out of scope")

    def check_pass(self, emb, arena, B: int, S: int) -> None:
        """Called by ``BertEmbeddings.forward`` inside a pass, before any launch."""
        if arena.reducer is not None:
            raise NotImplementedError("Adversary: this model's arena has a GradReducer attached; data parallel is out of scope")
        if S > K.ADV_MAX_S:
            raise NotImplementedError("Adversary: %d positions are outside the kernel limits (S <= %d)" % (S, K.ADV_MAX_S))

    # ---- buffers
    def _buffers(self, B: int, S: int) -> dict:
        b = self._bufs.get((B, S))
        if b is None:
            if S > K.ADV_MAX_S:
                raise NotImplementedError("Adversary: %d positions are outside the kernel limits (S <= %d)" % (S, K.ADV_MAX_S))
            dev = self.embeddings.word_embeddings.weight.device
            if dev.type != "cuda":
                raise TypeError("Adversary: the model must be on a ROCm device (icka_amd has no CPU path)")
            f32 = dict(dtype=torch.float32, device=dev)
            b = self._bufs[(B, S)] = {"delta": torch.zeros(B, S, self.H, **f32), "grad": torch.zeros(B, S, self.H, **f32),
                                      "norms": torch.zeros(B, 2, **f32),
                                      "ws": torch.zeros(K.adv_workspace_floats(B, S, self.H), **f32)}
        return b

    def _mask(self, input_mask) -> dict:
        if not torch.is_tensor(input_mask) or input_mask.dim() != 2:
            raise ValueError("input_mask must be an int64 [B, S] tensor")
        if input_mask.dtype != torch.int64:
            raise TypeError("input_mask must be int64 (as everywhere), got %s" % input_mask.dtype)
        B, S = input_mask.shape
        self._cur = self._buffers(B, S)
        return self._cur

    def pass_delta(self, B: int, S: int):
        """The perturbation of the open pass for ids of shape [B, S]: None in a clean pass."""
        self._ids_shape = (B, S)
        if self._mode != "perturbed":
            self._cur = self._buffers(B, S)
            return None
        if self._cur is None or tuple(self._cur["delta"].shape[:2]) != (B, S):
            raise ValueError("Adversary: the perturbation was prepared for an input_mask of shape %s, the ids of this pass are %s"
                             % (None if self._cur is None else tuple(self._cur["delta"].shape[:2]), (B, S)))
        return self._cur["delta"]

    def pass_grad(self, B: int, S: int) -> torch.Tensor:
        return self._buffers(B, S)["grad"]

    # ---- read-only views
    @property
    def delta(self):
        return None if self._cur is None else self._cur["delta"]

    @property
    def grad(self):
        return None if self._cur is None else self._cur["grad"]

    @property
    def norms(self):
        """f32 [B, 2] of the last ascent: (||g_b||, ||delta_b|| after the step)."""
        return None if self._cur is None else self._cur["norms"]

    # ---- passes
    def _enter(self, perturbed: bool) -> None:
        if self._mode is not None or self.embeddings._icka_adv is not None:
            raise RuntimeError("Adversary: a pass is already open on this embeddings module")
        self._refuse_modes()
        self._mode = "perturbed" if perturbed else "clean"
        self.embeddings._icka_adv = self
        _open.append(self)

    def _exit(self) -> None:
        self.embeddings._icka_adv = None
        self._mode = None
        _open.remove(self)

    def clean(self):
        """Context: forwards inside run without perturbation; their backward records ``grad``."""
        return _Pass(self, False)

    def perturbed(self):
        """Context: forwards inside add ``delta``; their backward records ``grad``."""
        return _Pass(self, True)

    # ---- the perturbation
    def reset(self, input_mask=None) -> None:
        """delta = 0 (of the shape of ``input_mask``; None: of the current shape)."""
        b = self._cur if input_mask is None else self._mask(input_mask)
        if b is not None:
            K.zero_(b["delta"].view(-1))

    def init_uniform(self, input_mask) -> None:
        """The uniform start of FreeLB (icka_hip.h: icka_adv_init_uniform), then the launch that advances the draw counter."""
        b = self._mask(input_mask)
        if self._counter is None:
            self._counter = torch.zeros(1, dtype=torch.int64, device=b["delta"].device)
        mask = input_mask if input_mask.is_contiguous() else input_mask.contiguous()
        K.adv_init_uniform(b["delta"], mask, epsilon=self.epsilon, seed=self.seed, counter=self._counter)
        K.adv_bump(self._counter)

    def ascend(self, input_mask, alpha: Optional[float] = None) -> None:
        """One ascent step from the gradient rows the last pass recorded (icka_hip.h: icka_adv_ascend)."""
        self._same_shape(input_mask)
        b = self._mask(input_mask)
        mask = input_mask if input_mask.is_contiguous() else input_mask.contiguous()
        K.adv_ascend(b["delta"], b["grad"], mask, b["norms"], b["ws"], alpha=self.alpha if alpha is None else alpha,
                     epsilon=self.epsilon)

    def _same_shape(self, input_mask) -> None:
        if self._ids_shape is not None and torch.is_tensor(input_mask) and tuple(input_mask.shape) != self._ids_shape:
            raise ValueError("Adversary: input_mask has shape %s, the ids of the last pass %s"
                             % (tuple(input_mask.shape), self._ids_shape))

    # ---- the recipes
    def run(self, closure: Callable[[], torch.Tensor], input_mask) -> torch.Tensor:
        if self.recipe == "fgm":
            with self.clean():
                loss = closure()
                loss.backward()
            self._same_shape(input_mask)
            self.reset(input_mask)
            self.ascend(input_mask)
            with self.perturbed():
                closure().backward()
            return loss
        if self.init == "uniform":
            self.init_uniform(input_mask)
        else:
            self.reset(input_mask)
        total = None
        for k in range(self.steps):
            with self.perturbed():
                loss = closure() / self.steps
                loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
            if k + 1 < self.steps:
                self.ascend(input_mask)
        return total
