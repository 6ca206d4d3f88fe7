"""Sharpness-aware minimisation on the parameter arena: SAM (Foret et al. 2021) and its scale-invariant form ASAM (Kwon et al.
2021).

    sam = icka_amd.SAM(model, optimizer, rho=0.05, adaptive=False)      # optimizer: an ArenaAdamW of model, either mode

    def step_fn(*batch):                                                # GraphedStep / TrainStep contract
        return sam.run(lambda: model(*batch[:-1], labels=batch[-1]))

    ts = TrainStep(model, step_fn, optimizer, inputs=first_batch)       # clean pass, ascent, second pass, restore, update: ONE graph

or, by hand: ``model.zero_grad(); loss = sam.run(closure); optimizer.step()``.

A step takes the gradient at w, climbs to w + e(w), takes the gradient there and lets the optimizer update w with that second
gradient.  The reference trains without it.  A stock wrapper walks ~220 parameter tensors twice with host-side norms; here
parameters, gradients and the 16-bit shadows share the arena's flat layout, so the ascent is three launches (include/icka_hip.h:
icka_sam_sqnorm, icka_sam_prepare, icka_sam_ascend) over the optimizer's own chunk table and the way back is one
(icka_sam_restore).  The norm, the step scale and the skip word stay in a device block (icka_sam_state): nothing here reads a
value back, so the whole sequence is legal inside one stream capture.

  * plain:     e = rho g / ||g||
  * adaptive:  e = rho p^2 g / || |p| g ||   -- over every perturbed element, biases included (the common formula; rho ~ 10x
               the plain one, Kwon et al. use 0.5 .. 2)
What is perturbed is exactly what the optimizer would update: the parameters of its groups that hold a gradient after the first
pass.  ``ascend()`` writes ``backup = p`` before it moves p and the 16-bit shadows; ``restore()`` copies the backup over p and
re-derives the shadows.  Restoring from a copy, not subtracting e, is deliberate: the weights after a step are bitwise what the
optimizer left, ``TrainStep``'s dry warm-up leaves no trace, and a NaN that reached the perturbation cannot survive it.  The
cost is one more f32 buffer of the arena's layout, as ``ArenaAdamW(average=)`` costs.  An ascent whose gradient norm is zero, inf
or NaN is refused ON THE DEVICE (``skipped_ascents()``): both launches return at once, the second pass runs at w, and the
optimizer's own non-finite guard then sees that gradient.  While ``optimizer._dry`` is set (``TrainStep``'s warm-up) the prepare
launch only sets the skip word and counts nothing.

``run(closure)``: ``loss = closure(); loss.backward()``; norm, prepare, ascend; the gradient slots are marked not live, so the
second backward's stores overwrite them; ``closure().backward()``; restore; returns the first (clean) loss.  Afterwards
``p.grad`` / ``gflat`` hold the gradient of the second pass alone, weights and shadows are bitwise those from before, and
``optimizer.step()`` -- or ``TrainStep``'s captured one -- runs unchanged, its clip and non-finite guard included.  The two
passes draw their own dropout masks, as the adversarial passes do.  ``ascend()`` / ``restore()`` / ``perturbed()`` are the
building blocks for other schedules; ``grad_norm()`` is a device scalar; ``ascents()`` / ``skipped_ascents()`` are the only calls
that synchronise.  Every precision mode (the fp32-exact one included) and packed models work: only the flat buffers are touched,
and a shadow the arena does not have is passed as NULL.  Nothing is checkpointed: the state is two diagnostic counters.

The chunk tables are the optimizer's (``ArenaAdamW._build``), with its capture rules: the first eager call, or the ``TrainStep``
warm-up, builds them; a changed gradient set inside a capture raises, as ``step()`` does.

Refused, each with its reason: ``rho <= 0``; an optimizer that is not an ``ArenaAdamW`` of this model; a ``GradReducer`` on the
arena (under data parallel it is undecided whether the norm is taken per rank or over the summed gradient: out of scope);
``run`` while ``optimizer.averaged_weights()`` is active; ``optimizer.step()`` / ``averaged_weights()`` while a perturbation is
in place; a nested ``run``; ``run`` when a gradient slot is already live (the first pass would add this batch to an earlier
micro-batch's sum, and the perturbation must come from this batch alone) and, for the same reason, ``TrainStep(accumulate > 1)``
for a model with a registered ``SAM``.

Out of scope: composing with ``Adversary`` inside one closure; parameters whose consumers keep a derived copy outside the arena
-- the image encoder's GEMM-layout convolution weights (``icka_amd.resnet``): keep them out of the groups, the rule
``ArenaAdamW.averaged_weights()`` documents; a ``rho`` schedule; m-sharpness; folding the restore into icka_optim_adamw_dev (it
would save one pass over the arena and change an existing entry point: to be decided from the profile).
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Callable

import torch

from . import _lib
from . import kernels as K
from .arena import ParamArena
from .optim import ArenaAdamW

_registry = weakref.WeakSet()      # every SAM alive (train_step.TrainStep asks ``registered``)


def registered(model) -> bool:
    """Does a ``SAM`` exist for ``model``?  (One empty-set test when none does.)"""
    if not _registry:
        return False
    return any(s.model is model for s in _registry)


class SAM(object):
    """Module docstring.  ``optimizer``: the ``ArenaAdamW`` (host or capturable mode) that updates ``model``; ``rho``: the radius
    of the ascent; ``adaptive``: ASAM's element-wise scaling by |p|."""

    def __init__(self, model: torch.nn.Module, optimizer, rho: float = 0.05, adaptive: bool = False):
        if not float(rho) > 0.0:
            raise ValueError("SAM(rho=): the ascent radius must be positive, got %r (rho = 0 is the plain step: use the "
                             "optimizer alone)" % (rho,))
        if not isinstance(optimizer, ArenaAdamW):
            raise TypeError("SAM: the ascent walks the optimizer's chunk tables over the parameter arena; it needs an "
                            "optim.ArenaAdamW, got %s" % type(optimizer).__name__)
        if optimizer.model is not model:
            raise ValueError("SAM: the optimizer belongs to another model (its tables describe that model's arena)")
        self.model, self.optimizer = model, optimizer
        self.rho, self.adaptive = float(rho), bool(adaptive)
        self._arena = None          # the arena the buffers below belong to
        self._backup = None         # f32 buffer of the arena's layout: the weights while they are perturbed
        self._state = None          # the icka_sam_state block
        self._table = None          # the chunk table of the perturbation in place (restore walks what ascend walked)
        self._running = False
        self._refuse_reducer(getattr(model, "_icka_arena", None))
        _registry.add(self)

    # ---- refusals
    @staticmethod
    def _refuse_reducer(arena) -> None:
        if arena is not None and arena.reducer is not None:
            raise NotImplementedError("SAM: this model's arena has a GradReducer attached; under data parallel it is undecided "
                                      "whether the norm is taken per rank or over the summed gradient: out of scope")

    def _bind(self) -> ParamArena:
        A = self.optimizer._bind()
        self._refuse_reducer(A)
        if A is not self._arena:
            if self.optimizer._perturbed:
                raise RuntimeError("SAM: the model's parameter arena was rebuilt while a perturbation was in place")
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SAM: the first ascent allocates the backup buffer; run one eager step (TrainStep's warm-up "
                                   "does) before capturing")
            self._arena = A
            self._backup = torch.zeros(A.total, dtype=torch.float32, device=A.device)
            self._state = K.sam_state_new(A.device)
        return A

    # ---- the building blocks
    @torch.no_grad()
    def ascend(self) -> None:
        """From the gradients held now: norm, step scale, and ``p <- p + e`` with the 16-bit shadows (module docstring)."""
        opt = self.optimizer
        if opt._perturbed:
            raise RuntimeError("SAM.ascend: a perturbation is already in place (restore() first)")
        if opt._swapped:
            raise RuntimeError("SAM.ascend: the optimizer's averaged weights are swapped in (averaged_weights() is active); the "
                               "ascent would perturb the average")
        A = self._bind()
        if A.pending_wgrad or A.pending_reductions:
            raise AssertionError("SAM.ascend: %d weight-gradient GEMMs and %d slab reductions of the arena are still queued; the "
                                 "norm would be taken over gradients that are not written yet"
                                 % (len(A.pending_wgrad), len(A.pending_reductions)))
        opt._build(A)               # the optimizer's tables for the gradients held now (raises inside a capture if they changed)
        table = opt._norm_table
        if table.shape[0] == 0:
            return
        K.sam_sqnorm(A.flat, A.gflat, table, opt._partials, self.adaptive)
        K.sam_prepare(opt._partials, table.shape[0], self.rho, self._state, dry=opt._dry)
        K.sam_ascend(A.flat, A.gflat, self._backup, A.shadow, A.shadow16, table, self._state, self.adaptive)
        self._table = table
        opt._perturbed = True

    @torch.no_grad()
    def restore(self) -> None:
        """``p <- backup`` with the 16-bit shadows: bitwise what ``ascend()`` found.  Without a perturbation in place: nothing."""
        if not self.optimizer._perturbed or self._table is None:
            return
        A = self._arena
        K.sam_restore(A.flat, self._backup, A.shadow, A.shadow16, self._table, self._state)
        self._table = None
        self.optimizer._perturbed = False

    @contextlib.contextmanager
    def perturbed(self):
        """Context: ``ascend()`` on entry, ``restore()`` on exit -- also after an exception.  Inside, the model, its
        ``state_dict()`` and its shadows are at w + e(w).  The gradients are left as they are: a pass inside accumulates onto
        them unless the caller drops them (``model.zero_grad()``; ``run`` marks the slots not live instead)."""
        self.ascend()
        try:
            yield self
        finally:
            self.restore()

    # ---- the recipe
    def run(self, closure: Callable[[], torch.Tensor]) -> torch.Tensor:
        """Module docstring.  ``closure`` runs the forward and returns the loss; ``run`` calls ``backward()``."""
        if self._running:
            raise RuntimeError("SAM.run: already running (run does not nest: the inner ascent would start from w + e(w))")
        opt = self.optimizer
        if opt._swapped:
            raise RuntimeError("SAM.run: the optimizer's averaged weights are swapped in (averaged_weights() is active); a "
                               "training pass now would perturb and train the average")
        if opt._perturbed:
            raise RuntimeError("SAM.run: a perturbation is already in place (restore() first)")
        A = getattr(self.model, "_icka_arena", None)
        if A is not None:
            self._refuse_reducer(A)
            live = [s.name for s in A.order if A._is_live(s)]
            if live:
                raise RuntimeError("SAM.run: %d gradient slots are already live (%s, ...): the first pass would add this batch to an "
                                   "earlier micro-batch's sum, and the perturbation must come from this batch alone "
                                   "(model.zero_grad() first; gradient accumulation is not supported)" % (len(live), live[0]))
        self._running = True
        try:
            loss = closure()
            loss.backward()
            with self.perturbed():
                for s in self._arena.order:      # the arena's own zero_grad rule: the next store into the slot overwrites
                    s.live = False
                closure().backward()
            return loss
        finally:
            self._running = False

    # ---- diagnostics
    def grad_norm(self) -> torch.Tensor:
        """Norm of the first-pass gradient of the last ascent (|p| g in adaptive mode), refused ones included: a device scalar."""
        self._bind()
        o = _lib.SamState.norm.offset
        return self._state[o:o + 4].view(torch.float32)[0]

    def _read(self) -> "_lib.SamState":
        if self._state is None:
            return _lib.SamState()
        return K.sam_state_read(self._state)

    def ascents(self) -> int:
        """Ascents applied so far (synchronises)."""
        return int(self._read().ascents)

    def skipped_ascents(self) -> int:
        """Ascents the device refused because the gradient norm was zero or not finite (synchronises)."""
        return int(self._read().skipped)
