"""TrainStep: a whole accumulation cycle of the reference's loop -- parameter update included -- replayed from captured graphs.

The reference's optimisation step (My_cross_attention.py:821-844) is ``gradient_accumulation_steps`` micro-batches of
``loss / k; loss.backward()`` and then ``clip_grad_norm_(1.0); optimizer.step(); scheduler.step(); model.zero_grad()``.
``graph.GraphedStep`` replays the micro-batches and leaves the update to the host.  With ``optim.ArenaAdamW(capturable=True)``
the update is three launches that read their step count, schedule and bias corrections from a device block, so it is captured
behind the k-th micro-batch:

    opt = ArenaAdamW(model, lr=3e-5, max_grad_norm=1.0, capturable=True, schedule=("linear", warmup_steps, total_steps))
    ts = TrainStep(model, step_fn, opt, inputs=first_batch, accumulate=k)
    for batch in loader:
        loss = ts(*batch)          # call number k of a cycle also clips, updates and moves the schedule

  * k = 1: ONE graph (gradient stores overwrite, then the update).  k > 1: THREE graphs -- overwrite (call 1 of a cycle),
    accumulate (calls 2 .. k-1), accumulate + update (call k) -- sharing one memory pool.  The position in the cycle is a host
    counter: after the k-th call it restarts, and the next call overwrites the gradients (the reference's ``zero_grad``;
    ``p.grad`` stays attached to the arena views, holding the last cycle's sum, for logging).  No torch LR scheduler, no
    ``optimizer.step()`` and no ``zero_grad()`` in the loop.  A caller that ends a cycle early (the reference's last, partial
    cycle of an epoch is simply dropped by its ``(step + 1) % k`` test) calls ``reset_cycle()``; interleaving other backward
    passes or updates of the same model between the calls of a cycle is not supported.
  * A non-finite gradient norm (a NaN batch; a fused launch that gave up a hand-off and NaN-poisoned its outputs) refuses the
    update ON THE DEVICE: weights, moments and shadows stay as they are (``optimizer.skipped_steps()``), and the host-side error
    words are still raised by the checks in front of the next replay.
  * Every replay goes through the step wrappers' common preamble (``graph._StepBase._prepare``): BiLSTM hand-off, fused dense +
    LayerNorm and packed-batch error words, and the "tracked" shadow policy (the update kernel writes fresh shadows, so there is
    nothing to re-cast).
  * A batch of another shape (the short last batch: the reference's loader has no ``drop_last``, :708) or a call in the other
    train / eval mode runs ``step_fn`` EAGERLY at the same position of the cycle -- on the k-th position followed by an eager
    ``optimizer.step()`` -- and leaves what a replay would have left.  A call never raises because of the wrapper.
  * Construction leaves no trace: the warm-up steps run the update launches DRY (the prepare launch sets the skip word and
    changes nothing else, so parameters, moments, t and the skipped count are never written), and the gradients the caller
    holds are put aside and restored (``graph._GradSnapshot``).  The captures themselves execute nothing.
  * ``ArenaAdamW(average="ema" | "swa")``: the averaging launches follow the update inside ``optimizer.step()``, so they are
    nodes of the update graph and nothing changes here; the dry warm-up leaves the average and its count untouched.  While
    ``optimizer.averaged_weights()`` is active a call raises (a replay could not check it: it runs no Python).
  * ``sam.SAM``: with ``sam.run`` in ``step_fn`` the clean pass, the ascent, the second pass and the restore are nodes of the
    same graph, in front of the update; the dry warm-up sets the ascent's skip word, so the weights are never moved and nothing
    is counted.  k > 1 is refused for a model with a registered ``SAM`` (its perturbation must come from one batch alone).

Data parallel (a ``GradReducer`` on the arena) is refused: exchanging or sharding the update inside the graph is out of scope.
"""
from __future__ import annotations

from typing import Callable

import torch

from . import kernels as K
from .attention_maps import active as _maps_active
from .graph import _GradSnapshot, _StepBase, _end_capture_quietly, _sig
from .optim import ArenaAdamW
from .sam import registered as _sam_registered

_FIRST, _MID, _LAST = "overwrite", "accumulate", "update"


class TrainStep(_StepBase):
    """``step_fn``: ``GraphedStep``'s contract (forward + backward, returns the loss; the 1 / k of the loss stays in it).
    ``optimizer``: an ``ArenaAdamW(capturable=True)`` of ``model``.  ``inputs``: the first batch (tuple / list / dict of tensors);
    ``ts(*batch)`` copies a batch into the static buffers and replays the graph of its position in the cycle.  ``stats`` counts
    ``captures`` / ``replays`` / ``eager`` calls (module docstring)."""

    _name = "TrainStep"

    def __init__(self, model: torch.nn.Module, step_fn: Callable[..., torch.Tensor], optimizer, inputs=None,
                 accumulate: int = 1, warmup: int = 3):
        if accumulate < 1:
            raise ValueError("accumulate must be >= 1")
        if not (isinstance(optimizer, ArenaAdamW) and optimizer.capturable):
            raise NotImplementedError("TrainStep captures the update: it needs optim.ArenaAdamW(capturable=True), got %s"
                                      % type(optimizer).__name__)
        if optimizer.model is not model:
            raise ValueError("TrainStep: the optimizer belongs to another model")
        if accumulate > 1 and _sam_registered(model):
            raise NotImplementedError("TrainStep(accumulate=%d): a sam.SAM is registered for this model; its first pass would add "
                                      "a micro-batch to the sum of the earlier ones, and the perturbation must come from one "
                                      "batch alone (use accumulate=1)" % accumulate)
        arena = getattr(model, "_icka_arena", None)
        if arena is not None and arena.reducer is not None:
            raise NotImplementedError("TrainStep: this model's arena has a GradReducer attached; a data-parallel update inside "
                                      "the graph is not implemented (use graph.build_step and a host-side optimizer.step())")
        self.optimizer = optimizer
        self.k = int(accumulate)
        self._pos = 0
        self._graphs = {}
        self._loss = {}
        self.stats = {"captures": 0, "replays": 0, "eager": 0}
        held = [(p, p.grad) for p in model.parameters()] if arena is None else None
        snap = _GradSnapshot(arena) if arena is not None else None
        self._setup(model, step_fn, inputs)
        self._training = bool(model.training)
        self._sigkey = self.inputs.signature() if self.inputs is not None else None
        try:
            optimizer._dry = True
            try:
                self._warm(max(1, warmup))
                self.arena = model._icka_arena
                if self.arena.reducer is not None:
                    raise NotImplementedError("TrainStep: this model's arena has a GradReducer attached")
                self.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self.side):      # binds the arena, uploads the hyperparameters, builds the chunk tables
                    optimizer.step()
                torch.cuda.current_stream().wait_stream(self.side)
                torch.cuda.synchronize()
            finally:
                optimizer._dry = False
            model.zero_grad()                           # gradients dropped -> the first capture's stores overwrite (beta = 0)
            if self.k == 1:
                self._capture(_LAST, False)
                self._grad_slots = [s for s in self.arena.order if s.live]
            else:
                self._capture(_FIRST, False)
                self._grad_slots = [s for s in self.arena.order if s.live]
                self._capture(_MID, True)
                self._capture(_LAST, True)
            self.loss = None
        except Exception:
            self._graphs = None
            self._close_nonce()
            _end_capture_quietly()
            raise
        finally:
            model.zero_grad()                           # a capture executes nothing: the gradients it "wrote" do not exist
            if snap is not None:
                snap.restore()
            else:
                for p, g in held:
                    p.grad = g

    def _capture(self, key: str, accumulate: bool) -> None:
        if accumulate:      # every gradient store of the capture must see its slot live: beta = 1, no 'mixed' memsets
            self.arena.attach_grads(self._grad_slots)
        g = torch.cuda.CUDAGraph()
        pool = next(iter(self._graphs.values())).pool() if self._graphs else None
        with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
            K.bump_dropout_nonce(self.nonce)
            self._loss[key] = self._step()
            if key == _LAST:
                self.optimizer.step()
        self._graphs[key] = g
        self.stats["captures"] += 1

    @property
    def captures(self) -> int:
        return 0 if self._graphs is None else len(self._graphs)

    def reset_cycle(self) -> None:
        """Start a new accumulation cycle at the next call: what the gradients hold is dropped (the next call overwrites
        them) and no update is made for the calls since the last one.  For a caller that ends a cycle before its k-th call."""
        self._pos = 0
        self._drop_grads()

    def _drop_grads(self) -> None:
        for s in self.arena.order:      # the arena's own zero_grad rule: the next gradient store into the slot overwrites
            s.live = False

    def _replayable(self, values) -> bool:
        if bool(self.model.training) != self._training:
            return False
        if values is None:
            return True
        return (self.inputs.is_dict, tuple(self.inputs.keys), _sig(values)) == self._sigkey

    def __call__(self, *args, **kwargs) -> torch.Tensor:
        if self._graphs is None:
            raise RuntimeError("TrainStep is closed")
        if self.optimizer._swapped:      # (a replay runs no Python: optimizer.step()'s own refusal would never be reached)
            raise RuntimeError("TrainStep: the optimizer's averaged weights are swapped in (averaged_weights() is active); a "
                               "training step now would train the average")
        values = self._values(args, kwargs)
        last = self._pos == self.k - 1
        if self._replayable(values) and not _maps_active():   # (attention maps are recorded from eager launches)
            self._prepare(False, values)
            key = _LAST if last else (_FIRST if self._pos == 0 else _MID)
            self._graphs[key].replay()
            self.arena.attach_grads(self._grad_slots)   # replay runs no Python
            self.stats["replays"] += 1
            self.loss = self._loss[key]
        else:
            self.stats["eager"] += 1
            self.loss = self._eager(values, last)
        if last:
            self._pos = 0
            self._drop_grads()
        else:
            self._pos += 1
        return self.loss

    def _eager(self, values, last: bool) -> torch.Tensor:
        """The call launched from Python at the same position of the cycle: the first one overwrites the gradients, the
        others accumulate into what the replays (or eager calls) before them left, the k-th one also updates."""
        if self._pos == 0:
            self._drop_grads()
        if values is None:
            loss = self._step()
        elif self.inputs.is_dict:
            loss = self._user_fn(**dict(zip(self.inputs.keys, values)))
        else:
            loss = self._user_fn(*values)
        if last:
            self.optimizer.step()
        return loss

    def close(self) -> None:
        """Release the graphs and unregister the dropout nonce (the kernels keep a raw pointer to it)."""
        self._close_nonce()
        self._graphs = None
