"""ArenaAdamW: the parameter update of the reference's training loop on the flat ParamArena buffers.

The reference updates with ``torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0); optimizer.step(); scheduler.step();
model.zero_grad()`` (My_cross_attention.py:831-844), ``optimizer = AdamW(grouped parameters, lr, weight_decay=0.01)`` with
biases and LayerNorm parameters in a no-decay group (:743-751).  As ~220 per-tensor launches that update costs 2.9 ms on top
of the 4.5 ms forward + backward of the c2 step.  Parameters, gradients (and here the two moment buffers) share ONE flat
layout, so the same update is three launches over chunk tables (include/icka_hip.h: icka_optim_*): gradient norm, clip
coefficient (kept on the device: no host synchronisation), and the AdamW arithmetic -- which also writes the 16-bit weight
shadows the next forward's GEMMs read, so the arena's per-forward re-cast has nothing left to do.

A ``torch.optim.Optimizer``: ``param_groups`` / ``lr`` are the usual ones, so the reference's
``get_linear_schedule_with_warmup`` (a LambdaLR) drives it unchanged.  Arithmetic = ``torch.optim.AdamW`` (what transformers
now ships in place of the ``transformers.AdamW`` the reference imported; that class is absent from the installed
transformers 5.x -- PARITY WITH IT IS UNPINNED: the defaults below (eps 1e-8, decoupled decay applied as in torch) are
torch's, the reference passed no eps; tests pin this class against torch.optim.AdamW + clip_grad_norm_).

Checkpoints: the moments and the step count live in flat arena-layout buffers, not in ``Optimizer.state``;
``state_dict()`` / ``load_state_dict()`` carry them (keys ``icka_m`` / ``icka_v`` / ``icka_t`` / ``icka_layout``), and a
resumed run continues with the same bias correction.  A state saved for another arena layout is refused; a model whose arena
is rebuilt after the first step (``.to()``, new Parameter objects) raises instead of silently restarting the moments.

``ArenaAdamW(..., capturable=True)``: the update as graph nodes.  The host mode above passes the learning rate, the step count
and both bias corrections as launch arguments, so a captured ``step()`` would freeze them.  The capturable mode keeps them in a
device block (include/icka_hip.h: icka_optim_state): ``step()`` launches icka_optim_sqnorm, icka_optim_prepare (norm,
non-finite test, clip coefficient, this update's rate and bias corrections, t += 1) and ONE icka_optim_adamw_dev for all
groups, reads nothing from the device and passes no per-step host value -- ``train_step.TrainStep`` captures it behind the last
micro-batch of an accumulation cycle.  The schedule (``schedule=None`` / ``"constant"`` / ``("linear", num_warmup_steps,
num_training_steps)`` = get_linear_schedule_with_warmup) is evaluated on the device from t; ``param_groups[g]["lr"]`` is the
BASE rate.  DO NOT attach a torch LR scheduler in this mode: it would rewrite the base rate on the host every step (uploaded
only outside a capture), compounding with the device schedule in eager steps and doing nothing at all in replayed ones.
With ``skip_nonfinite=True`` (default) a NaN / inf gradient norm refuses the update on the device: parameters, moments and
shadows stay as they are, t does not advance, ``skipped_steps()`` counts it.

``ArenaAdamW(..., average="ema" | "swa")``: an averaged copy of the weights, kept beside the update.  One more f32 buffer of the
arena's layout holds it; behind every update that ``average_start`` / ``average_every`` select, ONE launch over a chunk table of
every parameter of the groups moves it (``avg += (1 - d) * (p - avg)``; d = ``average_decay_at``: 0 for the first averaged
update, ``n / (n + 1)`` for SWA, ``min(decay, (1 + n) / (10 + n))`` for an EMA with warm-up).  In capturable mode the count n
and the decay live in a second device block (icka_average_state) written by a one-thread launch behind icka_optim_prepare, so
the averaging is captured with ``step()`` and a refused (non-finite) or dry update is neither averaged nor counted.
``averaged_weights()`` exchanges parameters and average IN PLACE (icka_optim_swap, which also writes the 16-bit shadows of the
weights it swaps in), so the model, its ``state_dict()`` and every graph captured earlier -- a ``GraphedModule`` dev pass --
run on the averaged weights inside the context without a re-cast and without a re-capture; ``step()`` and
``TrainStep.__call__`` refuse while they are swapped in.  Until the first averaged update the average holds the parameters as
they were when the optimizer bound the arena (its first ``step()`` / ``prepare_capture()``).  Checkpoints carry ``icka_avg`` /
``icka_avg_n``; a state WITHOUT them (saved by an optimizer that did not average) loaded into an averaging optimizer restarts
the average: n = 0 and the buffer a copy of the parameters at that moment, so the next averaged update copies the weights.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, Optional

import torch

from . import _lib
from . import kernels as K
from .arena import _OPT_STEPS, ParamArena, arena_of

NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")     # My_cross_attention.py:744


def reference_param_groups(model: torch.nn.Module, weight_decay: float = 0.01) -> List[dict]:
    """The reference's two groups (My_cross_attention.py:743-748): everything whose name contains 'bias', 'LayerNorm.bias'
    or 'LayerNorm.weight' is not decayed."""
    named = list(model.named_parameters())
    return [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": weight_decay},
            {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]


def schedule_factor(kind: str, warmup: int, total: int, t: int) -> float:
    """The factor the device applies to the base rate for update number t + 1 (csrc/optim.hip: optim_prepare_kernel), restated
    in Python: "constant" -> 1; "linear" -> the lambda of transformers.get_linear_schedule_with_warmup(optimizer, warmup,
    total) at scheduler step t (a LambdaLR starts at 0: with a warm-up the first update runs at rate 0)."""
    if kind == "constant":
        return 1.0
    if kind != "linear":
        raise ValueError("schedule kind %r: 'constant' or 'linear'" % (kind,))
    if t < warmup:
        return float(t) / float(max(1, warmup))
    return max(0.0, float(total - t) / float(max(1, total - warmup)))


def average_decay_at(kind: str, decay: float, warmup: bool, n: int) -> float:
    """The decay the averaged update number n + 1 uses (csrc/optim.hip: optim_average_prepare_kernel), restated in Python:
    ``avg <- avg + (1 - d) * (p - avg)``.  n == 0 -> 0 (the average starts as a copy of the weights); "swa" -> n / (n + 1)
    (the equal-weight mean of the n + 1 snapshots); "ema" -> ``decay``, with ``warmup`` min(decay, (1 + n) / (10 + n))."""
    if kind not in ("ema", "swa"):
        raise ValueError("average kind %r: 'ema' or 'swa'" % (kind,))
    if n < 0:
        raise ValueError("average_decay_at: n must be >= 0")
    if n == 0:
        return 0.0
    if kind == "swa":
        return float(n) / float(n + 1)
    return min(float(decay), float(1 + n) / float(10 + n)) if warmup else float(decay)


def average_applies(start: int, every: int, t: int) -> bool:
    """Whether update number t (1-based) is averaged: the first ``start`` updates are not, then every ``every``-th one is."""
    return t > start and (t - start - 1) % every == 0


def _parse_schedule(schedule):
    if schedule is None or schedule == "constant":
        return ("constant", 0, 0)
    if isinstance(schedule, (tuple, list)) and len(schedule) == 3 and schedule[0] == "linear":
        warmup, total = int(schedule[1]), int(schedule[2])
        if warmup < 0 or total < 0:
            raise ValueError("schedule ('linear', num_warmup_steps, num_training_steps): counts must be >= 0")
        return ("linear", warmup, total)
    raise ValueError("schedule: None, 'constant' or ('linear', num_warmup_steps, num_training_steps), got %r" % (schedule,))


class ArenaAdamW(torch.optim.Optimizer):
    def __init__(self, model: torch.nn.Module, params=None, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, max_grad_norm: Optional[float] = None, capturable: bool = False, schedule=None,
                 skip_nonfinite: bool = True, average: Optional[str] = None, average_decay: float = 0.999,
                 average_warmup: bool = True, average_start: int = 0, average_every: int = 1):
        """``model``: the module whose forward built (or will build) the ParamArena.  ``params``: parameters or param groups
        (default: ``reference_param_groups(model, weight_decay)``).  ``max_grad_norm``: clip the global gradient norm inside
        ``step()`` (the reference's clip_grad_norm_(..., 1.0)); None = no clipping.

        ``capturable=True`` (module docstring): step count, schedule and bias corrections live on the device and ``step()`` can
        be captured into a graph; at most 8 parameter groups.  ``schedule`` and ``skip_nonfinite`` belong to this mode
        (``schedule`` is refused without it).  A torch LR scheduler must NOT be attached in this mode: ``lr`` is the base rate
        of the device schedule.  Host edits of ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` reach the device at the next
        ``step()`` made outside a capture, or at once with ``sync_hyperparameters()``.  ``grad_norm()`` stays a device scalar;
        ``current_lr()``, ``steps_taken()`` and ``skipped_steps()`` read the device block and are the only calls that
        synchronise.  Before capturing ``step()`` by hand, call ``prepare_capture()`` once with the gradients in place.

        ``average="ema"`` / ``"swa"`` (module docstring; None: nothing is allocated or launched): keep an averaged copy of the
        weights of every parameter in the groups.  ``average_decay`` in [0, 1) and ``average_warmup`` belong to the EMA;
        the first ``average_start`` updates are not averaged, after them every ``average_every``-th one is."""
        if average not in (None, "ema", "swa"):
            raise ValueError("ArenaAdamW(average=): None, 'ema' or 'swa', got %r" % (average,))
        if not 0.0 <= float(average_decay) < 1.0:
            raise ValueError("ArenaAdamW(average_decay=): in [0, 1), got %r" % (average_decay,))
        if int(average_start) != average_start or average_start < 0:
            raise ValueError("ArenaAdamW(average_start=): a non-negative integer, got %r" % (average_start,))
        if int(average_every) != average_every or average_every < 1:
            raise ValueError("ArenaAdamW(average_every=): a positive integer, got %r" % (average_every,))
        if params is None:
            params = reference_param_groups(model, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self.max_grad_norm = max_grad_norm
        self.capturable = bool(capturable)
        if not self.capturable and schedule is not None:
            raise ValueError("ArenaAdamW(schedule=) belongs to capturable=True; in host mode a torch LR scheduler drives 'lr'")
        if self.capturable and len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError("ArenaAdamW(capturable=True): at most %d parameter groups, got %d"
                             % (_lib.OPTIM_MAX_GROUPS, len(self.param_groups)))
        self.schedule = _parse_schedule(schedule)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._state = None       # capturable: the icka_optim_state block (uint8 device tensor); t lives there once bound
        self._uploaded = None    # capturable: the hyperparameters the device block holds
        self._table3 = None
        self._table_cache = {}   # capturable: tables per gradient set, kept alive (a captured step() reads their addresses)
        self._dry = False        # capturable: launches that apply nothing (train_step.TrainStep's warm-up)
        self._arena: Optional[ParamArena] = None
        self._m = self._v = None
        self._t = 0
        self._sig = None
        self._tables = None
        self._norm_table = None
        self._partials = None
        self._clip = None
        self._pending = None     # state loaded before the arena was bound
        self.average = average
        self.average_decay, self.average_warmup = float(average_decay), bool(average_warmup)
        self.average_start, self.average_every = int(average_start), int(average_every)
        self._avg = None         # average=: f32 buffer of the arena's layout
        self._avg_table = None   # average=: chunk table over every parameter of the groups, built once per arena
        self._avg_state = None   # average=, capturable: the icka_average_state block; n lives there once bound
        self._avg_n = 0          # averaged updates so far (host mode; capturable: what waits for the block)
        self._swapped = False    # averaged_weights() is active: parameters and average are exchanged
        self._perturbed = False  # a sam.SAM perturbation is in place: the parameters are w + e(w), not w

    # ------------------------------------------------------------------------------------------------------------
    def _bind(self) -> ParamArena:
        A = arena_of(self.model)
        if A.device.type != "cuda":
            raise RuntimeError("ArenaAdamW: the model's parameters are on %s (icka_amd has no CPU path)" % A.device)
        if A is not self._arena:
            if self._arena is not None and self.capturable:
                self._t = int(K.optim_state_read(self._state).t)
            if self._arena is not None and self._t > 0:
                raise RuntimeError("ArenaAdamW: the model's parameter arena was rebuilt after %d optimizer steps (.to() / new "
                                   "Parameter objects): the moment buffers belong to the old layout.  Save state_dict() before "
                                   "moving the model and load it into a new optimizer afterwards." % self._t)
            self._arena = A
            self._m = torch.zeros(A.total, dtype=torch.float32, device=A.device)
            self._v = torch.zeros(A.total, dtype=torch.float32, device=A.device)
            self._clip = torch.ones(2, dtype=torch.float32, device=A.device)
            self._sig = None
            if self.capturable:
                self._state = K.optim_state_new(A.device)
                self._uploaded = None
                self._table_cache = {}
                self._write_t(self._t)
            if self.average is not None:
                self._bind_average(A)
            if self._pending is not None:       # a state loaded before the arena existed
                self._install(A, self._pending)
                self._pending = None
        return A

    def _bind_average(self, A: ParamArena) -> None:
        """The average buffer (a copy of the parameters), its chunk table over every parameter of the groups -- with or
        without a gradient: the average of a parameter that does not change is that parameter -- and, capturable, the block."""
        ranges = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                s = A.slots.get(id(p))
                if s is None:
                    raise RuntimeError("ArenaAdamW: a parameter of group %d is not in the model's arena" % gi)
                ranges.append((s.off, s.off + (s.numel + 7) // 8 * 8))
        merged = []
        for lo, hi in sorted(ranges):
            if merged and merged[-1][1] == lo:
                merged[-1] = (merged[-1][0], hi)
            else:
                merged.append((lo, hi))
        self._avg_table = K.dp_chunk_table(merged, A.device)
        self._avg = A.flat.detach().clone()
        if self.capturable:
            self._avg_state = K.average_state_new(A.device)
            h = _lib.AverageState()
            h.n = int(self._avg_n)
            h.kind = _lib.AVERAGE_SWA if self.average == "swa" else _lib.AVERAGE_EMA
            h.warmup, h.decay = int(self.average_warmup), self.average_decay
            h.start, h.every = self.average_start, self.average_every
            K.average_state_write(self._avg_state, h, 0, C.sizeof(_lib.AverageState))

    # ------------------------------------------------------------------------------------------------------------ checkpoints
    @staticmethod
    def _layout(A: ParamArena):
        return [(s.name, s.off, s.numel) for s in A.order]

    def state_dict(self):
        sd = super().state_dict()
        if self._arena is not None and self._m is not None:
            sd["icka_m"], sd["icka_v"] = self._m.detach().cpu().clone(), self._v.detach().cpu().clone()
            sd["icka_layout"] = self._layout(self._arena)
        elif self._pending is not None:
            sd["icka_m"], sd["icka_v"], sd["icka_layout"] = self._pending["icka_m"], self._pending["icka_v"], self._pending["icka_layout"]
        sd["icka_t"] = self.steps_taken() if self._state is not None else int(self._t)
        if self.average is not None:
            if self._swapped:
                raise RuntimeError("ArenaAdamW.state_dict: the averaged weights are swapped in (leave averaged_weights() first)")
            if self._avg is not None:
                sd["icka_avg"], sd["icka_avg_n"] = self._avg.detach().cpu().clone(), self.average_count()
            elif self._pending is not None and "icka_avg" in self._pending:
                sd["icka_avg"], sd["icka_avg_n"] = self._pending["icka_avg"], int(self._pending["icka_avg_n"])
        return sd

    def load_state_dict(self, state_dict):
        if self._swapped:
            raise RuntimeError("ArenaAdamW.load_state_dict: the averaged weights are swapped in (leave averaged_weights() first)")
        keys = ("icka_m", "icka_v", "icka_layout", "icka_t") + (("icka_avg", "icka_avg_n") if self.average is not None else ())
        extra = {k: state_dict[k] for k in keys if k in state_dict}
        if ("icka_avg" in extra) != ("icka_avg_n" in extra) or ("icka_avg" in extra and "icka_layout" not in extra):
            raise ValueError("ArenaAdamW.load_state_dict: 'icka_avg', 'icka_avg_n' and 'icka_layout' come together")
        if "icka_t" not in extra:
            raise ValueError("ArenaAdamW.load_state_dict: no 'icka_t' -- not a state_dict of this class (moments and step count "
                             "would silently restart)")
        super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("icka_")})
        self._t = int(extra["icka_t"])
        if self._state is not None:
            self._write_t(self._t)
        if "icka_m" in extra:
            if self._arena is not None:
                self._install(self._arena, extra)
            else:
                self._pending = extra          # installed when the arena is bound (first step)
        if self.average is not None and "icka_avg" not in extra:
            # a state without an average: it restarts from the parameters as they are now (when bound: copied here; else at _bind)
            self._write_avg_n(0)
            if self._avg is not None:
                self._avg.copy_(self._arena.flat)

    def _install(self, A: ParamArena, extra) -> None:
        if list(map(tuple, extra["icka_layout"])) != self._layout(A):
            raise ValueError("ArenaAdamW.load_state_dict: the saved moments belong to another parameter layout (different model "
                             "or registration order)")
        if "icka_avg" in extra and (self._avg is None or tuple(extra["icka_avg"].shape) != tuple(self._avg.shape)):
            raise ValueError("ArenaAdamW.load_state_dict: the saved average belongs to another parameter layout")
        self._m.copy_(extra["icka_m"])
        self._v.copy_(extra["icka_v"])
        if "icka_avg" in extra:
            self._avg.copy_(extra["icka_avg"])
            self._write_avg_n(int(extra["icka_avg_n"]))

    def _write_avg_n(self, n: int) -> None:
        self._avg_n = int(n)
        if self._avg_state is not None:
            self._avg_state[0:8].view(torch.int64).copy_(torch.tensor([int(n)], dtype=torch.int64))

    def _build(self, A: ParamArena):
        """Chunk tables: one per param group over the slots that hold a gradient this step, one over all of them."""
        sig, per_group, every = [], [], []
        for gi, group in enumerate(self.param_groups):
            ranges = []
            for p in group["params"]:
                s = A.slots.get(id(p))
                if s is None:
                    raise RuntimeError("ArenaAdamW: a parameter of group %d is not in the model's arena" % gi)
                g = p.grad
                if g is None:
                    continue
                if g.data_ptr() != A.gflat.data_ptr() + 4 * s.off:     # a foreign gradient tensor: bring it into the arena
                    A.gflat[s.off:s.off + s.numel].view(s.shape).copy_(g)
                lo, hi = s.off, s.off + (s.numel + 7) // 8 * 8
                if ranges and ranges[-1][1] == lo:
                    ranges[-1] = (ranges[-1][0], hi)
                else:
                    ranges.append((lo, hi))
                sig.append(s.off)
            per_group.append(ranges)
            every += ranges
        sig = tuple(sig)
        if sig != self._sig and self.capturable:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ArenaAdamW(capturable=True): the set of parameters that hold a gradient %s; inside a capture "
                                   "step() cannot build its chunk tables (call prepare_capture() or one step() outside the "
                                   "capture, with the same gradients in place)"
                                   % ("changed" if self._sig is not None else "is not known yet"))
            hit = self._table_cache.get(sig)
            if hit is None:
                norm = K.dp_chunk_table(sorted(every), A.device)
                hit = self._table_cache[sig] = (norm, K.optim_chunk_table3([sorted(r) for r in per_group], A.device),
                                                torch.empty(max(1, norm.shape[0]), dtype=torch.float32, device=A.device))
            self._sig = sig
            self._norm_table, self._table3, self._partials = hit
        elif sig != self._sig:
            self._sig = sig
            self._tables = [K.dp_chunk_table(sorted(r), A.device) for r in per_group]
            self._norm_table = K.dp_chunk_table(sorted(every), A.device)
            self._partials = torch.empty(max(1, self._norm_table.shape[0]), dtype=torch.float32, device=A.device)

    # ------------------------------------------------------------------------------------------------------------ capturable mode
    def _need_capturable(self, what: str) -> None:
        if not self.capturable:
            raise RuntimeError("ArenaAdamW.%s belongs to capturable=True" % what)

    def _write_t(self, t: int) -> None:
        self._state[0:8].view(torch.int64).copy_(torch.tensor([int(t)], dtype=torch.int64))

    def _hyperparameters(self):
        return (self.schedule,) + tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                         float(g["weight_decay"])) for g in self.param_groups)

    def sync_hyperparameters(self) -> None:
        """Upload the schedule and every group's ``lr`` (the base rate) / ``betas`` / ``eps`` / ``weight_decay`` into the
        device block now (``step()`` does so by itself when they changed, but only outside a capture)."""
        self._need_capturable("sync_hyperparameters()")
        self._bind()
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError("ArenaAdamW(capturable=True): at most %d parameter groups" % _lib.OPTIM_MAX_GROUPS)
        h = _lib.OptimState()
        kind, h.warmup, h.total = self.schedule
        h.kind = _lib.OPTIM_SCHEDULE_LINEAR if kind == "linear" else _lib.OPTIM_SCHEDULE_CONSTANT
        h.n_groups = len(self.param_groups)
        hp = self._hyperparameters()
        for i, (lr, b1, b2, eps, wd) in enumerate(hp[1:]):
            h.base_lr[i], h.beta1[i], h.beta2[i], h.eps[i], h.weight_decay[i] = lr, b1, b2, eps, wd
        K.optim_state_write(self._state, h, _lib.OptimState.HOST_LO, _lib.OptimState.HOST_HI)
        self._uploaded = hp

    def prepare_capture(self) -> None:
        """Bind the arena, upload the hyperparameters and build the chunk tables for the gradients held NOW, launching
        nothing: what a hand-made capture of ``step()`` needs beforehand (``train_step.TrainStep`` warms up by itself)."""
        self._need_capturable("prepare_capture()")
        A = self._bind()
        self._build(A)
        self.sync_hyperparameters()

    def _read_state(self):
        self._need_capturable("device-state reads")
        self._bind()
        return K.optim_state_read(self._state)

    def steps_taken(self) -> int:
        """Updates applied so far (t of the device block; synchronises).  Host mode: the host counter."""
        if self._state is None:          # host mode, or not bound yet (a loaded count waits on the host)
            return int(self._t)
        return int(K.optim_state_read(self._state).t)

    def skipped_steps(self) -> int:
        """Updates the device refused because the gradient norm was not finite (synchronises)."""
        return int(self._read_state().skipped)

    def current_lr(self) -> List[float]:
        """Per group, the rate the last applied update used, as the device computed it (synchronises; zeros before the
        first update)."""
        st = self._read_state()
        return [float(st.lr[i]) for i in range(len(self.param_groups))]

    def _step_capturable(self, A: ParamArena) -> None:
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing and self._uploaded != self._hyperparameters():
            self.sync_hyperparameters()
        n = self._norm_table.shape[0]
        K.optim_sqnorm(A.gflat, self._norm_table, self._partials)
        K.optim_prepare(self._partials, n, float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0, self._state,
                        dry=self._dry, guard=self.skip_nonfinite)
        K.optim_adamw_dev(A.flat, A.gflat, self._m, self._v, A.shadow, A.shadow16, self._table3, self._state)
        if self.average is not None:
            K.optim_average_prepare(self._avg_state, self._state)
            K.optim_average_dev(A.flat, self._avg, self._avg_table, self._avg_state)

    @torch.no_grad()
    def step(self, closure=None):
        if self._swapped:
            raise RuntimeError("ArenaAdamW.step: the averaged weights are swapped in (averaged_weights() is active); an update "
                               "now would train the average and average the trained weights")
        if self._perturbed:
            raise RuntimeError("ArenaAdamW.step: a sharpness-aware perturbation is in place (SAM.perturbed() is active); an "
                               "update now would move w + e(w), and the restore would then throw it away")
        loss = closure() if closure is not None else None
        if self.capturable and self._uploaded is None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ArenaAdamW(capturable=True): call prepare_capture() (or one step()) before capturing step()")
        A = self._bind()
        self._build(A)
        if self._norm_table.shape[0] == 0:
            return loss
        if self.capturable:
            self._step_capturable(A)
            self._mark_shadows_fresh(A)
            return loss
        lib = K._lib.load()
        st = K._stream()
        self._t += 1
        coef = None
        if self.max_grad_norm is not None:
            K.check(lib.icka_optim_sqnorm(A.gflat.data_ptr(), self._norm_table.data_ptr(), self._norm_table.shape[0],
                                          self._partials.data_ptr(), st), "icka_optim_sqnorm")
            K.check(lib.icka_optim_clip(self._partials.data_ptr(), self._norm_table.shape[0], float(self.max_grad_norm),
                                        self._clip.data_ptr(), st), "icka_optim_clip")
            coef = self._clip[1:].data_ptr()
        sh = A.shadow.data_ptr() if A.shadow is not None else None
        sh16 = A.shadow16.data_ptr() if A.shadow16 is not None else None
        for group, table in zip(self.param_groups, self._tables):
            if table.shape[0] == 0:
                continue
            b1, b2 = group["betas"]
            K.check(lib.icka_optim_adamw(A.flat.data_ptr(), A.gflat.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), sh, sh16,
                                         table.data_ptr(), table.shape[0], coef, float(group["lr"]), float(b1), float(b2),
                                         float(group["eps"]), float(group["weight_decay"]), self._t, st), "icka_optim_adamw")
        if self.average is not None and average_applies(self.average_start, self.average_every, self._t):
            K.optim_average(A.flat, self._avg, self._avg_table,
                            average_decay_at(self.average, self.average_decay, self.average_warmup, self._avg_n))
            self._avg_n += 1
        self._mark_shadows_fresh(A)
        return loss

    # ------------------------------------------------------------------------------------------------------------ averaged weights
    def _need_average(self, what: str) -> ParamArena:
        if self.average is None:
            raise RuntimeError("ArenaAdamW.%s belongs to average='ema' / 'swa'" % what)
        return self._bind()

    def average_count(self) -> int:
        """Averaged updates so far (n of the device block in capturable mode: synchronises; host mode: the host counter)."""
        if self.average is None:
            raise RuntimeError("ArenaAdamW.average_count() belongs to average='ema' / 'swa'")
        if self._avg_state is None:       # host mode, or not bound yet (a loaded count waits on the host)
            return int(self._pending["icka_avg_n"]) if self._pending is not None and "icka_avg_n" in self._pending \
                else int(self._avg_n)
        return int(K.average_state_read(self._avg_state).n)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the context the model runs on the averaged weights: parameters and average are exchanged in place (one
        launch, which also writes the 16-bit shadows), so ``model.state_dict()``, eager forwards and graphs captured earlier
        all see them; on exit -- also after an exception -- they are exchanged back, bit for bit.  No re-cast is triggered
        under the "tracked" shadow policy.  ``step()`` / ``TrainStep.__call__`` raise inside it; it does not nest.  What follows
        the swap is the arena (masters and shadows); a weight copy a module derives for itself outside the arena -- the image
        encoder's GEMM-layout convolution weights (``icka_amd.resnet``) -- does not: keep such a module out of the groups (the
        reference's loop leaves its ResNet frozen)."""
        A = self._need_average("averaged_weights()")
        if self._swapped:
            raise RuntimeError("ArenaAdamW.averaged_weights(): already active (the context does not nest)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ArenaAdamW.averaged_weights(): not inside a capture")
        if self._perturbed:
            raise RuntimeError("ArenaAdamW.averaged_weights(): a sharpness-aware perturbation is in place (SAM.perturbed() is "
                               "active); its restore would overwrite the averaged weights with the trained ones")
        K.optim_swap(A.flat, self._avg, A.shadow, A.shadow16, self._avg_table)
        self._swapped = True
        try:
            yield self
        finally:
            K.optim_swap(A.flat, self._avg, A.shadow, A.shadow16, self._avg_table)
            self._swapped = False

    @torch.no_grad()
    def averaged_state_dict(self):
        """The averaged weights keyed like ``model.state_dict()`` (fresh tensors on the parameters' device).  Parameters that
        are in no group, and buffers, are passed through as the model holds them.  Does not swap."""
        A = self._need_average("averaged_state_dict()")
        avg = A.flat if self._swapped else self._avg      # (while swapped, the arena holds the average)
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        sd = self.model.state_dict()
        named = dict(self.model.named_parameters(remove_duplicate=False))
        out = type(sd)()
        for k, v in sd.items():
            p = named.get(k)
            s = A.slots.get(id(p)) if p is not None else None
            if s is not None and id(p) in mine:
                out[k] = avg[s.off:s.off + s.numel].view(s.shape).clone()
            else:
                out[k] = v.detach().clone()
        return out

    @staticmethod
    def _mark_shadows_fresh(A: ParamArena) -> None:
        # every GEMM operand that changed got its 16-bit shadows from the update kernel itself (embedding tables have none):
        # tell the arena, so that the "tracked" policy does not re-cast after this step (the global post-step hook bumps
        # _OPT_STEPS by one right after step() returns; parameters not in any group / without gradient did not change)
        v = _OPT_STEPS[0] + 1
        for s in A.order:
            v += s.param._version
        A._synced = v

    def grad_norm(self) -> torch.Tensor:
        """Total gradient norm of the last clipped step (device scalar, as clip_grad_norm_ returns it).  Capturable mode: of
        the last step, clipped or not -- the norm word of the device block."""
        if self.capturable:
            self._bind()
            return self._state[_lib.OptimState.norm.offset:_lib.OptimState.norm.offset + 4].view(torch.float32)[0]
        return self._clip[0]
