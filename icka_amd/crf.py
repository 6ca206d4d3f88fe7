"""Linear-chain CRF layer on the HIP kernels (`icka_crf_*`).

Drop-in for the ``torchcrf.CRF`` object the reference constructs as ``CRF(num_tags, batch_first=True)``
(Cross_Modal_Interaction_Module.py:911; my_bert/cl_modeling.py:1269) and calls as
``-crf(emissions, tags=labels, mask=mask, reduction='token_mean' | 'mean')`` and ``crf.decode(emissions, mask=mask)``
(:1045-1057; cl_modeling.py:1380-1386): same constructor, parameter names (``start_transitions``, ``end_transitions``,
``transitions``), initialisation (uniform(-0.1, 0.1)), argument validation and return types.  The arithmetic follows
pytorch-crf 0.7.2 (the package is third-party and absent from the reference tree: parity unpinned, see
oracle/crf_oracle.py)."""
from __future__ import annotations

import contextlib
import threading
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import kernels as K
from .arena import ArenaModule, ParamArena, arena_of

F32 = torch.float32
_state = threading.local()


@contextlib.contextmanager
def device_decode():
    """While active (on this thread), ``CRF.decode`` and ``CRF.decode_llh`` return a ``DeviceTags`` instead of python lists:
    one launch, no host sync, so the call can be captured in a graph.  ``graph.GraphedModule(..., decode=True)`` sets it around
    the calls it captures and replays."""
    prev = getattr(_state, "on", False)
    _state.on = True
    try:
        yield
    finally:
        _state.on = prev


def device_decode_active() -> bool:
    return getattr(_state, "on", False)


def split_tags(lens: Sequence[int], flat: Sequence[int]) -> List[List[int]]:
    """Cut the back-to-back paths ``flat`` into one list per sample of ``lens[b]`` tags."""
    out, o = [], 0
    for n in lens:
        n = int(n)
        if n < 0 or o + n > len(flat):
            raise ValueError("path lengths %s do not fit %d tags" % (list(lens), len(flat)))
        out.append(list(flat[o:o + n]))
        o += n
    return out


class DeviceTags(object):
    """Viterbi paths kept on the device (``icka_crf_score_decode``): ``lens`` int32 [B] and ``tags_flat`` int32 [>= B*S], the
    paths back to back.  ``tolist()`` gives what ``CRF.decode`` returns.  ``DeviceTags.empty`` puts both in one buffer so that
    ``tolist()`` is one device-to-host copy.  ``deferred_check`` (None or a callable): the error check the producer did NOT run
    because it did not sync the host (``GraphedModule(decode="device")``); whoever reads results derived from these tags back
    calls it after that copy (``metrics.ChunkEvaluator.compute`` does)."""

    def __init__(self, lens: torch.Tensor, tags_flat: torch.Tensor, _joint: Optional[torch.Tensor] = None):
        for n, t in (("lens", lens), ("tags_flat", tags_flat)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("DeviceTags: %s must be a tensor, got %s" % (n, type(t).__name__))
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("DeviceTags: %s must be a contiguous 1-D int32 tensor, got %s %s"
                                 % (n, t.dtype, tuple(t.shape)))
        if lens.device != tags_flat.device:
            raise ValueError("DeviceTags: lens on %s, tags_flat on %s" % (lens.device, tags_flat.device))
        self.lens = lens
        self.tags_flat = tags_flat
        self._joint = _joint
        self.deferred_check = None

    @classmethod
    def empty(cls, B: int, S: int, device) -> "DeviceTags":
        buf = torch.empty(B + B * S, dtype=torch.int32, device=device)
        return cls(buf[:B], buf[B:], _joint=buf)

    @property
    def batch_size(self) -> int:
        return self.lens.numel()

    @property
    def capacity(self) -> int:
        return self.tags_flat.numel()

    def check(self, B: int, S: int) -> None:
        """Raise unless this can hold the paths of a [B, S] batch."""
        K.check_flat_tags(self.lens, self.tags_flat, B, S)

    def tolist(self) -> List[List[int]]:
        if self._joint is not None:
            h = self._joint.cpu().tolist()
            B = self.batch_size
            lens, flat = h[:B], h[B:]
        else:
            lens, flat = self.lens.cpu().tolist(), self.tags_flat.cpu().tolist()
        return split_tags(lens, flat)

    def __repr__(self) -> str:
        return "DeviceTags(batch=%d, capacity=%d, device=%s)" % (self.batch_size, self.capacity, self.lens.device)


def _check_reduction(reduction: str) -> None:
    if reduction not in ("none", "sum", "mean", "token_mean"):
        raise ValueError("invalid reduction: %s" % reduction)


def _grads_for_atomics(mod, A: ParamArena):
    """The three transition parameters of ``mod`` and their arena gradients, which the gradient kernels ADD to with atomics: so
    they are zeroed here on the first write of an accumulation cycle."""
    ps = (mod.start_transitions, mod.end_transitions, mod.transitions)
    if A.grad_beta(ps) == 0.0:
        for p in ps:
            A.g(p).zero_()
    return ps, tuple(A.g(p) for p in ps)


class _CrfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, emissions, tags, mask, mod, A: ParamArena):
        B = emissions.shape[0]
        llh = torch.empty(B, dtype=F32, device=emissions.device)
        K.crf_llh(emissions, tags, mask, mod.start_transitions, mod.end_transitions, mod.transitions, llh)
        ctx.mod, ctx.A = mod, A
        ctx.save_for_backward(emissions, tags, mask)
        return llh

    @staticmethod
    def backward(ctx, gllh):
        emissions, tags, mask = ctx.saved_tensors
        ps, gs = _grads_for_atomics(ctx.mod, ctx.A)
        de = torch.empty_like(emissions)
        K.crf_grad(emissions, tags, mask, *ps, gllh.to(F32).contiguous(), de, *gs)
        ctx.A.flush_final()
        return None, de, None, None, None, None


class _CrfConstrainedFn(torch.autograd.Function):
    """``log Z_A - log Z`` per sample (icka_crf_constrained_llh / _grad); the arena gradients are handled as in ``_CrfFn``."""

    @staticmethod
    def forward(ctx, anchor, emissions, allowed, mask, mod, A: ParamArena):
        B = emissions.shape[0]
        out = torch.empty(3, B, dtype=F32, device=emissions.device)      # llh | log Z | log Z_A
        K.crf_constrained_llh(emissions, mask, allowed, mod.start_transitions, mod.end_transitions, mod.transitions,
                              out[0], out[1], out[2])
        ctx.mod, ctx.A = mod, A
        ctx.save_for_backward(emissions, allowed, mask)
        return out[0]

    @staticmethod
    def backward(ctx, gllh):
        emissions, allowed, mask = ctx.saved_tensors
        ps, gs = _grads_for_atomics(ctx.mod, ctx.A)
        de = torch.empty_like(emissions)
        K.crf_constrained_grad(emissions, mask, allowed, *ps, gllh.to(F32).contiguous(), de, *gs)
        ctx.A.flush_final()
        return None, de, None, None, None, None


class _ExpectCfg(object):
    """What one ``_CrfExpectFn`` call is asked for.  ``relative``: the payoff mode of icka_crf_expect; ``want_expect``: False
    computes log Z only; ``other`` / ``A_other``: the CRF (and its arena) whose three parameters are the second lattice's, or
    None when those parts are plain tensors; ``first_grad`` / ``second_grad``: whether that lattice is differentiated."""

    def __init__(self, relative, want_expect, other=None, A_other=None, first_grad=True, second_grad=True):
        self.relative, self.want_expect, self.other, self.A_other = relative, want_expect, other, A_other
        self.first_grad, self.second_grad = first_grad, second_grad


def _params(mod):
    return (mod.start_transitions.detach(), mod.end_transitions.detach(), mod.transitions.detach())


class _CrfExpectFn(torch.autograd.Function):
    """``(log Z_p, E_p[r])`` per sample (icka_crf_expect / _grad): one launch forward, one backward.  The gradients of a CRF
    module's own parameters -- the first lattice's and, with ``cfg.other``, the second's -- are added into the arena as in
    ``_CrfFn``; payoff parts given as plain tensors get theirs through autograd from freshly zeroed buffers."""

    @staticmethod
    def forward(ctx, anchor, emissions, mask, mod, A: ParamArena, cfg: _ExpectCfg, second, second_start, second_end,
                second_trans):
        B = emissions.shape[0]
        out = torch.empty(2 if cfg.want_expect else 1, B, dtype=F32, device=emissions.device)     # log Z | E[r]
        if cfg.other is not None:
            second_start, second_end, second_trans = _params(cfg.other)
        K.crf_expect(emissions, mask, *_params(mod), out[0], out[1] if cfg.want_expect else None, second=second,
                     second_start=second_start, second_end=second_end, second_trans=second_trans, relative=cfg.relative)
        ctx.mod, ctx.A, ctx.cfg = mod, A, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(emissions, mask, second, second_start, second_end, second_trans)
        return out[0], (out[1] if cfg.want_expect else None)

    @staticmethod
    def backward(ctx, g_logz, g_expect):
        emissions, mask, second, s_start, s_end, s_trans = ctx.saved_tensors
        cfg = ctx.cfg
        none = (None,) * 10
        g_logz = None if g_logz is None else g_logz.to(F32).contiguous()
        g_expect = None if g_expect is None else g_expect.to(F32).contiguous()
        if g_logz is None and g_expect is None:
            return none
        de, gs = None, (None, None, None)
        if cfg.first_grad:
            _, gs = _grads_for_atomics(ctx.mod, ctx.A)
            de = torch.empty_like(emissions)
        d2, gs2 = None, (None, None, None)
        if cfg.second_grad and g_expect is not None:
            if second is not None and ctx.needs_input_grad[6]:
                d2 = torch.empty_like(second)
            if cfg.other is not None:
                _, gs2 = _grads_for_atomics(cfg.other, cfg.A_other)
            else:
                gs2 = tuple(torch.zeros_like(t) if t is not None and ctx.needs_input_grad[7 + n] else None
                            for n, t in enumerate((s_start, s_end, s_trans)))
        K.crf_expect_grad(emissions, mask, *_params(ctx.mod), g_logz, g_expect, de, *gs, second=second, second_start=s_start,
                          second_end=s_end, second_trans=s_trans, relative=cfg.relative, d_second=d2, d_second_start=gs2[0],
                          d_second_end=gs2[1], d_second_trans=gs2[2])
        if cfg.first_grad:
            ctx.A.flush_final()
        if cfg.other is not None and gs2[0] is not None:
            cfg.A_other.flush_final()
            gs2 = (None, None, None)      # the arena holds them: nothing goes through autograd
        return (None, de, None, None, None, None, d2) + tuple(gs2)


class CRF(ArenaModule):
    def __init__(self, num_tags: int, batch_first: bool = False) -> None:
        if num_tags <= 0:
            raise ValueError("invalid number of tags: %d" % num_tags)
        if num_tags > 64:
            raise ValueError("icka_amd.CRF supports at most 64 tags (one lane per tag)")
        super().__init__()
        self.num_tags = num_tags
        self.batch_first = batch_first
        self.start_transitions = nn.Parameter(torch.empty(num_tags))
        self.end_transitions = nn.Parameter(torch.empty(num_tags))
        self.transitions = nn.Parameter(torch.empty(num_tags, num_tags))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.uniform_(self.start_transitions, -0.1, 0.1)
        nn.init.uniform_(self.end_transitions, -0.1, 0.1)
        nn.init.uniform_(self.transitions, -0.1, 0.1)

    def __repr__(self) -> str:
        return "%s(num_tags=%d)" % (self.__class__.__name__, self.num_tags)

    # ------------------------------------------------------------------------------------------------------------
    def _prep(self, emissions, tags, mask):
        if emissions.dim() != 3:
            raise ValueError("emissions must have dimension of 3, got %d" % emissions.dim())
        if emissions.size(2) != self.num_tags:
            raise ValueError("expected last dimension of emissions is %d, got %d" % (self.num_tags, emissions.size(2)))
        if not emissions.is_cuda:
            raise TypeError("icka_amd.CRF: emissions are on %s; there is no CPU path" % emissions.device)
        if not self.batch_first:   # the kernels are batch-first
            emissions = emissions.transpose(0, 1)
            tags = tags.transpose(0, 1) if tags is not None else None
            mask = mask.transpose(0, 1) if mask is not None else None
        B, S, _ = emissions.shape
        if tags is not None and tuple(tags.shape) != (B, S):
            raise ValueError("the first two dimensions of emissions and tags must match, got %s and %s"
                             % ((B, S), tuple(tags.shape)))
        if mask is not None:
            if tuple(mask.shape) != (B, S):
                raise ValueError("the first two dimensions of emissions and mask must match, got %s and %s"
                                 % ((B, S), tuple(mask.shape)))
            mask = (mask != 0).to(torch.int64).contiguous()
        e = emissions.to(F32).contiguous()
        t = tags.to(torch.int64).contiguous() if tags is not None else None
        return e, t, mask

    def forward(self, emissions: torch.Tensor, tags: torch.Tensor, mask: Optional[torch.Tensor] = None,
                reduction: str = "sum") -> torch.Tensor:
        """Log-likelihood of ``tags`` given ``emissions`` (``none`` | ``sum`` | ``mean`` | ``token_mean``).
        Like the package, the first position of every sequence is treated as unmasked (the package raises when it is
        not; checking would cost a device->host sync, so it is not checked here)."""
        _check_reduction(reduction)
        e, t, m = self._prep(emissions, tags, mask)
        A = self._arena()
        llh = _CrfFn.apply(A.anchor, e, t, m, self, A)
        return self._reduce(llh, m, e, reduction)

    @staticmethod
    def _reduce(llh: torch.Tensor, m: Optional[torch.Tensor], e: torch.Tensor, reduction: str) -> torch.Tensor:
        if reduction == "none":
            return llh
        if reduction == "sum":
            return llh.sum()
        if reduction == "mean":
            return llh.mean()
        n = m.to(F32).sum() if m is not None else float(e.shape[0] * e.shape[1])
        return llh.sum() / n

    def _score_decode(self, e, t, m, out: Optional[DeviceTags]):
        B, S = e.shape[0], e.shape[1]
        if out is None:
            out = DeviceTags.empty(B, S, e.device)
        out.check(B, S)
        llh = torch.empty(B, dtype=F32, device=e.device) if t is not None else None
        self._arena()
        K.crf_score_decode(e, t, m, self.start_transitions.detach(), self.end_transitions.detach(),
                           self.transitions.detach(), llh, out.lens, out.tags_flat)
        return out, llh

    def decode_llh(self, emissions: torch.Tensor, tags: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   reduction: str = "sum"):
        """``(self.decode(emissions, mask), self(emissions, tags, mask, reduction))`` -- the dev pass of the reference.  Under
        ``device_decode()`` (and without autograd to feed) both come from ONE launch: ``(DeviceTags, llh)``, the llh bit for
        bit the forward's."""
        _check_reduction(reduction)
        if not device_decode_active() or (torch.is_grad_enabled() and
                                          (emissions.requires_grad or self.transitions.requires_grad)):
            return self.decode(emissions, mask), self(emissions, tags, mask, reduction)
        e, t, m = self._prep(emissions.detach(), tags, mask)
        out, llh = self._score_decode(e, t, m, None)
        return out, self._reduce(llh, m, e, reduction)

    def decode(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[DeviceTags] = None):
        """Most likely tag sequence per sample (Viterbi), as python lists of length sum(mask).  Under ``device_decode()``, or
        given ``out``, a ``DeviceTags`` (written into ``out`` when given) instead."""
        if out is not None or device_decode_active():
            e, _, m = self._prep(emissions.detach(), None, mask)
            return self._score_decode(e, None, m, out)[0]
        e, _, m = self._prep(emissions.detach(), None, mask)
        self._arena()
        best = torch.empty(e.shape[0], e.shape[1], dtype=torch.int64, device=e.device)
        K.crf_decode(e, m, self.start_transitions.detach(), self.end_transitions.detach(), self.transitions.detach(),
                     best)
        rows = best.cpu().tolist()
        return [[v for v in r if v >= 0] for r in rows]

    def decode_nbest(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, nbest: int = 1) -> "NBestPaths":
        """The ``nbest`` most likely tag sequences per sample, best first (``icka_crf_nbest``; the definitions and the tie rule
        are written out in include/icka_hip.h): one launch, no host sync, capturable in a graph.  A path has one tag per
        on-position (position 0 and the positions with ``mask != 0``); a sample with fewer than ``nbest`` distinct paths
        (``num_tags ** L``) reports that many in ``n_paths``.  Rank 0 is ``decode``'s path.  Detached.  Limits:
        ``num_tags <= 16``, ``1 <= nbest <= 8``, ``S <= 512``, ``B <= 2048``, ``S * num_tags * nbest <= 49152``.  Exact
        log-probabilities of the ranks take ``log_z`` from a second launch: ``out.log_probs(crf.posterior(...).log_z)``, or
        ``crf.posterior(emissions, out.rank(r), mask).seq_logp`` per rank."""
        e, _, m = self._prep(emissions.detach(), None, mask)
        self._arena()
        B, S, _ = e.shape
        if isinstance(nbest, bool) or not isinstance(nbest, int):
            raise ValueError("CRF.decode_nbest: nbest must be an int, got %s" % type(nbest).__name__)
        if not 1 <= nbest <= K.CRF_NBEST_MAX_K:     # before the buffers are sized by it
            raise ValueError("CRF.decode_nbest: 1 <= nbest <= %d, got %d" % (K.CRF_NBEST_MAX_K, nbest))
        out = NBestPaths(B, S, nbest, e.device)
        K.crf_nbest(e, m, self.start_transitions.detach(), self.end_transitions.detach(), self.transitions.detach(), nbest,
                    out.lens, out.n_paths, out.scores, out.tags)
        return out

    def sample(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, num_samples: int = 1,
               seed=0) -> "SampledPaths":
        """``num_samples`` independent exact draws from ``p(y | emissions)`` per sample (``icka_crf_sample``; the algorithm and
        the uniforms are written out in include/icka_hip.h): one launch, no host sync, capturable in a graph.  A path has one
        tag per on-position (position 0 and the positions with ``mask != 0``).  ``seed``: an int in [0, 2^64), or a device
        int64 [1] tensor whose two 32-bit halves are XORed into a by-value seed of 0 -- a captured graph that increments that
        tensor draws fresh paths on every replay.  Equal arguments give bitwise equal results; no process-wide state is
        read.  A tag whose step weight underflows to 0 (a ``-1e4`` transition) is never drawn.  Detached.  Limits:
        ``num_tags <= 64``, ``1 <= num_samples <= 64``, ``S * num_tags <= 12288``, ``B <= 2048``.  Sampling under allowed sets
        and packed batches are not covered."""
        e, _, m = self._prep(emissions.detach(), None, mask)
        self._arena()
        B, S, Cn = e.shape
        if isinstance(num_samples, bool) or not isinstance(num_samples, int):
            raise ValueError("CRF.sample: num_samples must be an int, got %s" % type(num_samples).__name__)
        if not 1 <= num_samples <= K.CRF_SAMPLE_MAX_K:     # before the buffers are sized by it
            raise ValueError("CRF.sample: 1 <= num_samples <= %d, got %d" % (K.CRF_SAMPLE_MAX_K, num_samples))
        if S * Cn > K.CRF_MAX_SC:
            raise ValueError("CRF.sample: S * num_tags <= %d, got %d * %d = %d" % (K.CRF_MAX_SC, S, Cn, S * Cn))
        if B > K.CRF_FLAT_MAX_B:
            raise ValueError("CRF.sample: B <= %d, got %d" % (K.CRF_FLAT_MAX_B, B))
        seed_dev = None
        if isinstance(seed, torch.Tensor):
            if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != e.device:
                raise ValueError("CRF.sample: a tensor seed must be int64 [1] on %s, got %s %s on %s"
                                 % (e.device, seed.dtype, tuple(seed.shape), seed.device))
            seed_dev, seed = seed.reshape(1), 0
        elif isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError("CRF.sample: seed must be an int in [0, 2^64) or a device int64 [1] tensor, got %r" % (seed,))
        out = SampledPaths(B, S, num_samples, e.device)
        K.crf_sample(e, m, self.start_transitions.detach(), self.end_transitions.detach(), self.transitions.detach(),
                     num_samples, seed, seed_dev, out.lens, out.log_z, out.scores, out.tags)
        return out

    def path_llh(self, emissions: torch.Tensor, paths, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``log p(path | emissions)`` of every row of ``paths`` -- a ``DeviceTags`` (one row), an ``NBestPaths`` or a
        ``SampledPaths`` -- f32 [B, R], differentiable in ``emissions`` and the three parameters: the candidate
        log-probabilities of minimum-risk training (``minimum_risk``).  Each row becomes singleton allowed sets at the
        on-positions (torch ops on the device, no host sync) and goes through ``constrained_llh``'s kernels, one call per
        row: ``score(path) - log Z`` in the chain over position 0 and the positions with ``mask != 0``.  A missing rank (-1
        tags), a tag outside [0, num_tags) or a path shorter than its sample's chain is an empty set: value ``-inf``, zero
        gradient."""
        who = "CRF.path_llh"
        if isinstance(paths, DeviceTags):
            lens, rows = paths.lens, paths.tags_flat[None, :]
        elif isinstance(paths, (NBestPaths, SampledPaths)):
            lens, rows = paths.lens, paths.tags
        else:
            raise ValueError("%s: paths must be a DeviceTags, NBestPaths or SampledPaths, got %s" % (who, type(paths).__name__))
        e, _, m = self._prep(emissions, None, mask)
        B, S, Cn = e.shape
        if lens.numel() != B or lens.device != e.device:
            raise ValueError("%s: paths hold %d samples on %s for a batch of %d on %s"
                             % (who, lens.numel(), lens.device, B, e.device))
        if S * Cn > K.CRF_MAX_SC:
            raise ValueError("%s: S * num_tags <= %d, got %d * %d = %d" % (who, K.CRF_MAX_SC, S, Cn, S * Cn))
        if m is not None:
            m[:, 0] = 1            # (m is _prep's own copy) position 0 is on, as in posterior
        on = torch.ones(B, S, dtype=torch.bool, device=e.device) if m is None else m != 0
        ln = lens.to(torch.int64)
        rank = on.to(torch.int64).cumsum(1) - 1                         # index of an on-position in its sample's path
        cap = rows.shape[1]
        idx = ((ln.cumsum(0) - ln)[:, None] + rank).clamp(0, cap - 1)
        inside = on & (rank < ln[:, None])
        A = self._arena()
        out = []
        for r in range(rows.shape[0]):
            t = rows[r].to(torch.int64)[idx]
            ok = inside & (t >= 0) & (t < Cn)
            al = torch.where(ok, torch.ones_like(t) << t.clamp(0, 63), torch.zeros_like(t)).contiguous()
            out.append(_CrfConstrainedFn.apply(A.anchor, e, al, m, self, A))
        return torch.stack(out, 1)

    # ------------------------------------------------------------------------------------------------- posteriors
    def marginals(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``P(y_t = j | emissions)``, f32 in the layout of ``emissions`` ([B,S,C], or [S,B,C] without ``batch_first``): the
        chain runs over position 0 and the positions with ``mask != 0``; the other positions hold exact zeros.  Detached;
        one launch, no host sync."""
        e, _, m = self._prep(emissions.detach(), None, mask)
        self._arena()
        B, S, Cn = e.shape
        out = torch.empty(B, S, Cn, dtype=F32, device=e.device)
        small = torch.empty(B + 1, dtype=torch.int32, device=e.device)     # log Z and the (unused: no path) refusal count
        K.crf_posterior(e, m, self.start_transitions.detach(), self.end_transitions.detach(), self.transitions.detach(),
                        small[:B].view(F32), small[B:], marginals=out)
        return out if self.batch_first else out.transpose(0, 1)

    def _paths_into(self, tags: DeviceTags, paths, m: Optional[torch.Tensor], B: int, S: int) -> None:
        """Write ``paths`` (DeviceTags | integer [B,S] device tensor | per-sample lists) into ``tags`` without a host sync."""
        if isinstance(paths, DeviceTags):
            if paths.batch_size != B:
                raise ValueError("paths hold %d samples for a batch of %d" % (paths.batch_size, B))
            n = min(paths.capacity, tags.capacity)
            tags.lens.copy_(paths.lens)
            tags.tags_flat[:n].copy_(paths.tags_flat[:n])
            tags.deferred_check = paths.deferred_check
        elif isinstance(paths, torch.Tensor):
            if not self.batch_first:
                paths = paths.transpose(0, 1)
            if paths.is_floating_point() or tuple(paths.shape) != (B, S) or paths.device != tags.lens.device:
                raise ValueError("paths must be an integer [B, S] tensor on the device of the emissions, got %s %s on %s"
                                 % (paths.dtype, tuple(paths.shape), paths.device))
            dev, cap = paths.device, tags.capacity
            if m is None:
                lens = torch.full((B,), S, dtype=torch.int64, device=dev)
            else:
                lens = m[:, 1:].sum(1) + 1                                  # position 0 is always on
            ar = torch.arange(S, device=dev)
            idx = (lens.cumsum(0) - lens)[:, None] + ar[None, :]
            idx = torch.where(ar[None, :] < lens[:, None], idx, torch.full_like(idx, cap))   # the rest of a row: a spare slot
            tmp = torch.empty(cap + 1, dtype=torch.int32, device=dev)
            tmp.scatter_(0, idx.reshape(-1), paths.reshape(-1).to(torch.int32))
            tags.lens.copy_(lens)
            tags.tags_flat.copy_(tmp[:cap])
        else:
            rows = [list(r) for r in paths]
            if len(rows) != B or sum(len(r) for r in rows) > tags.capacity:
                raise ValueError("paths hold %d samples / %d tags for a batch of %d x %d"
                                 % (len(rows), sum(len(r) for r in rows), B, S))
            flat = [int(v) for r in rows for v in r]
            tags.lens.copy_(torch.tensor([len(r) for r in rows], dtype=torch.int32))
            if flat:
                tags.tags_flat[:len(flat)].copy_(torch.tensor(flat, dtype=torch.int32))

    def posterior(self, emissions: torch.Tensor, paths=None, mask: Optional[torch.Tensor] = None, *,
                  marginals: bool = False, label_table=None) -> "CrfPosterior":
        """How sure the model is of ``paths`` (default: of its own Viterbi paths): ``log_z``, ``seq_logp``, ``token_conf``
        and, with ``marginals=True``, the token marginals; with ``label_table`` (the words of ``metrics.label_table``) the
        chunks of every path and their exact posteriors.  The definitions are written out in include/icka_hip.h.  A path has
        one tag per on-position (position 0 and the positions with ``mask != 0``): what ``decode`` returns for the same mask.
        ``paths``: a ``DeviceTags``, an integer device tensor in the layout of the mask (the first L entries of each sample),
        per-sample lists, or None: then ``icka_crf_score_decode`` runs first (two launches in all).  Outside autograd, no host
        sync; a sample whose path does not fit its mask or holds a tag id outside [0, num_tags) is refused (NaN outputs,
        counted in ``bad``)."""
        e, _, m = self._prep(emissions.detach(), None, mask)
        self._arena()
        B, S, Cn = e.shape
        if S * Cn > K.CRF_MAX_SC or B > K.CRF_FLAT_MAX_B:
            raise ValueError("CRF.posterior: B <= %d and S * num_tags <= %d, got [%d, %d, %d]"
                             % (K.CRF_FLAT_MAX_B, K.CRF_MAX_SC, B, S, Cn))
        if m is not None:
            m[:, 0] = 1            # (m is _prep's own copy) position 0 is on: decode and posterior count the same path length
        if label_table is not None and not isinstance(label_table, torch.Tensor):
            label_table = torch.tensor(list(label_table), dtype=torch.int32).to(e.device)
        post = CrfPosterior(B, S, e.device, label_table is not None)
        post.bad.zero_()
        P = (self.start_transitions.detach(), self.end_transitions.detach(), self.transitions.detach())
        if paths is None:
            K.crf_score_decode(e, None, m, *P, None, post.tags.lens, post.tags.tags_flat)
        else:
            self._paths_into(post.tags, paths, m, B, S)
        mg = torch.empty(B, S, Cn, dtype=F32, device=e.device) if marginals else None
        K.crf_posterior(e, m, *P, post.log_z, post.bad, lens=post.tags.lens, tags_flat=post.tags.tags_flat,
                        seq_logp=post.seq_logp, token_conf=post.token_conf, marginals=mg, label_table=label_table,
                        ent=post.ent, ent_conf=post.ent_conf, n_ent=post.n_ent)
        if mg is not None:
            post.marginals = mg if self.batch_first else mg.transpose(0, 1)
        return post

    # ------------------------------------------------------------------------------------------------ constraints
    @staticmethod
    def allowed_from_tags(tags: torch.Tensor, num_tags: int, unknown_index: int = -1) -> torch.Tensor:
        """The allowed sets of partially labelled data, int64 bit sets in the shape of ``tags``: a known tag ``k`` becomes
        ``1 << k``, ``unknown_index`` becomes "every tag" (the low ``num_tags`` bits; -1 at 64 tags).  Pure torch: works on
        any device."""
        if not 1 <= num_tags <= 64:
            raise ValueError("allowed_from_tags: 1 <= num_tags <= 64, got %d" % num_tags)
        if not isinstance(tags, torch.Tensor) or tags.is_floating_point() or tags.dtype == torch.bool:
            raise ValueError("allowed_from_tags: tags must be an integer tensor, got %s"
                             % getattr(tags, "dtype", type(tags).__name__))
        t = tags.to(torch.int64)
        every = -1 if num_tags == 64 else (1 << num_tags) - 1
        one = torch.ones_like(t) << t.clamp(0, 63)          # 1 << 63 wraps to the sign bit: bit 63
        known = (t >= 0) & (t < num_tags) & (t != unknown_index)
        out = torch.where(known, one, torch.zeros_like(t))  # an id that names no tag allows nothing
        return torch.where(t == unknown_index, torch.full_like(t, every), out)

    @staticmethod
    def pack_allowed(allowed: torch.Tensor) -> torch.Tensor:
        """bool / uint8 [..., C] (non-zero = allowed) -> int64 [...] bit sets, bit j = tag j (C <= 64; tag 63 is the sign
        bit).  Layout work with torch ops on the tensor's own device."""
        if not isinstance(allowed, torch.Tensor) or allowed.dtype not in (torch.bool, torch.uint8) or allowed.dim() < 1:
            raise ValueError("pack_allowed: a bool or uint8 [..., C] tensor, got %s %s"
                             % (getattr(allowed, "dtype", type(allowed).__name__), tuple(getattr(allowed, "shape", ()))))
        Cn = allowed.shape[-1]
        if not 1 <= Cn <= 64:
            raise ValueError("pack_allowed: 1 <= C <= 64, got %d" % Cn)
        bits = torch.ones(Cn, dtype=torch.int64, device=allowed.device) << torch.arange(Cn, device=allowed.device)
        return ((allowed != 0).to(torch.int64) * bits).sum(-1)     # distinct bits: the sum is their union (wraps at bit 63)

    def _prep_allowed(self, who: str, emissions, allowed, mask):
        """The host-side checks of ``allowed`` (before any device check) -> (e, m, int64 [B,S] bit sets), batch-first, with
        position 0 of the mask forced on."""
        if not isinstance(allowed, torch.Tensor):
            raise ValueError("%s: allowed must be a tensor, got %s" % (who, type(allowed).__name__))
        if isinstance(emissions, torch.Tensor) and emissions.dim() == 3 and emissions.size(2) == self.num_tags:
            lead = tuple(emissions.shape[:2])
            if allowed.dtype == torch.int64:
                want = lead
            elif allowed.dtype in (torch.bool, torch.uint8):
                want = lead + (self.num_tags,)
            else:
                raise ValueError("%s: allowed must be int64 bit sets %s or bool / uint8 %s, got %s"
                                 % (who, lead, lead + (self.num_tags,), allowed.dtype))
            if tuple(allowed.shape) != want:
                raise ValueError("%s: allowed must have shape %s for %s, got %s"
                                 % (who, want, allowed.dtype, tuple(allowed.shape)))
            S = lead[1] if self.batch_first else lead[0]
            if S * self.num_tags > K.CRF_MAX_SC:
                raise ValueError("%s: S * num_tags <= %d, got %d * %d = %d"
                                 % (who, K.CRF_MAX_SC, S, self.num_tags, S * self.num_tags))
            if allowed.device != emissions.device:
                raise ValueError("%s: emissions on %s, allowed on %s" % (who, emissions.device, allowed.device))
        e, _, m = self._prep(emissions, None, mask)
        if allowed.dtype != torch.int64:
            allowed = self.pack_allowed(allowed)
        if not self.batch_first:
            allowed = allowed.transpose(0, 1)
        if m is not None:
            m[:, 0] = 1            # (m is _prep's own copy) position 0 is on, as in posterior
        return e, m, allowed.contiguous()

    def constrained_llh(self, emissions: torch.Tensor, allowed: torch.Tensor, mask: Optional[torch.Tensor] = None,
                        reduction: str = "sum") -> torch.Tensor:
        """The marginal log-likelihood of all tag paths inside per-position allowed sets, ``log Z_A - log Z`` (<= 0): the loss
        of partially labelled data (``-crf.constrained_llh(...)``).  Differentiable in ``emissions`` and the three
        parameters.  ``allowed``: int64 bit sets in the layout of the mask (bit j = tag j; ``allowed_from_tags`` builds them
        from labels with an unknown index), or a bool / uint8 tensor in the layout of the emissions.  The chain runs over
        position 0 and the positions with ``mask != 0``, as in ``posterior``; reductions as in ``forward``.  A sample with an
        empty set at one of its positions is infeasible: its value is ``-inf`` (so is a reduction over it) and its gradients
        are zeros.  No host sync.  The definitions are written out in include/icka_hip.h.  Posteriors, N-best and entity
        confidences under constraints, transition-level constraint arguments (write -1e4 into ``transitions``) and packed
        batches are not covered."""
        _check_reduction(reduction)
        e, m, al = self._prep_allowed("CRF.constrained_llh", emissions, allowed, mask)
        A = self._arena()
        llh = _CrfConstrainedFn.apply(A.anchor, e, al, m, self, A)
        return self._reduce(llh, m, e, reduction)

    def constrained_decode(self, emissions: torch.Tensor, allowed: torch.Tensor,
                           mask: Optional[torch.Tensor] = None) -> "ConstrainedPaths":
        """The most likely tag path inside per-position allowed sets (``allowed`` as in ``constrained_llh``): known tags are
        forced with singleton sets, excluded ones by clearing their bits.  Ties take the first maximum over the allowed
        tags, so with every tag allowed the paths are ``decode``'s.  An infeasible sample is reported, never decoded: -1
        tags, a ``-inf`` score, ``None`` in ``tolist()``, one more in ``infeasible``.  Detached, one launch, no host sync."""
        e, m, al = self._prep_allowed("CRF.constrained_decode", emissions.detach() if isinstance(emissions, torch.Tensor)
                                      else emissions, allowed, mask)
        self._arena()
        B, S, _ = e.shape
        if B > K.CRF_FLAT_MAX_B:
            raise ValueError("CRF.constrained_decode: B <= %d, got %d" % (K.CRF_FLAT_MAX_B, B))
        out = ConstrainedPaths(B, S, e.device)
        out.infeasible.zero_()
        K.crf_constrained_decode(e, m, al, self.start_transitions.detach(), self.end_transitions.detach(),
                                 self.transitions.detach(), out.tags.lens, out.tags.tags_flat, out.scores, out.infeasible)
        return out

    # ----------------------------------------------------------------------------------------------- expectations
    def _prep_expect(self, who: str, emissions, mask):
        """(e, m) batch-first with position 0 of the mask forced on, inside the limit of icka_crf_expect."""
        e, _, m = self._prep(emissions, None, mask)
        S = e.shape[1]
        if S * self.num_tags > K.CRF_EXPECT_MAX_SC:
            raise ValueError("%s: S * num_tags <= %d, got %d * %d = %d"
                             % (who, K.CRF_EXPECT_MAX_SC, S, self.num_tags, S * self.num_tags))
        if m is not None:
            m[:, 0] = 1            # (m is _prep's own copy) position 0 is on, as in posterior
        return e, m

    def _like_emissions(self, who: str, name: str, t, emissions) -> torch.Tensor:
        """``t`` (a second [.., .., C] tensor in the layout of ``emissions``) as contiguous f32 [B,S,C]"""
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError("%s: %s must be a floating-point tensor, got %s"
                             % (who, name, getattr(t, "dtype", type(t).__name__)))
        if isinstance(emissions, torch.Tensor) and tuple(t.shape) != tuple(emissions.shape):
            raise ValueError("%s: %s must have the shape of the emissions %s, got %s"
                             % (who, name, tuple(emissions.shape), tuple(t.shape)))
        if not self.batch_first:
            t = t.transpose(0, 1)
        return t.to(F32).contiguous()

    def log_partition(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``log Z`` per sample, f32 [B], differentiable in ``emissions`` and the three parameters (icka_crf_expect / _grad:
        one launch forward, one backward, no host sync).  The chain runs over position 0 and the positions with
        ``mask != 0``, as in ``posterior``."""
        e, m = self._prep_expect("CRF.log_partition", emissions, mask)
        A = self._arena()
        return _CrfExpectFn.apply(A.anchor, e, m, self, A, _ExpectCfg(True, False), None, None, None, None)[0]

    def entropy(self, emissions: torch.Tensor, mask: Optional[torch.Tensor] = None, reduction: str = "none") -> torch.Tensor:
        """The entropy of the distribution over tag paths, ``H = log Z - E_p[score(y)]`` (>= 0, at most ``L log num_tags``):
        the uncertainty measure of active learning and the entropy-minimisation term on unlabelled data.  Differentiable in
        ``emissions`` and the three parameters: one launch forward, one backward, no host sync.  The chain runs over position
        0 and the positions with ``mask != 0``, as in ``posterior``; reductions as in ``forward``.  Limit:
        ``S * num_tags <= 4096``.  Constraints and packed batches are not covered."""
        _check_reduction(reduction)
        e, m = self._prep_expect("CRF.entropy", emissions, mask)
        A = self._arena()
        log_z, ex = _CrfExpectFn.apply(A.anchor, e, m, self, A, _ExpectCfg(True, True), None, None, None, None)
        return self._reduce(log_z - ex, m, e, reduction)

    def kl_divergence(self, emissions: torch.Tensor, other_emissions: torch.Tensor, mask: Optional[torch.Tensor] = None,
                      other: Optional["CRF"] = None, detach: str = "none", reduction: str = "none") -> torch.Tensor:
        """``KL(p || q)`` between two CRF distributions over the tag paths of the same sentences: ``p`` is this module on
        ``emissions``, ``q`` is ``other`` (a CRF with the same ``num_tags``; default: this module, two views through one CRF)
        on ``other_emissions``.  Differentiable on both sides; ``detach="self"`` / ``"other"`` gives that side no gradient and
        skips its gradient work (a detached teacher, a stop-gradient view).  Two launches forward and two backward
        (``E_p[s_p - s_q]`` and ``log Z_p``, then ``log Z_q``), no host sync.  Mask, reductions and limits as in ``entropy``."""
        who = "CRF.kl_divergence"
        _check_reduction(reduction)
        if detach not in ("none", "self", "other"):
            raise ValueError("%s: detach must be 'none', 'self' or 'other', got %r" % (who, detach))
        q = self if other is None else other
        if not isinstance(q, CRF) or q.num_tags != self.num_tags:
            raise ValueError("%s: other must be a CRF with num_tags = %d, got %s"
                             % (who, self.num_tags, q if isinstance(q, CRF) else type(q).__name__))
        e2 = self._like_emissions(who, "other_emissions", other_emissions, emissions)
        if detach == "self" and isinstance(emissions, torch.Tensor):
            emissions = emissions.detach()
        if detach == "other":
            e2 = e2.detach()
        e, m = self._prep_expect(who, emissions, mask)
        A, Aq = self._arena(), q._arena()
        cfg = _ExpectCfg(True, True, other=q, A_other=Aq, first_grad=detach != "self", second_grad=detach != "other")
        log_zp, ex = _CrfExpectFn.apply(A.anchor, e, m, self, A, cfg, e2, None, None, None)
        if detach == "other":
            log_zq = K.crf_expect(e2, m, *_params(q), torch.empty_like(log_zp))
        else:
            log_zq = _CrfExpectFn.apply(Aq.anchor, e2, m, q, Aq, _ExpectCfg(True, False), None, None, None, None)[0]
        return self._reduce(ex - log_zp + log_zq, m, e, reduction)

    def expected(self, emissions: torch.Tensor, payoff: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                 payoff_start: Optional[torch.Tensor] = None, payoff_end: Optional[torch.Tensor] = None,
                 payoff_transitions: Optional[torch.Tensor] = None, reduction: str = "none") -> torch.Tensor:
        """``E_p[r(y)]`` of a path-additive payoff: ``payoff`` in the layout of ``emissions`` scores tag j at position t,
        ``payoff_start`` / ``payoff_end`` [num_tags] the first / last tag and ``payoff_transitions`` [num_tags, num_tags] every
        transition (each optional: zeros).  Differentiable in ``emissions``, the three parameters and every payoff tensor
        (those through ordinary autograd): one launch forward, one backward, no host sync.  Mask, reductions and limits as in
        ``entropy``."""
        who = "CRF.expected"
        _check_reduction(reduction)
        g = self._like_emissions(who, "payoff", payoff, emissions)
        parts = []
        for name, t, shape in (("payoff_start", payoff_start, (self.num_tags,)), ("payoff_end", payoff_end, (self.num_tags,)),
                               ("payoff_transitions", payoff_transitions, (self.num_tags, self.num_tags))):
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_floating_point() or tuple(t.shape) != shape):
                raise ValueError("%s: %s must be a floating-point tensor of shape %s, got %s %s"
                                 % (who, name, shape, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))
            parts.append(None if t is None else t.to(F32).contiguous())
        e, m = self._prep_expect(who, emissions, mask)
        A = self._arena()
        ex = _CrfExpectFn.apply(A.anchor, e, m, self, A, _ExpectCfg(False, True), g, *parts)[1]
        return self._reduce(ex, m, e, reduction)

    def expected_cost(self, emissions: torch.Tensor, tags: torch.Tensor, mask: Optional[torch.Tensor] = None,
                      cost: Optional[torch.Tensor] = None, reduction: str = "none") -> torch.Tensor:
        """The expected cost of the model's tag path against ``tags``: ``sum_t E_p[cost[tags_t, y_t]]`` over the chain's
        positions.  ``cost``: f32 [num_tags, num_tags] (gold, predicted); default ``1 - I``, the expected number of wrong tags
        (minimum-risk training, a calibrated error estimate).  ``expected`` with ``payoff = cost[tags]``; tag ids are clamped
        into [0, num_tags) where they are read, so positions that are off may carry pad labels."""
        who = "CRF.expected_cost"
        Cn = self.num_tags
        if not isinstance(tags, torch.Tensor) or tags.is_floating_point() or tags.dtype == torch.bool:
            raise ValueError("%s: tags must be an integer tensor, got %s" % (who, getattr(tags, "dtype", type(tags).__name__)))
        if isinstance(emissions, torch.Tensor) and tuple(tags.shape) != tuple(emissions.shape[:2]):
            raise ValueError("%s: the first two dimensions of emissions and tags must match, got %s and %s"
                             % (who, tuple(emissions.shape[:2]), tuple(tags.shape)))
        if cost is None:
            cost = 1.0 - torch.eye(Cn, dtype=F32, device=tags.device)
        elif not isinstance(cost, torch.Tensor) or cost.dtype != F32 or tuple(cost.shape) != (Cn, Cn):
            raise ValueError("%s: cost must be an f32 tensor of shape %s, got %s %s"
                             % (who, (Cn, Cn), getattr(cost, "dtype", type(cost).__name__), tuple(getattr(cost, "shape", ()))))
        if cost.device != tags.device:
            raise ValueError("%s: tags on %s, cost on %s" % (who, tags.device, cost.device))
        return self.expected(emissions, cost[tags.to(torch.int64).clamp(0, Cn - 1)], mask, reduction=reduction)


class _JointBuffer(object):
    """Named fields back to back in ONE int32 buffer, so that a result object reaches the host in one copy.  ``sizes``:
    ``[(name, n_words)]`` in buffer order; ``slices[name]`` is a field's (first, past-the-last) word, ``joint`` the buffer."""

    def __init__(self, sizes, device):
        self.slices, o = {}, 0
        for name, n in sizes:
            self.slices[name] = (o, o + n)
            o += n
        self.joint = torch.empty(o, dtype=torch.int32, device=device)

    def part(self, name: str, h: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The words of field ``name`` as a view of ``joint`` or, given one, of a host copy ``h`` of it."""
        a, b = self.slices[name]
        return (self.joint if h is None else h)[a:b]

    def host(self) -> dict:
        """``unpack`` of the one device-to-host copy of ``joint`` (a host sync)."""
        return self.unpack(self.joint.cpu())


class ConstrainedPaths(_JointBuffer):
    """The outputs of ``CRF.constrained_decode`` on the device, in ONE buffer (``joint``, int32 words; ``scores`` is an f32
    view of it) so that ``host()`` is one device-to-host copy:

        infeasible int32 [1] | lens int32 [B] | tags_flat int32 [B*S] | scores f32 [B]

    ``tags`` is a ``DeviceTags`` view of lens + tags_flat, which ``CRF.posterior(paths=...)`` and ``metrics.ChunkEvaluator``
    take as it is.  An infeasible sample holds -1 in its ``lens[b]`` slots and ``scores[b] = -inf``."""

    def __init__(self, B: int, S: int, device):
        cap = B * S
        super().__init__([("infeasible", 1), ("lens", B), ("tags_flat", cap), ("scores", B)], device)
        part = self.part
        self.batch_size, self.capacity = B, cap
        self.infeasible = part("infeasible")
        self.tags = DeviceTags(part("lens"), part("tags_flat"))
        self.scores = part("scores").view(F32)

    def unpack(self, h: torch.Tensor) -> dict:
        """What ``host()`` returns, from a host copy ``h`` of ``joint`` (the caller's own, as part of a larger copy):
        ``infeasible``, ``lens``, ``scores`` and ``paths`` (per sample a list of tags, None for an infeasible sample)."""
        lens, flat = self.part("lens", h).tolist(), self.part("tags_flat", h).tolist()
        paths = [None if (p and p[0] < 0) else p for p in split_tags(lens, flat)]
        return {"infeasible": int(self.part("infeasible", h)[0]), "lens": lens,
                "scores": self.part("scores", h).view(F32).tolist(), "paths": paths}

    def tolist(self) -> List[Optional[List[int]]]:
        """Per sample its path, or None for an infeasible sample (one device-to-host copy)."""
        return self.host()["paths"]

    def __repr__(self) -> str:
        return "ConstrainedPaths(batch=%d, capacity=%d, device=%s)" % (self.batch_size, self.capacity, self.joint.device)


class CrfPosterior(_JointBuffer):
    """The outputs of ``CRF.posterior`` on the device, all but the marginals in ONE buffer (``joint``, int32 words; the f32
    fields are views of it) so that ``host()`` is one device-to-host copy:

        bad int32 [1] | tags.lens int32 [B] | tags.tags_flat int32 [B*S] | n_ent int32 [B] | ent int32 [B*S, 3] |
        log_z f32 [B] | seq_logp f32 [B] | token_conf f32 [B*S] | ent_conf f32 [B*S]

    ``tags`` is a ``DeviceTags``; ``token_conf`` is aligned with ``tags.tags_flat``; chunk k of sample b sits at row
    ``sum(lens[:b]) + k`` of ``ent`` (type id, start, end exclusive; path coordinates) and ``ent_conf``, ``n_ent[b]`` rows per
    sample (only with a label table: else these three are None).  ``marginals``: None unless asked for."""

    def __init__(self, B: int, S: int, device, entities: bool):
        cap = B * S
        super().__init__([("bad", 1), ("lens", B), ("tags_flat", cap), ("n_ent", B if entities else 0),
                          ("ent", 3 * cap if entities else 0), ("log_z", B), ("seq_logp", B), ("token_conf", cap),
                          ("ent_conf", cap if entities else 0)], device)
        part = self.part
        self.batch_size, self.capacity = B, cap
        self.bad = part("bad")
        self.tags = DeviceTags(part("lens"), part("tags_flat"))
        self.log_z, self.seq_logp, self.token_conf = (part(n).view(F32) for n in ("log_z", "seq_logp", "token_conf"))
        self.n_ent = part("n_ent") if entities else None
        self.ent = part("ent").view(cap, 3) if entities else None
        self.ent_conf = part("ent_conf").view(F32) if entities else None
        self.marginals = None

    def host(self) -> dict:
        """Everything but the marginals on the host, as python lists keyed by field name: the one device-to-host copy (a host
        sync).  Runs the check the producer of the paths deferred, if any."""
        h = self.joint.cpu()
        if self.tags.deferred_check is not None:
            self.tags.deferred_check()
        return self.unpack(h)

    def unpack(self, h: torch.Tensor) -> dict:
        """``host()`` of a host copy ``h`` of ``joint`` the caller made (as part of a larger copy)."""
        out = {}
        for name in self.slices:
            w = self.part(name, h)
            out[name] = (w.view(F32) if name in ("log_z", "seq_logp", "token_conf", "ent_conf") else w).tolist()
        out["bad"] = out["bad"][0]
        return out

    def __repr__(self) -> str:
        return "CrfPosterior(batch=%d, capacity=%d, entities=%s, device=%s)" % (
            self.batch_size, self.capacity, self.ent is not None, self.joint.device)


class NBestPaths(_JointBuffer):
    """The outputs of ``CRF.decode_nbest`` on the device, in ONE buffer (``joint``, int32 words; ``scores`` is an f32 view of
    it) so that ``host()`` is one device-to-host copy:

        lens int32 [B] | n_paths int32 [B] | scores f32 [B, nbest] | tags int32 [nbest, B*S]

    ``lens[b]`` is the length of every path of sample b, ``n_paths[b]`` how many ranks it has (``min(nbest, num_tags ** L)``),
    ``scores[b, r]`` the score of rank r (-inf past ``n_paths[b]``, non-increasing in r) and row r of ``tags`` holds rank r of
    all samples back to back, sample b at ``sum(lens[:b])`` (-1 at the ranks a sample does not have): ``rank(r)`` is a
    ``DeviceTags`` view of it."""

    def __init__(self, B: int, S: int, nbest: int, device):
        cap = B * S
        super().__init__([("lens", B), ("n_paths", B), ("scores", B * nbest), ("tags", nbest * cap)], device)
        part = self.part
        self.batch_size, self.capacity, self.nbest = B, cap, nbest
        self.lens, self.n_paths = part("lens"), part("n_paths")
        self.scores = part("scores").view(F32).view(B, nbest)
        self.tags = part("tags").view(nbest, cap)

    def rank(self, r: int) -> DeviceTags:
        """Rank ``r`` of every sample as a ``DeviceTags`` (a view: no copy), which ``CRF.posterior(paths=...)`` and
        ``metrics.ChunkEvaluator`` take as it is.  A sample with ``n_paths[b] <= r`` holds -1 there (the posterior kernel
        refuses such a path and counts it in ``bad``)."""
        if not 0 <= r < self.nbest:
            raise IndexError("rank %d of %d" % (r, self.nbest))
        return DeviceTags(self.lens, self.tags[r])

    def log_probs(self, log_z: torch.Tensor) -> torch.Tensor:
        """``scores - log_z[:, None]`` on the device, f32 [B, nbest]: the log-probability of every rank (-inf at the ranks a
        sample does not have), given ``log_z`` of the same emissions and mask (``CRF.posterior(...).log_z``)."""
        if tuple(log_z.shape) != (self.batch_size,):
            raise ValueError("log_z must have shape (%d,), got %s" % (self.batch_size, tuple(log_z.shape)))
        return self.scores - log_z.to(F32)[:, None]

    def unpack(self, h: torch.Tensor) -> dict:
        """What ``host()`` returns, from a host copy ``h`` of ``joint`` (the caller's own, as part of a larger copy):
        python lists keyed by field name, ``scores`` and ``tags`` nested by row."""
        return {"lens": self.part("lens", h).tolist(), "n_paths": self.part("n_paths", h).tolist(),
                "scores": self.part("scores", h).view(F32).view(self.batch_size, self.nbest).tolist(),
                "tags": self.part("tags", h).view(self.nbest, self.capacity).tolist()}

    @staticmethod
    def paths_of(h: dict) -> List[List[tuple]]:
        """Per sample the list of ``(path, score)`` of its ``n_paths[b]`` ranks from the dict of ``host()``."""
        out, o = [], 0
        for b, n in enumerate(h["lens"]):
            out.append([(h["tags"][r][o:o + n], h["scores"][b][r]) for r in range(h["n_paths"][b])])
            o += n
        return out

    def tolist(self) -> List[List[tuple]]:
        """Per sample a list of ``n_paths[b]`` pairs ``(path, score)``, best first (one device-to-host copy)."""
        return self.paths_of(self.host())

    def __repr__(self) -> str:
        return "NBestPaths(batch=%d, nbest=%d, capacity=%d, device=%s)" % (
            self.batch_size, self.nbest, self.capacity, self.joint.device)


class SampledPaths(_JointBuffer):
    """The outputs of ``CRF.sample`` on the device, in ONE buffer (``joint``, int32 words; ``log_z`` and ``scores`` are f32 views
    of it) so that ``host()`` is one device-to-host copy:

        lens int32 [B] | log_z f32 [B] | scores f32 [B, num_samples] | tags int32 [num_samples, B*S]

    ``lens[b]`` is the length of every draw of sample b, ``scores[b, k]`` the score of draw k and row k of ``tags`` holds draw k
    of all samples back to back, sample b at ``sum(lens[:b])``: ``draw(k)`` is a ``DeviceTags`` view of it."""

    def __init__(self, B: int, S: int, num_samples: int, device):
        cap = B * S
        super().__init__([("lens", B), ("log_z", B), ("scores", B * num_samples), ("tags", num_samples * cap)], device)
        part = self.part
        self.batch_size, self.capacity, self.num_samples = B, cap, num_samples
        self.lens = part("lens")
        self.log_z = part("log_z").view(F32)
        self.scores = part("scores").view(F32).view(B, num_samples)
        self.tags = part("tags").view(num_samples, cap)

    def draw(self, k: int) -> DeviceTags:
        """Draw ``k`` of every sample as a ``DeviceTags`` (a view: no copy), which ``CRF.posterior(paths=...)``,
        ``CRF.path_llh`` and ``metrics.ChunkEvaluator`` take as it is."""
        if not 0 <= k < self.num_samples:
            raise IndexError("draw %d of %d" % (k, self.num_samples))
        return DeviceTags(self.lens, self.tags[k])

    def log_probs(self) -> torch.Tensor:
        """``scores - log_z[:, None]`` on the device, f32 [B, num_samples]: the log-probability of every draw."""
        return self.scores - self.log_z[:, None]

    def unpack(self, h: torch.Tensor) -> dict:
        """What ``host()`` returns, from a host copy ``h`` of ``joint`` (the caller's own, as part of a larger copy):
        python lists keyed by field name, ``scores`` and ``tags`` nested by row."""
        return {"lens": self.part("lens", h).tolist(), "log_z": self.part("log_z", h).view(F32).tolist(),
                "scores": self.part("scores", h).view(F32).view(self.batch_size, self.num_samples).tolist(),
                "tags": self.part("tags", h).view(self.num_samples, self.capacity).tolist()}

    def tolist(self) -> List[List[tuple]]:
        """Per sample a list of ``num_samples`` pairs ``(path, log_prob)`` in draw order (one device-to-host copy)."""
        h = self.host()
        out, o = [], 0
        for b, n in enumerate(h["lens"]):
            out.append([(h["tags"][k][o:o + n], h["scores"][b][k] - h["log_z"][b]) for k in range(self.num_samples)])
            o += n
        return out

    def __repr__(self) -> str:
        return "SampledPaths(batch=%d, num_samples=%d, capacity=%d, device=%s)" % (
            self.batch_size, self.num_samples, self.capacity, self.joint.device)


def minimum_risk(logp: torch.Tensor, cost: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """The risk of a candidate set, f32 [B]: ``sum_r q_r cost_r`` with ``q = softmax_r(scale * logp)`` over the rows with
    finite ``logp`` ([B, R]: ``CRF.path_llh``; ``cost`` [B, R]: ``metrics.f1_cost``).  A row with a non-finite ``logp`` (a
    missing rank) has no weight and passes no gradient; a sample with no finite row returns 0.  Plain torch."""
    if logp.dim() != 2 or tuple(cost.shape) != tuple(logp.shape):
        raise ValueError("minimum_risk: logp and cost must both be [B, R], got %s and %s" % (tuple(logp.shape), tuple(cost.shape)))
    finite = torch.isfinite(logp)
    some = finite.any(1, keepdim=True)
    z = torch.where(finite, logp * scale, torch.full_like(logp, float("-inf")))
    z = torch.where(some, z, torch.zeros_like(z))               # (a softmax over nothing but -inf would be NaN)
    q = torch.where(finite, torch.softmax(z, 1), torch.zeros_like(z))
    return (q * torch.where(finite, cost.to(logp.dtype), torch.zeros_like(logp))).sum(1)
