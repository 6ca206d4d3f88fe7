"""Chunk-level accuracy / precision / recall / F1 of the dev and test passes, scored on the device.

The number the reference trains FOR -- it decides which checkpoint is kept (My_cross_attention.py:913-917, :1089) -- comes from a
per-token Python loop over every sample (:882-903) and from ``ner_evaluate.py`` (``get_chunks`` :4-48, ``evaluate`` :64-110,
``evaluate_each_class`` :112-148).  ``ChunkEvaluator`` keeps the counts behind it in a device table that one launch of
``icka_chunk_eval`` per batch adds to (csrc/metrics.hip; the rules are written out in include/icka_hip.h), so a whole dev epoch
costs ONE host sync, in ``compute()``.  ``chunks`` and ``evaluate_lists`` restate the same rules in plain Python: what the tests
pin the kernel to, and the scorer for a caller whose predictions are python lists and who has no device tensor.

The rules.  A label map gives every tag id a name; ``name.split('-')[0] == "B"`` makes it a begin tag, ``name.split('-')[-1]``
is its type (so ``"PAD"``, ``"X"``, ``"[CLS]"`` are types of their own), the id named ``default`` (``"O"``) is outside every
chunk.  On a sequence of ids, with O(i) = default, t(i) = type: ``start(i) = !O(i) and (i == 0 or O(i-1) or t(i) != t(i-1) or
B(i))``, ``term(i) = O(i) or start(i)``; a chunk begins at every start, has that token's type and ends at the next term or at
the end of the sequence.  A predicted chunk is correct when the gold sequence has the same (type, start, end)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import kernels as K

DEFAULT_SKIP = ("X", "</s>", "<s>", "[CLS]", "[SEP]")      # My_cross_attention.py:891-893: gold labels the loop drops
# MNERProcessor.get_labels (My_cross_attention.py:215): the names of the reference's tag ids 1 .. 14 (id 0 = "PAD")
REFERENCE_LABEL_LIST = ("O", "B-MISC", "I-MISC", "B-PER", "I-PER", "B-ORG", "I-ORG", "B-LOC", "I-LOC", "X", "[CLS]", "[SEP]",
                        "<s>", "</s>")
LT_DEFAULT, LT_BEGIN, LT_SKIP, LT_TYPE_SHIFT = 1, 2, 4, 8   # bits of a label_table word (include/icka_hip.h)
HEAD = K.CHUNK_EVAL_HEAD                                    # kept, equal, correct_preds, total_preds, total_correct, bad_ids


def label_names(id_to_label) -> List[str]:
    """The names of ids 0 .. L-1 as a list, from a ``{id: name}`` dict (every id from 0 to its largest) or a sequence."""
    if isinstance(id_to_label, dict):
        n = len(id_to_label)
        if sorted(id_to_label) != list(range(n)):
            raise ValueError("the label map must name every id from 0 to %d, got ids %s" % (n - 1, sorted(id_to_label)))
        names = [id_to_label[i] for i in range(n)]
    else:
        names = list(id_to_label)
    if not names or not all(isinstance(s, str) for s in names):
        raise ValueError("the label map must hold at least one name, all strings")
    return names


def label_list_map(label_list: Sequence[str]) -> Dict[int, str]:
    """The reference's id -> name map of a label list: ``{0: "PAD", 1: label_list[0], ...}`` (My_cross_attention.py:859-860)."""
    m = {i: name for i, name in enumerate(label_list, 1)}
    m[0] = "PAD"
    return m


def label_table(id_to_label, default: str = "O", skip: Sequence[str] = DEFAULT_SKIP) -> Tuple[List[int], List[str]]:
    """(one ``label_table`` word per tag id, type names by type id) -- the operand of ``icka_chunk_eval``.  Type ids are given
    in the order the types first appear among the ids."""
    names = label_names(id_to_label)
    if default not in names:
        raise ValueError("the default tag %r is not in the label map %s" % (default, names))
    if len(names) > K.CHUNK_EVAL_MAX_IDS:
        raise ValueError("%d tag ids: the scorer takes at most %d" % (len(names), K.CHUNK_EVAL_MAX_IDS))
    types: List[str] = []
    words = []
    for name in names:
        ty = name.split("-")[-1]
        if ty not in types:
            types.append(ty)
        w = types.index(ty) << LT_TYPE_SHIFT
        if name == default:
            w |= LT_DEFAULT
        if name.split("-")[0] == "B":
            w |= LT_BEGIN
        if name in skip:
            w |= LT_SKIP
        words.append(w)
    if len(types) > K.CHUNK_EVAL_MAX_TYPES:
        raise ValueError("%d chunk types: the scorer takes at most %d" % (len(types), K.CHUNK_EVAL_MAX_TYPES))
    return words, types


def chunks(seq: Sequence[int], id_to_label, default: str = "O") -> List[Tuple[str, int, int]]:
    """The ``(type, start, end)`` chunks of a sequence of tag ids (end exclusive), by the rules of the module docstring."""
    names = label_names(id_to_label)
    out: List[Tuple[str, int, int]] = []
    open_type, open_at = None, 0
    prev_o, prev_type = True, None
    for i, tok in enumerate(seq):
        name = names[tok]
        o = name == default
        ty = name.split("-")[-1]
        start = (not o) and (prev_o or ty != prev_type or name.split("-")[0] == "B")
        if (o or start) and open_type is not None:
            out.append((open_type, open_at, i))
            open_type = None
        if start:
            open_type, open_at = ty, i
        prev_o, prev_type = o, ty
    if open_type is not None:
        out.append((open_type, open_at, len(seq)))
    return out


def filter_batch(pred, labels, output_mask, id_to_label, skip: Sequence[str] = DEFAULT_SKIP):
    """(pred_lists, gold_lists) of one batch as the reference's loop makes them (My_cross_attention.py:882-903): per sample
    the positions before the first zero of ``output_mask`` whose GOLD label is not in ``skip``; the prediction at position j
    is ``pred[b][j]``.  ``pred``: per-sample lists (what ``CRF.decode`` returns); ``labels`` / ``output_mask``: [B, S] lists,
    arrays or tensors."""
    names = label_names(id_to_label)
    labels = labels.tolist() if hasattr(labels, "tolist") else labels
    output_mask = output_mask.tolist() if hasattr(output_mask, "tolist") else output_mask
    pl, gl = [], []
    for b, mask in enumerate(output_mask):
        p, g = [], []
        for j, m in enumerate(mask):
            if not m:
                break
            if names[labels[b][j]] not in skip:
                g.append(int(labels[b][j]))
                p.append(int(pred[b][j]))
        pl.append(p)
        gl.append(g)
    return pl, gl


def _ratio_scores(correct: int, preds: int, golds: int) -> Tuple[float, float, float]:
    """(f1, p, r) with the reference's expressions (ner_evaluate.py:104-106, :144-146), in float64."""
    p = correct / preds if correct > 0 else 0
    r = correct / golds if correct > 0 else 0
    f1 = 2 * p * r / (p + r) if correct > 0 else 0
    return f1, p, r


class ChunkScores(object):
    """What a scorer returns.  Unpacks as the reference's ``evaluate``: ``acc, f1, p, r = scores``.  ``counts`` = {kept_tokens,
    equal_tokens, correct_preds, total_preds, total_correct}; ``per_class[type] = (f1, p, r)`` (``evaluate_each_class``) and
    ``per_class_counts[type] = (correct, preds, golds)`` for every type of the label map but the default tag's; ``mean_loss``
    (None when no loss was accumulated)."""

    def __init__(self, counts: Dict[str, int], type_counts: Dict[str, Tuple[int, int, int]], mean_loss: Optional[float] = None):
        self.counts = dict(counts)
        self.per_class_counts = dict(type_counts)
        self.f1, self.p, self.r = _ratio_scores(counts["correct_preds"], counts["total_preds"], counts["total_correct"])
        kept = counts["kept_tokens"]
        self.acc = counts["equal_tokens"] / kept if kept > 0 else float("nan")     # (the reference's np.mean([]) is nan)
        self.per_class = {t: _ratio_scores(*c) for t, c in type_counts.items()}
        self.mean_loss = mean_loss

    def __iter__(self):
        return iter((self.acc, self.f1, self.p, self.r))

    def __repr__(self) -> str:
        return "ChunkScores(acc=%r, f1=%r, p=%r, r=%r, counts=%r)" % (self.acc, self.f1, self.p, self.r, self.counts)


def _scores_from_table(table: Sequence[int], types: Sequence[str], default_type: str, mean_loss=None) -> ChunkScores:
    counts = dict(zip(("kept_tokens", "equal_tokens", "correct_preds", "total_preds", "total_correct"), (int(v) for v in table)))
    tc = {t: tuple(int(v) for v in table[HEAD + 3 * i:HEAD + 3 * i + 3]) for i, t in enumerate(types) if t != default_type}
    return ChunkScores(counts, tc, mean_loss)


def evaluate_lists(pred: Sequence[Sequence[int]], gold: Sequence[Sequence[int]], id_to_label, default: str = "O") -> ChunkScores:
    """Score filtered per-sample id lists (``filter_batch``) on the host: the reference's ``evaluate`` and, per type, its
    ``evaluate_each_class``, restated over ``chunks``."""
    _, types = label_table(id_to_label, default, ())
    table = [0] * (HEAD + 3 * len(types))
    for p, g in zip(pred, gold):
        n = min(len(p), len(g))
        table[0] += n
        table[1] += sum(1 for a, b in zip(g, p) if a == b)
        gc, pc = set(chunks(g, id_to_label, default)), set(chunks(p, id_to_label, default))
        table[2] += len(gc & pc)
        table[3] += len(pc)
        table[4] += len(gc)
        for i, t in enumerate(types):
            pt = {c for c in pc if c[0] == t}
            table[HEAD + 3 * i] += len(pt & gc)
            table[HEAD + 3 * i + 1] += len(pt)
            table[HEAD + 3 * i + 2] += len({c for c in gc if c[0] == t})
    return _scores_from_table(table, types, default.split("-")[-1])


def f1_cost(counts: torch.Tensor) -> torch.Tensor:
    """``1 - F1`` of every candidate path, f32 [B, R], from ``ChunkEvaluator.path_counts``'s int32 [R, B, 4]:
    ``1 - 2 c / (p + g)`` with c = correct_preds, p = total_preds, g = total_correct; 0 where ``p + g == 0`` (nothing to find,
    nothing predicted), 1 for a bad sample.  Plain torch on the tensor's own device, no host sync."""
    if not isinstance(counts, torch.Tensor) or counts.dim() != 3 or counts.shape[2] != 4 or counts.is_floating_point():
        raise ValueError("f1_cost: counts must be an integer [R, B, 4] tensor, got %s %s"
                         % (getattr(counts, "dtype", type(counts).__name__), tuple(getattr(counts, "shape", ()))))
    c, p, g, bad = (counts[..., i].to(torch.float32) for i in range(4))
    n = p + g
    cost = torch.where(n > 0, 1.0 - 2.0 * c / n.clamp(min=1.0), torch.zeros_like(n))
    return torch.where(bad != 0, torch.ones_like(cost), cost).transpose(0, 1).contiguous()


class ChunkEvaluator(object):
    """Accumulates the chunk-level counts of a dev / test epoch on the device.

        ev = ChunkEvaluator.for_label_list(label_list)
        for batch in dev_dataloader:
            tags, loss = model(..., labels=label_ids, mode="dev")        # GraphedModule(decode="device"): DeviceTags, loss
            ev.update(tags, label_ids, all_output_mask); ev.add_loss(loss)   # two launches, no sync
        acc, f1, p, r = scores = ev.compute()                             # the one device-to-host copy

    ``counters`` is the device table (int64: kept_tokens, equal_tokens, correct_preds, total_preds, total_correct, bad_ids,
    then (correct, preds, golds) per type id); a data-parallel caller all-reduces it before ``compute()``."""

    def __init__(self, id_to_label, default: str = "O", skip: Sequence[str] = DEFAULT_SKIP, device=None):
        self.names = label_names(id_to_label)
        self.id_to_label = dict(enumerate(self.names))
        self.default, self.skip = default, tuple(skip)
        self.table_words, self.types = label_table(self.names, default, self.skip)
        self.device = torch.device(device) if device is not None else None
        self._buf = None
        self._checks = {}

    @classmethod
    def for_label_list(cls, label_list: Sequence[str], **kw) -> "ChunkEvaluator":
        return cls(label_list_map(label_list), **kw)

    def _ensure(self, device=None) -> None:
        if self._buf is not None:
            return
        if self.device is None:
            self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        n = HEAD + 3 * len(self.types)
        self._buf = torch.zeros(n + 2, dtype=torch.int64, device=self.device)     # the table, then the f64 loss sum and count
        self._loss_acc = self._buf[n:].view(torch.float64)
        self._table = torch.tensor(self.table_words, dtype=torch.int32, device=self.device)

    @property
    def counters(self) -> torch.Tensor:
        self._ensure()
        return self._buf[:HEAD + 3 * len(self.types)]

    def _i64(self, t, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        if t.is_floating_point() or t.dim() != 2:
            raise ValueError("%s must be an integer [B, S] tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
        return t.to(device=self.device, dtype=torch.int64).contiguous()

    def update(self, pred, labels, output_mask) -> None:
        """Add one batch: ``pred`` a ``crf.DeviceTags``, a device integer tensor [B, S] or per-sample python lists (uploaded;
        a list shorter than its sample's kept range counts as ``bad_ids``).  One launch, no host sync; reads its operands in
        stream order, so the static outputs of a ``GraphedModule(decode="device")`` replay may be overwritten by the next."""
        from .crf import DeviceTags
        self._ensure(labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else None)
        labels = self._i64(labels, "labels")
        output_mask = self._i64(output_mask, "output_mask")
        kw = {}
        if isinstance(pred, DeviceTags):
            kw = {"lens": pred.lens, "tags_flat": pred.tags_flat}
            if pred.deferred_check is not None:
                self._checks[id(pred.deferred_check)] = pred.deferred_check
        elif isinstance(pred, torch.Tensor):
            kw = {"pred": self._i64(pred, "pred")}
        else:
            B, S = labels.shape
            if len(pred) != B:
                raise ValueError("pred holds %d samples for a batch of %d" % (len(pred), B))
            rows = [(list(r)[:S] + [-1] * S)[:S] for r in pred]
            kw = {"pred": torch.tensor(rows, dtype=torch.int64).reshape(B, S).to(self.device)}
        K.chunk_eval(labels, output_mask, self._table, self.counters, len(self.types), **kw)

    def path_counts(self, paths, labels, output_mask) -> torch.Tensor:
        """The chunk counts of every candidate path of every sample, int32 [R, B, 4] = (correct_preds, total_preds,
        total_correct, bad) on the device (``icka_chunk_counts``): ``paths`` a ``crf.DeviceTags`` (R = 1), ``crf.NBestPaths``
        or ``crf.SampledPaths`` (one row per rank / draw).  The rules are ``update``'s; nothing is added to ``counters``.  A
        sample ``update`` would count as ``bad_ids`` -- a rank an N-best sample does not have (-1 tags) among them -- gets
        (0, 0, 0, 1).  One launch, no host sync; ``f1_cost`` turns the result into a per-candidate cost."""
        from .crf import DeviceTags, NBestPaths, SampledPaths
        self._ensure(labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else None)
        labels = self._i64(labels, "labels")
        output_mask = self._i64(output_mask, "output_mask")
        if isinstance(paths, DeviceTags):
            lens, rows = paths.lens, paths.tags_flat[None, :]
        elif isinstance(paths, (NBestPaths, SampledPaths)):
            lens, rows = paths.lens, paths.tags
        else:
            raise ValueError("path_counts: paths must be a DeviceTags, NBestPaths or SampledPaths, got %s" % type(paths).__name__)
        counts = torch.empty(rows.shape[0], labels.shape[0], 4, dtype=torch.int32, device=self.device)
        return K.chunk_counts(lens, rows, labels, output_mask, self._table, counts, len(self.types))

    def add_loss(self, loss: torch.Tensor) -> None:
        """``dev_total_loss += loss.item(); index += 1`` (My_cross_attention.py:877-878) on the device, in float64: the f32
        loss converts exactly and the adds run in call order, so ``mean_loss`` is bitwise the reference loop's."""
        self._ensure(loss.device)
        loss = loss.detach()
        K.loss_accumulate(loss if loss.dtype == torch.float32 else loss.float(), self._loss_acc)

    def compute(self) -> ChunkScores:
        """Read the table back (the one host sync), run the checks deferred by the producers of the predictions, and turn the
        integer counts into the reference's floats.  Raises ValueError when a sample was refused (``bad_ids``)."""
        self._ensure()
        h = self._buf.cpu()
        for chk in list(self._checks.values()):
            chk()
        n = HEAD + 3 * len(self.types)
        table = h[:n].tolist()
        loss_sum, loss_n = h[n:].view(torch.float64).tolist()
        if table[5] != 0:
            raise ValueError("ChunkEvaluator: %d sample(s) were refused: a tag id outside [0, %d) or a predicted path shorter "
                             "than its sample's kept range" % (table[5], len(self.names)))
        return _scores_from_table(table, self.types, self.default.split("-")[-1], loss_sum / loss_n if loss_n > 0 else None)

    def reset(self) -> None:
        self._checks = {}
        if self._buf is not None:
            self._buf.zero_()
