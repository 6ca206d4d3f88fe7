#!/usr/bin/env python3
"""Generate tests/golden/chunk_eval.npz by running the REFERENCE's own scorer (dev container only, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chunk_eval.py

``ner_evaluate.py`` (get_chunks :4-48, evaluate :64-110, evaluate_each_class :112-148) is imported from the reference tree and
fed what the dev loop of My_cross_attention.py:853-913 feeds it: seeded Twitter-shaped batches [32, 128] -- gold labels with
``X`` continuation pieces, ``[CLS]`` first and ``[SEP]`` last, ragged lengths, one sample whose output mask is not a prefix
mask; predictions = gold with 30 % of the ids redrawn over all 15 ids -- filtered by the rule of the loop at :882-903
(``filter_lists``).  ``evaluate`` writes ./test_results.txt into the working directory, so it runs in a temporary one.  Recorded
(int8 arrays unless said): the padded labels / predictions / masks, the filtered lists (flattened + lengths), evaluate's
(acc, f1, p, r) as float64 and the three counts, evaluate_each_class's (f1, p, r) for every type, and get_chunks of 64
sequences as (type index, start, end) rows.  Ends by asserting that the written file reproduces."""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (REF: where the reference tree lies)

OUT = os.path.join(HERE, "chunk_eval.npz")
LABEL_LIST = ["O", "B-MISC", "I-MISC", "B-PER", "I-PER", "B-ORG", "I-ORG", "B-LOC", "I-LOC", "X", "[CLS]", "[SEP]", "<s>", "</s>"]
NBATCH, B, S, L = 3, 32, 128, 15


def make_batches(rng):
    label_map = {i: label for i, label in enumerate(LABEL_LIST, 1)}
    label_map[0] = "PAD"
    rev = {v: k for k, v in label_map.items()}
    ents = ["MISC", "PER", "ORG", "LOC"]
    labels = np.zeros((NBATCH, B, S), dtype=np.int8)
    masks = np.zeros((NBATCH, B, S), dtype=np.int8)
    for n in range(NBATCH):
        for b in range(B):
            ln = int(rng.integers(3, S + 1))
            if b == 0:
                ln = S
            seq = [rev["[CLS]"]]
            while len(seq) < ln - 1:
                r = rng.random()
                if r < 0.55:
                    word = [rev["O"]]
                else:
                    e = ents[int(rng.integers(0, 4))]
                    first = "B-" if rng.random() < 0.85 else "I-"       # (an I- after O opens a chunk too)
                    word = [rev[first + e]] + [rev["I-" + e]] * int(rng.integers(0, 3))
                for w in word:
                    seq.append(w)
                    for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.3 else 0):
                        seq.append(rev["X"])
            seq = seq[:ln - 1] + [rev["[SEP]"]]
            labels[n, b, :ln] = seq
            masks[n, b, :ln] = 1
        masks[n, 5, 7] = 0                      # not a prefix mask: the loop breaks at the first zero
        masks[n, 6, :] = 0                      # nothing kept
    redraw = rng.random((NBATCH, B, S)) < 0.3
    preds = np.where(redraw, rng.integers(0, L, (NBATCH, B, S)), labels).astype(np.int8)
    return label_map, labels, preds, masks


SKIP = ("X", "</s>", "<s>", "[CLS]", "[SEP]")


def filter_lists(label_map, label_ids, pred_ids, output_mask):
    """What the dev loop hands to the scorer (My_cross_attention.py:882-903; that loop sits inside the script's main and cannot
    be imported, so its rule is applied here with numpy): per sample the positions before the first zero of the mask whose
    gold label is none of SKIP -> (gold names, predicted names, gold ids, predicted ids)."""
    out = ([], [], [], [])
    for g, p, m in zip(label_ids, pred_ids, output_mask):
        zeros = np.flatnonzero(m == 0)
        n0 = int(zeros[0]) if zeros.size else len(m)
        keep = [j for j in range(n0) if label_map[int(g[j])] not in SKIP]
        out[0].append([label_map[int(g[j])] for j in keep])
        out[1].append([label_map[int(p[j])] for j in keep])
        out[2].append([int(g[j]) for j in keep])
        out[3].append([int(p[j]) for j in keep])
    return out


def build():
    sys.path.insert(0, MG.REF)
    import ner_evaluate as NE
    rng = np.random.default_rng(20261016)
    label_map, labels, preds, masks = make_batches(rng)
    y_true, y_pred, y_true_idx, y_pred_idx = [], [], [], []
    for n in range(NBATCH):
        for acc_list, part in zip((y_true, y_pred, y_true_idx, y_pred_idx), filter_lists(label_map, labels[n], preds[n], masks[n])):
            acc_list += part
    reverse_label_map = {label: i for i, label in enumerate(LABEL_LIST, 1)}
    reverse_label_map["PAD"] = 0
    words = [list(range(len(r))) for r in y_true_idx]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                acc, f1, p, r = NE.evaluate(y_pred_idx, y_true_idx, y_pred, y_true, words, reverse_label_map)
        finally:
            os.chdir(cwd)
    correct = total_preds = total_correct = 0
    for lab, lab_pred in zip(y_true_idx, y_pred_idx):
        a, b = set(NE.get_chunks(lab, reverse_label_map)), set(NE.get_chunks(lab_pred, reverse_label_map))
        correct += len(a & b); total_preds += len(b); total_correct += len(a)
    types = []
    for i in range(L):
        t = label_map[i].split("-")[-1]
        if t not in types:
            types.append(t)
    each = np.array([NE.evaluate_each_class(y_pred_idx, y_true_idx, words, reverse_label_map, t) for t in types], dtype=np.float64)
    chunk_seqs = (y_true_idx[:32] + y_pred_idx[:32])
    rows, row_len = [], []
    for sq in chunk_seqs:
        cs = NE.get_chunks(sq, reverse_label_map)
        row_len.append(len(cs))
        rows += [(types.index(t), s, e) for t, s, e in cs]
    flat = lambda ll: np.array([v for r in ll for v in r], dtype=np.int8)  # noqa: E731
    return {
        "labels": labels, "preds": preds, "masks": masks,
        "gold_flat": flat(y_true_idx), "pred_flat": flat(y_pred_idx), "list_len": np.array([len(r) for r in y_true_idx], dtype=np.int16),
        "evaluate": np.array([acc, f1, p, r], dtype=np.float64),
        "counts": np.array([correct, total_preds, total_correct], dtype=np.int64),
        "each_class": each, "types": np.array(types), "label_list": np.array(LABEL_LIST),
        "chunk_seq_flat": flat(chunk_seqs), "chunk_seq_len": np.array([len(r) for r in chunk_seqs], dtype=np.int16),
        "chunk_rows": np.array(rows, dtype=np.int16).reshape(-1, 3), "chunk_row_len": np.array(row_len, dtype=np.int16),
    }


def main():
    fx = build()
    np.savez_compressed(OUT, **fx)
    again, disk = build(), np.load(OUT)
    for k, v in again.items():
        assert np.array_equal(disk[k], v) and disk[k].dtype == v.dtype, k
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
