"""CPU: the chunk scorer's Python restatement (icka_amd.metrics.chunks / evaluate_lists / filter_batch) and a numpy
restatement of the kernel's label_table + flag formulation against tests/golden/chunk_eval.npz, recorded from the reference's
own ner_evaluate.py (tests/golden/make_golden_chunk_eval.py): counts equal, floats bitwise."""
import os

import numpy as np
import pytest

from icka_amd import metrics as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    f = np.load(os.path.join(HERE, "golden", "chunk_eval.npz"))
    d = {k: f[k] for k in f.files}
    d["label_map"] = M.label_list_map([str(s) for s in d["label_list"]])
    d["type_names"] = [str(s) for s in d["types"]]
    return d


def _split(flat, lens):
    out, o = [], 0
    for n in lens:
        out.append([int(v) for v in flat[o:o + int(n)]])
        o += int(n)
    assert o == len(flat)
    return out


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.int64)[0]


def test_for_label_list_is_the_reference_map(fx):
    ev = M.ChunkEvaluator.for_label_list(M.REFERENCE_LABEL_LIST)
    assert [str(s) for s in fx["label_list"]] == list(M.REFERENCE_LABEL_LIST)
    assert ev.id_to_label == {0: "PAD", **{i: n for i, n in enumerate(M.REFERENCE_LABEL_LIST, 1)}}
    assert ev.types == fx["type_names"] and len(ev.types) == 11
    words = ev.table_words
    assert words[1] & M.LT_DEFAULT and not any(w & M.LT_DEFAULT for i, w in enumerate(words) if i != 1)
    assert [i for i, w in enumerate(words) if w & M.LT_BEGIN] == [2, 4, 6, 8]
    assert [i for i, w in enumerate(words) if w & M.LT_SKIP] == [10, 11, 12, 13, 14]
    assert [w >> M.LT_TYPE_SHIFT for w in words] == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10]


def test_constructor_refusals():
    with pytest.raises(ValueError):
        M.ChunkEvaluator({0: "PAD", 1: "B-PER"})                         # no default tag
    with pytest.raises(ValueError):
        M.ChunkEvaluator(["O"] + ["B-T%d" % (i % 3) for i in range(64)])  # 65 ids
    with pytest.raises(ValueError):
        M.ChunkEvaluator(["O"] + ["B-T%d" % i for i in range(32)])        # 33 types
    with pytest.raises(ValueError):
        M.ChunkEvaluator({0: "O", 2: "B-PER"})                            # a hole in the ids
    M.ChunkEvaluator(["O"] + ["B-T%d" % i for i in range(31)])            # 32 types, 32 ids: fine
    M.ChunkEvaluator(["O"] + ["B-T%d" % (i % 31) for i in range(63)])     # 64 ids: fine


def test_chunks_equal_the_recorded_chunks(fx):
    seqs = _split(fx["chunk_seq_flat"], fx["chunk_seq_len"])
    assert len(seqs) == 64
    rows = fx["chunk_rows"].tolist()
    o = 0
    for seq, n in zip(seqs, fx["chunk_row_len"]):
        want = [(fx["type_names"][t], s, e) for t, s, e in rows[o:o + int(n)]]
        o += int(n)
        assert M.chunks(seq, fx["label_map"]) == want
    assert o == len(rows)


def test_filter_batch_equals_the_recorded_lists(fx):
    gold, pred = _split(fx["gold_flat"], fx["list_len"]), _split(fx["pred_flat"], fx["list_len"])
    pl, gl = [], []
    for n in range(fx["labels"].shape[0]):
        p, g = M.filter_batch(fx["preds"][n].tolist(), fx["labels"][n], fx["masks"][n], fx["label_map"])
        pl += p
        gl += g
    assert gl == gold and pl == pred


def _check_scores(sc, fx):
    assert [sc.counts["correct_preds"], sc.counts["total_preds"], sc.counts["total_correct"]] == fx["counts"].tolist()
    assert sc.counts["kept_tokens"] == int(fx["list_len"].sum())
    for got, want in zip(tuple(sc), fx["evaluate"]):
        assert _bits(got) == _bits(want), (got, want)
    assert sorted(sc.per_class) == sorted(t for t in fx["type_names"] if t != "O")
    for i, t in enumerate(fx["type_names"]):
        if t == "O":
            assert fx["each_class"][i].tolist() == [0.0, 0.0, 0.0]
            continue
        for got, want in zip(sc.per_class[t], fx["each_class"][i]):
            assert _bits(got) == _bits(want), (t, got, want)


def test_evaluate_lists_equals_the_reference(fx):
    gold, pred = _split(fx["gold_flat"], fx["list_len"]), _split(fx["pred_flat"], fx["list_len"])
    sc = M.evaluate_lists(pred, gold, fx["label_map"])
    _check_scores(sc, fx)
    assert sum(sc.per_class_counts[t][0] for t in sc.per_class) == sc.counts["correct_preds"]


def flag_counts(pred, labels, mask, words, ntypes):
    """The kernel's formulation in numpy: label_table words, compaction, start / term flags, first term of either side."""
    table = np.zeros(M.HEAD + 3 * ntypes, dtype=np.int64)
    W = np.asarray(words, dtype=np.int64)
    for p, g, m in zip(np.asarray(pred), np.asarray(labels), np.asarray(mask)):
        z = np.flatnonzero(m == 0)
        n0 = int(z[0]) if z.size else len(m)
        g, p = g[:n0].astype(np.int64), p[:n0].astype(np.int64)
        keep = (W[g] & M.LT_SKIP) == 0
        g, p = g[keep], p[keep]
        n = len(g)
        table[0] += n
        table[1] += int((g == p).sum())
        if n == 0:
            continue
        flags = []
        for w in (W[g], W[p]):
            o = (w & M.LT_DEFAULT) != 0
            t = w >> M.LT_TYPE_SHIFT
            prev_o = np.concatenate([[True], o[:-1]])
            prev_t = np.concatenate([[-1], t[:-1]])
            start = ~o & (prev_o | (t != prev_t) | ((w & M.LT_BEGIN) != 0))
            flags.append((start, o | start, t))
        (sg, tg, ty_g), (sp, tp, ty_p) = flags
        np.add.at(table, M.HEAD + 3 * ty_g[sg] + 2, 1)
        np.add.at(table, M.HEAD + 3 * ty_p[sp] + 1, 1)
        table[3] += int(sp.sum())
        table[4] += int(sg.sum())
        either, both = tg | tp, tg & tp
        for i in np.flatnonzero(sg & sp & (ty_g == ty_p)):
            nxt = np.flatnonzero(either[i + 1:])
            if nxt.size == 0 or both[i + 1 + nxt[0]]:
                table[2] += 1
                table[M.HEAD + 3 * ty_g[i]] += 1
    return table


def test_flag_formulation_equals_the_reference(fx):
    words, types = M.label_table(fx["label_map"])
    table = sum(flag_counts(fx["preds"][n], fx["labels"][n], fx["masks"][n], words, len(types))
                for n in range(fx["labels"].shape[0]))
    sc = M._scores_from_table(table.tolist(), types, "O")
    _check_scores(sc, fx)
    gold, pred = _split(fx["gold_flat"], fx["list_len"]), _split(fx["pred_flat"], fx["list_len"])
    ref = M.evaluate_lists(pred, gold, fx["label_map"])
    assert sc.counts == ref.counts and sc.per_class_counts == ref.per_class_counts


def test_no_kept_token_gives_nan_accuracy(fx):
    sc = M.evaluate_lists([[]], [[]], fx["label_map"])
    assert np.isnan(sc.acc) and (sc.f1, sc.p, sc.r) == (0, 0, 0) and sc.mean_loss is None
