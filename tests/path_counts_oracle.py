"""Host oracle of icka_chunk_counts (no test functions): per (path row, sample) the counts (correct_preds, total_preds,
total_correct, bad) from the host scorer of icka_amd/metrics.py (``chunks``), by the rules written out for icka_chunk_eval in
include/icka_hip.h, and the case builder the CPU and GPU tests share."""
import numpy as np

from icka_amd import metrics as M

LMAP = M.label_list_map(M.REFERENCE_LABEL_LIST)         # 0 PAD, 1 O, 2 B-MISC .. 9 I-LOC, 10 X, 11 [CLS], 12 [SEP], 13 <s>, 14 </s>
L = len(LMAP)


def n0_of(mask_row):
    z = np.flatnonzero(np.asarray(mask_row) == 0)
    return int(z[0]) if z.size else len(mask_row)


def host_counts(lens, rows, labels, mask, id_to_label=LMAP, skip=M.DEFAULT_SKIP):
    """lens [B], rows [R][capacity] (paths back to back), labels / mask [B][S] -> int array [R, B, 4]"""
    names = M.label_names(id_to_label)
    nl = len(names)
    labels, mask = np.asarray(labels), np.asarray(mask)
    B = len(lens)
    out = np.zeros((len(rows), B, 4), dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    for r, row in enumerate(rows):
        for b in range(B):
            path = list(row[offs[b]:offs[b] + lens[b]])
            n0 = n0_of(mask[b])
            gold = [int(v) for v in labels[b, :n0]]
            bad = len(path) < n0 or offs[b] + n0 > len(row) or any(not 0 <= v < nl for v in gold)
            g, p = [], []
            if not bad:
                for j in range(n0):
                    if names[gold[j]] in skip:
                        continue
                    if not 0 <= path[j] < nl:
                        bad = True
                        break
                    g.append(gold[j])
                    p.append(int(path[j]))
            if bad:
                out[r, b] = (0, 0, 0, 1)
                continue
            gc, pc = set(M.chunks(g, id_to_label)), set(M.chunks(p, id_to_label))
            out[r, b] = (len(gc & pc), len(pc), len(gc), 0)
    return out


def random_case(B, S, R, rng, kind="random"):
    """-> (lens [B], rows [R, B*S + 3] int64 with -7 past the paths, labels, mask): gold with entity runs, every row the gold
    with 30 % redrawn, ragged prefix masks with one non-prefix row; path b has n0_b <= lens[b] <= S tags."""
    ids = np.arange(L)
    labels = rng.choice(ids, size=(B, S), p=np.array([1, 8, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1]) / 40.0)
    mask = (np.arange(S)[None, :] < rng.integers(0, S + 1, (B, 1))).astype(np.int64)
    mask[0] = 1
    if B > 2 and S > 2:
        mask[2, S // 2] = 0
    if kind == "all_default":
        labels[:] = 1
    elif kind == "entity_to_end" and S >= 3:
        labels[:, -3:] = [4, 5, 5]                     # B-PER I-PER I-PER up to the last kept token of the full rows
    elif kind == "skipped":
        labels[:, ::2] = rng.choice([10, 11, 12], size=labels[:, ::2].shape)      # X, [CLS], [SEP]
    lens = [max(1, int(rng.integers(n0_of(mask[b]), S + 1))) for b in range(B)]
    rows = np.full((R, B * S + 3), -7, dtype=np.int64)
    for r in range(R):
        pred = np.where(rng.random((B, S)) < 0.3, rng.integers(0, L, (B, S)), labels)
        flat = np.concatenate([pred[b, :lens[b]] for b in range(B)])
        rows[r, :len(flat)] = flat
    return lens, rows, labels, mask
