"""GPU: icka_chunk_counts / ChunkEvaluator.path_counts against the host oracle of tests/path_counts_oracle.py per (row,
sample), as exact integers; for every row the column sums against what icka_chunk_eval adds for that row; guard bands."""
import numpy as np
import pytest
import torch

import kernel_check as kc
import path_counts_oracle as PC
from icka_amd import crf as crf_mod
from icka_amd import kernels as K
from icka_amd import metrics as M

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _i64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).cuda()


def _run(ev, lens, rows, labels, mask):
    """icka_chunk_counts into a guarded buffer -> int64 array [R, B, 4]; also asserts the column sums against icka_chunk_eval
    on (lens, row r) for every r."""
    R, B = len(rows), len(lens)
    ev._ensure()
    lens_t = torch.tensor(list(lens), dtype=I32).cuda()
    rows_t = torch.as_tensor(np.asarray(rows), dtype=I32).cuda()
    counts, chk = kc.guarded(R * B, 4, I32)
    K.chunk_counts(lens_t, rows_t, _i64(labels), _i64(mask), ev._table, counts.view(R, B, 4), len(ev.types))
    torch.cuda.synchronize()
    chk()
    got = counts.view(R, B, 4).cpu().numpy().astype(np.int64)
    for r in range(R):
        ev.reset()
        ev.update(crf_mod.DeviceTags(lens_t, rows_t[r].contiguous()), _i64(labels), _i64(mask))
        c = ev.counters.tolist()
        assert got[r].sum(0).tolist() == [c[2], c[3], c[4], c[5]], (r, got[r].sum(0), c[:6])
    return got


@pytest.mark.parametrize("kind", ["random", "all_default", "entity_to_end", "skipped"])
@pytest.mark.parametrize("B,S,R", [(1, 1, 1), (5, 1, 8), (1, 9, 8), (5, 70, 1), (5, 130, 8)])
def test_counts_equal_the_host_scorer(kind, B, S, R):
    rng = np.random.default_rng(B * 1000 + S * 10 + R)
    lens, rows, labels, mask = PC.random_case(B, S, R, rng, kind)
    got = _run(M.ChunkEvaluator(PC.LMAP), lens, rows, labels, mask)
    want = PC.host_counts(lens, rows, labels, mask)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    if kind != "random" or S == 1:
        return
    assert int(want[..., 3].sum()) == 0 and (S < 9 or int(want[..., 0].sum()) > 0)


def test_bad_samples_get_one_bad_and_nothing_else():
    rng = np.random.default_rng(7)
    B, S, R = 5, 40, 8
    lens, rows, labels, mask = PC.random_case(B, S, R, rng)
    mask[:] = 1
    labels[:, 10] = 1                                      # a kept position in every sample
    lens = [S, S - 1, S, S, S]                             # sample 1: a path shorter than n0
    rows[:] = -7
    for r in range(R):
        pred = np.where(rng.random((B, S)) < 0.3, rng.integers(0, PC.L, (B, S)), labels)
        flat = np.concatenate([pred[b, :lens[b]] for b in range(B)])
        rows[r, :len(flat)] = flat
    offs = np.concatenate([[0], np.cumsum(lens)])
    rows[2, offs[3] + 10] = PC.L                           # ids outside [0, L) at a kept position
    rows[3, offs[4] + 10] = -1
    rows[5, offs[0] + 10] = 1 << 20
    labels[2, S - 1] = 99                                  # a gold id outside [0, L): every row of sample 2
    got = _run(M.ChunkEvaluator(PC.LMAP), lens, rows, labels, mask)
    want = PC.host_counts(lens, rows, labels, mask)
    assert np.array_equal(got, want)
    bad = got[..., 3]
    assert bad[:, 1].tolist() == [1] * R and bad[:, 2].tolist() == [1] * R
    assert bad[2, 3] == 1 and bad[3, 4] == 1 and bad[5, 0] == 1 and int(bad.sum()) == 2 * R + 3
    assert not got[bad == 1][:, :3].any()


def test_missing_nbest_ranks_are_bad_and_the_rest_scores():
    """3 tags: a sample of one position has 3 paths for 8 ranks; its other ranks hold -1"""
    names = ["O", "B-PER", "I-PER"]
    B, S, C, R = 5, 6, 3, 8
    g = torch.Generator().manual_seed(3)
    e = torch.randn(B, S, C, generator=g) * 2.0
    mask = (torch.arange(S)[None, :] < torch.tensor([6, 1, 3, 5, 2])[:, None]).long()
    labels = torch.randint(0, C, (B, S), generator=g)
    torch.manual_seed(1)
    crf = crf_mod.CRF(C, batch_first=True).cuda()
    nb = crf.decode_nbest(e.cuda(), mask.cuda(), nbest=R)
    h = nb.host()
    assert h["n_paths"][1] == 3 and all(n == R for b, n in enumerate(h["n_paths"]) if b != 1)
    ev = M.ChunkEvaluator(names)
    got = ev.path_counts(nb, labels.cuda(), mask.cuda())
    assert got.dtype == I32 and tuple(got.shape) == (R, B, 4)
    want = PC.host_counts(h["lens"], h["tags"], labels, mask, names)
    assert np.array_equal(got.cpu().numpy(), want)
    assert got[:, 1, 3].tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and int(got[..., 3].sum()) == 5
    cost = M.f1_cost(got)
    assert tuple(cost.shape) == (B, R) and cost[1, 3:].tolist() == [1.0] * 5
    # one DeviceTags row, and the draws of the sampler, go through the same entry
    one = ev.path_counts(nb.rank(0), labels.cuda(), mask.cuda())
    assert torch.equal(one[0], got[0])
    sp = crf.sample(e.cuda(), mask.cuda(), num_samples=4, seed=5)
    hs = sp.host()
    assert np.array_equal(ev.path_counts(sp, labels.cuda(), mask.cuda()).cpu().numpy(),
                          PC.host_counts(hs["lens"], hs["tags"], labels, mask, names))


def test_refusals():
    ev = M.ChunkEvaluator(PC.LMAP)
    ev._ensure()
    lab = torch.ones(2, 4, dtype=torch.int64, device="cuda")
    lens = torch.full((2,), 4, dtype=I32, device="cuda")
    ok = torch.zeros(3, 8, dtype=I32, device="cuda")
    with pytest.raises(ValueError, match="tags"):
        K.chunk_counts(lens, torch.zeros(65, 8, dtype=I32, device="cuda"), lab, lab, ev._table,
                       torch.zeros(65, 2, 4, dtype=I32, device="cuda"), len(ev.types))
    with pytest.raises(ValueError, match="counts"):
        K.chunk_counts(lens, ok, lab, lab, ev._table, torch.zeros(3, 2, 3, dtype=I32, device="cuda"), len(ev.types))
    with pytest.raises(ValueError, match="512"):
        big = torch.ones(2, 513, dtype=torch.int64, device="cuda")
        K.chunk_counts(lens, ok, big, big, ev._table, torch.zeros(3, 2, 4, dtype=I32, device="cuda"), len(ev.types))
    with pytest.raises(ValueError, match="paths"):
        ev.path_counts([[1, 1, 1, 1]] * 2, lab, lab)
