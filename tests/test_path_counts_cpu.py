"""CPU: the host oracle of icka_chunk_counts (tests/path_counts_oracle.py) against metrics.evaluate_lists and hand-made
samples, and the two plain-torch pieces of the minimum-risk recipe, metrics.f1_cost and icka_amd.minimum_risk."""
import math

import numpy as np
import pytest
import torch

import path_counts_oracle as PC
from icka_amd import metrics as M
from icka_amd.crf import minimum_risk


def test_oracle_sums_equal_evaluate_lists():
    rng = np.random.default_rng(4)
    for kind in ("random", "all_default", "entity_to_end", "skipped"):
        lens, rows, labels, mask = PC.random_case(5, 9, 3, rng, kind)
        got = PC.host_counts(lens, rows, labels, mask)
        assert int(got[..., 3].sum()) == 0
        offs = np.concatenate([[0], np.cumsum(lens)])
        for r in range(3):
            pred = [rows[r, offs[b]:offs[b] + lens[b]].tolist() + [0] * 9 for b in range(5)]
            pl, gl = M.filter_batch(pred, labels, mask, PC.LMAP)
            sc = M.evaluate_lists(pl, gl, PC.LMAP)
            assert got[r, :, :3].sum(0).tolist() == [sc.counts["correct_preds"], sc.counts["total_preds"], sc.counts["total_correct"]]


def test_oracle_on_hand_made_samples():
    # ids: 1 O, 4 B-PER, 5 I-PER, 8 B-LOC, 10 X
    labels = [[4, 5, 10, 1, 8], [1, 1, 1, 1, 1]]
    mask = [[1, 1, 1, 1, 1], [1, 1, 1, 0, 1]]
    lens = [5, 3]
    rows = [[4, 5, 7, 1, 8, 1, 1, 1],          # exact (the X position is dropped whatever is predicted there)
            [4, 1, 1, 1, 8, 4, 1, 1],          # PER cut short, LOC right; a false PER in sample 1
            [4, 5, 1, 1, -1, 1, 1, 1],         # -1 at a kept position: bad
            [4, 5, -1, 1, 8, 1, 1, 99]]        # -1 at a skipped position is not read; 99 at a kept position: bad
    got = PC.host_counts(lens, rows, labels, mask).tolist()
    assert got[0] == [[2, 2, 2, 0], [0, 0, 0, 0]]
    assert got[1] == [[1, 2, 2, 0], [0, 1, 0, 0]]
    assert got[2] == [[0, 0, 0, 1], [0, 0, 0, 0]]
    assert got[3] == [[2, 2, 2, 0], [0, 0, 0, 1]]
    assert PC.host_counts([4, 3], [r[1:] for r in rows[:1]], labels, mask).tolist()[0][0] == [0, 0, 0, 1]     # shorter than n0


def test_f1_cost():
    counts = torch.tensor([[[2, 2, 2, 0], [0, 0, 0, 0], [0, 0, 0, 1]],
                           [[1, 2, 2, 0], [0, 1, 0, 0], [3, 4, 5, 0]]], dtype=torch.int32)
    cost = M.f1_cost(counts)
    assert tuple(cost.shape) == (3, 2) and cost.dtype == torch.float32
    want = [[0.0, 0.5], [0.0, 1.0], [1.0, 1.0 - 6.0 / 9.0]]
    assert torch.allclose(cost, torch.tensor(want), atol=1e-7)
    with pytest.raises(ValueError):
        M.f1_cost(torch.zeros(2, 3))


def test_minimum_risk_value_and_gradient():
    inf = float("inf")
    logp = torch.tensor([[-1.0, -2.0, -inf], [-inf, -inf, -inf], [-0.5, -0.5, -3.0]], dtype=torch.float64, requires_grad=True)
    cost = torch.tensor([[0.0, 1.0, 5.0], [1.0, 1.0, 1.0], [0.2, 0.4, 1.0]], dtype=torch.float64)
    risk = minimum_risk(logp, cost, scale=2.0)
    q0 = math.exp(-2.0) / (math.exp(-2.0) + math.exp(-4.0))
    q2 = [math.exp(-1.0), math.exp(-1.0), math.exp(-6.0)]
    want = [1.0 - q0, 0.0, sum(q * c for q, c in zip(q2, [0.2, 0.4, 1.0])) / sum(q2)]
    assert torch.allclose(risk, torch.tensor(want, dtype=torch.float64), atol=1e-12)
    risk.sum().backward()
    g = logp.grad
    assert bool(torch.isfinite(g).all()) and float(g[1].abs().sum()) == 0 and float(g[0, 2]) == 0
    # d risk / d logp_r = scale q_r (cost_r - risk)
    assert abs(float(g[0, 0]) - 2.0 * q0 * (0.0 - want[0])) < 1e-12
    with pytest.raises(ValueError):
        minimum_risk(torch.zeros(2, 3), torch.zeros(2, 4))
