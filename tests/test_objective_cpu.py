"""CPU: the objective oracle (tests/objective_oracle.py) against the reference's own losses stored in tests/golden/objective_*.npz
(made by tests/golden/make_golden_objective.py), and the closed-form contrastive gradient of csrc/objective.hip against float64
autograd of the oracle."""
import glob
import os

import numpy as np
import pytest
import torch

import objective_oracle as OO
from golden_util import GOLDEN_DIR

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "objective_*.npz")))


def test_fixture_set_is_complete():
    assert len(CASES) == 8, CASES


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_fixture(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    temp, temp_lamb, lamb, nr, n = z["meta_objective"]
    variant = str(z["meta_variant"])
    B = z["input_ids"].shape[0]
    if variant == "gate_cl":
        assert OO.negatives(B, None if nr < 0 else int(nr)) == int(n)
    t, v = torch.from_numpy(z["t"]).double(), torch.from_numpy(z["v"]).double()
    main, cl, crs = z["parts"]
    assert abs(OO.cl_loss(t, v, temp, temp_lamb).item() - cl) <= 1e-6
    if variant == "gate_cl":
        assert abs(OO.crs_loss(torch.from_numpy(z["crs"]).double(), int(n)).item() - crs) <= 1e-6
        total = lamb * main + (1 - lamb) * (crs + cl)
    else:
        total = 0.88 * main + 0.12 * cl
    assert abs(total - z["loss"][0]) <= 1e-6 * max(1.0, abs(total))


@pytest.mark.parametrize("B,n", [(8, 0), (8, 1), (8, 3), (8, 4), (8, 8), (5, 4), (1, 1)])
def test_swap_matches_the_reference_loop(B, n):
    x = torch.arange(B * 6, dtype=torch.float64).view(B, 2, 3)
    ref = x.clone()
    neg = ref[B - n:]
    front, after = neg[:n // 2], neg[n // 2:]
    for i in range(front.shape[0]):              # gate_cl_modeling.py:1349-1353
        tmp = front[i].clone()
        front[i] = after[i].clone()
        after[i] = tmp.clone()
    assert torch.equal(OO.swap(x, n), ref)
    assert torch.equal(OO.swap(OO.swap(x, n), n), x)      # its own inverse


def test_negatives_rule():
    assert OO.negatives(8, None) == 0 and OO.negatives(8, 8) == 0 and OO.negatives(8, 16) == 0
    assert OO.negatives(8, 0) == 0 and OO.negatives(8, 3) == 3 and OO.negatives(32, 16) == 16
    assert OO.crs_labels(6, 2).tolist() == [1, 1, 1, 1, 0, 0]


@pytest.mark.parametrize("B,D", [(1, 8), (2, 16), (7, 64), (32, 96)])
@pytest.mark.parametrize("temp,temp_lamb", [(0.05, 0.7), (0.179, 0.0), (1.0, 1.0), (0.179, 0.7)])
def test_closed_form_gradient_matches_autograd(B, D, temp, temp_lamb):
    g = torch.Generator().manual_seed(B * 1000 + D)
    t = torch.randn(B, D, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(B, D, generator=g, dtype=torch.float64, requires_grad=True)
    OO.cl_loss(t, v, temp, temp_lamb).backward()
    dt, dv = OO.cl_grad(t.detach(), v.detach(), temp, temp_lamb)
    assert torch.allclose(dt, t.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(dv, v.grad, rtol=1e-10, atol=1e-12)
    if B == 1:
        assert OO.cl_loss(t, v, temp, temp_lamb).item() == 0.0
