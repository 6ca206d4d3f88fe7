"""CPU: the checker of tests/crf_sample_check.py against the f32 emulation of icka_crf_sample's normative algorithm -- the
emulation passes on every case of the GPU list with at most 5 % borderline steps, every planted fault is rejected, and the
uniforms give the enumerated path frequencies."""
import itertools
import math

import numpy as np
import pytest
import torch

import crf_check as CC
import crf_sample_check as SC


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_emulation_passes_the_checker_within_the_borderline_cap(case):
    inp = SC.make_case(case)
    K = case[4]
    share = SC.check(inp, SC.emulate(inp, K, SC.SEED), K, SC.SEED, verbose=case[0])
    assert share <= SC.CAP, share


def test_centred_bounds_stay_below_the_uncentred_ones():
    """re-centring only removes the u |alpha| terms of crf_check.log_errors: on a chain whose scores grow the log Z bound of the
    centred recursion is smaller, and on a chain of one position (nothing to re-centre but alpha_0) it is at most 2 u |alpha_0|
    larger"""
    inp = SC.make_case(SC.CASES[8])
    c = SC.chain(inp, 0)
    assert SC.alpha_errors(c)[2] < CC.log_errors(c)[2]
    one = SC.chain(SC.make_case(SC.CASES[1]), 0)
    assert SC.alpha_errors(one)[2] <= CC.log_errors(one)[2] + 2 * SC.U_ACC * float(one.alpha.abs().max())


def test_another_seed_and_a_device_seed_pass_too():
    case = SC.CASES[2]
    inp, K = SC.make_case(case), case[4]
    a = SC.emulate(inp, K, SC.SEED)
    for seed, dev in ((SC.SEED + 1, (0, 0)), (SC.SEED, (7, 0)), (0, (3, 0x8000_0001))):
        o = SC.emulate(inp, K, seed, dev)
        assert o["tags"] != a["tags"]
        assert SC.check(inp, o, K, seed, dev) <= SC.CAP
        with pytest.raises(AssertionError):
            SC.check(inp, o, K, SC.SEED)                     # and not under the first seed


FAULT_CASE = ("faults", 4, 9, 5, 8, "holes", 2.0, 0)


@pytest.mark.parametrize("fault", [f for f in SC.FAULTS if f != "greater_equal"])
def test_planted_faults_are_rejected(fault):
    inp, K = SC.make_case(FAULT_CASE), FAULT_CASE[4]
    assert SC.check(inp, SC.emulate(inp, K, SC.SEED), K, SC.SEED) <= SC.CAP
    with pytest.raises(AssertionError):
        SC.check(inp, SC.emulate(inp, K, SC.SEED, fault=fault), K, SC.SEED)


def test_greater_equal_draws_a_zero_weight_tag_and_is_rejected():
    """tag 0 cannot end a path (end[0] = -1e4) and the uniform of the first step drawn is exactly 0: `>=` takes tag 0"""
    B, S, C, K = 1, 3, 4, 1
    g = torch.Generator().manual_seed(5)
    inp = {"e": torch.randn(B, S, C, generator=g), "mask": None, "start": torch.zeros(C), "end": torch.zeros(C),
           "trans": torch.randn(C, C, generator=g) * 0.5}
    inp["end"][0] = -1e4
    seed = SC.seed_with_zero_uniform(S - 1)                  # b = 0, k = 0, position S - 1
    assert SC.uniforms(seed, (0, 0), 0, K, 0, S, [S - 1])[0] == 0.0
    good = SC.emulate(inp, K, seed)
    assert good["tags"][0][S - 1] != 0 and SC.check(inp, good, K, seed) <= 1.0
    bad = SC.emulate(inp, K, seed, fault="greater_equal")
    assert bad["tags"][0][S - 1] == 0
    with pytest.raises(AssertionError, match="exactly 0"):
        SC.check(inp, bad, K, seed)


def test_empirical_path_frequencies():
    """2 tags, 3 positions, 64 draws of 32 identical samples: each of the 8 paths within 5 standard deviations of its
    enumerated probability (a check of the uniforms, not of the kernel)"""
    B, S, C, K = 32, 3, 2, 64
    g = torch.Generator().manual_seed(11)
    e1 = torch.randn(1, S, C, generator=g)
    inp = {"e": e1.expand(B, S, C).contiguous(), "mask": None, "start": torch.randn(C, generator=g) * 0.5,
           "end": torch.randn(C, generator=g) * 0.5, "trans": torch.randn(C, C, generator=g) * 0.7}
    out = SC.emulate(inp, K, SC.SEED)
    assert SC.check(inp, out, K, SC.SEED) <= SC.CAP
    c = SC.chain(inp, 0)
    count = {}
    for row in SC.split_rows(out["lens"], out["tags"]):
        for y in row:
            count[tuple(y)] = count.get(tuple(y), 0) + 1
    n = B * K
    for y in itertools.product(range(C), repeat=S):
        p = math.exp(sum(CC.path_terms(list(y), c.x, c.start, c.end, c.T)) - float(c.log_z))
        assert abs(count.get(y, 0) - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (y, count.get(y, 0), n * p)
