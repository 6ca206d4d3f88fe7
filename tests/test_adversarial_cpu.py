"""CPU: the adversarial-training oracle (tests/adversarial_oracle.py), its bounds (tests/adversarial_check.py) and what of
icka_amd.adversarial needs no device.  The bounds accept an f32 emulation of icka_adv_ascend and reject five seeded faults; the
oracle has the properties the recipes rely on; the API refuses what it documents."""
import math

import numpy as np
import pytest
import torch

import adversarial_check as ac
import adversarial_oracle as ao
import test_dropout_hash_cpu as dh

F32 = torch.float32
EPS = float(np.float32(0.7))


def _case(B, S, H):
    return ac.ascend_inputs(B, S, H, zero_sample=1 if B >= 4 else None, inf_sample=3 if B >= 4 else None)


def _alphas(delta, grad, mask):
    """(alpha with the projection inactive for every sample, alpha with it active for every sample that steps)"""
    return float(np.float32(1e-3)), float(np.float32(5.0))


# ------------------------------------------------------------------------------------------------ oracle properties
@pytest.mark.parametrize("shape", ac.ASCEND_SHAPES)
def test_fgm_step_lands_on_the_sphere_and_pads_are_zero(shape):
    B, S, H = shape
    delta, grad, mask = _case(B, S, H)
    v = mask != 0
    zero = torch.where(v[:, :, None], torch.zeros_like(delta), delta)        # delta = 0 at the valid positions, junk elsewhere
    refs = ac.ascend_refs(zero, grad, mask, EPS, EPS)
    o = ao.ascend64(zero, grad, mask, EPS, EPS)
    n = torch.sqrt(ao.sumsq(o["delta"], v))
    st = o["stepped"]
    assert bool(st.any())
    bound = refs["norms"][1][:, 1]
    assert bool(((n[st] - EPS).abs() <= bound[st]).all()), (n, bound)
    assert not bool(o["delta"][~v].ne(0).any())
    assert bool((o["delta"][~st] == torch.where(v[:, :, None], zero, torch.zeros_like(zero)).double()[~st]).all())


@pytest.mark.parametrize("shape", ac.ASCEND_SHAPES)
def test_projection_never_leaves_the_ball_and_stayers_stay(shape):
    B, S, H = shape
    delta, grad, mask = _case(B, S, H)
    v = mask != 0
    for alpha, active in zip(_alphas(delta, grad, mask), (False, True)):
        o = ao.ascend64(delta, grad, mask, alpha, EPS)
        assert bool((o["shrunk"][o["stepped"]] == active).all()), "the two alphas cover the projection inactive and active"
        n = torch.sqrt(ao.sumsq(o["delta"], v))
        st = o["stepped"]
        assert bool((n[st] <= EPS * (1 + 1e-12)).all())
        assert bool((o["norms"][st, 1] <= EPS).all())
        assert not bool(o["delta"][~v].ne(0).any())
        for b in torch.nonzero(~st)[:, 0].tolist():
            assert torch.equal(o["delta"][b][v[b]], delta[b][v[b]].double())
    if B >= 4:
        o = ao.ascend64(delta, grad, mask, 1.0, EPS)
        assert not bool(o["stepped"][1]) and float(o["norms"][1, 0]) == 0.0            # g == 0
        assert not bool(o["stepped"][3]) and math.isinf(float(o["norms"][3, 0]))       # an inf in g
        assert not bool(o["stepped"][2])                                               # no valid position
        assert bool(o["stepped"][0])


def test_hash_restatement_equals_the_dropout_one_and_r_range():
    idx = np.concatenate([np.arange(1 << 16, dtype=np.uint32), np.array([2 ** 31, 2 ** 32 - 1], dtype=np.uint32)])
    for s0, s1 in ((0, 0), (0x9abc, 0x12345678), (0xffffffff, 0x80000001)):
        assert np.array_equal(ao.icka_hash(s0, s1, idx), dh.icka_hash(s0, s1, idx))
    r = ao.uniform_r(1 << 18, seed=(7 << 32) + 5, counter=3)
    assert r.min() >= -1.0 and r.max() < 1.0 and abs(r.mean()) < 0.01 and abs(r.std() - 1 / math.sqrt(3)) < 0.01
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r), "r is exact in f32"
    assert np.array_equal(ao.uniform_r(64, 10, 5), ao.uniform_r(64, 15, 0)), "the counter is added to the seed"
    assert not np.array_equal(ao.uniform_r(64, 10, 5), ao.uniform_r(64, 10, 6))


def test_uniform_start_norm_and_f32_form():
    B, S, H = 3, 5, 72
    _, _, mask = ac.ascend_inputs(B, S, H)
    d64 = ao.uniform_start64(mask, H, EPS, seed=11, counter=2)
    d32 = ao.uniform_start_f32(mask, H, EPS, seed=11, counter=2)
    v = mask != 0
    assert not bool(d32[~v].view(torch.int32).ne(0).any())
    assert bool(((d32.double() - d64).abs() <= 3 * 2.0 ** -24 * d64.abs()).all())       # sqrt, division, product
    n = torch.sqrt(ao.sumsq(d64, v))
    assert bool((n <= EPS).all()), "|r| < 1: the start lies inside the ball"
    assert bool((n[v.sum(1) >= 3] > 0.3 * EPS).all())


# ------------------------------------------------------------------------------------------------ bounds: emulation and faults
def _run(shape, alpha, fault=None, from_zero=False):
    B, S, H = shape
    delta, grad, mask = _case(B, S, H)
    if from_zero:
        delta = torch.where((mask != 0)[:, :, None], torch.zeros_like(delta), delta)
    refs = ac.ascend_refs(delta, grad, mask, alpha, EPS)
    out, norms = ac.emulate_ascend(delta, grad, mask, alpha, EPS, fault=fault)
    ac.compare_ascend(out, norms, delta, refs, "emulation %s %s" % (shape, fault))


@pytest.mark.parametrize("shape", ac.ASCEND_SHAPES)
def test_bounds_accept_the_f32_emulation(shape):
    for alpha in _alphas(None, None, None):
        _run(shape, alpha)
    _run(shape, EPS, from_zero=True)         # FGM: the projection decision is a coin toss, both outcomes are inside
    ac.report("adversarial_cpu %s" % (shape,))


@pytest.mark.parametrize("fault", ac.FAULTS)
def test_bounds_reject_the_seeded_faults(fault):
    shape = (4, 37, 520)
    alpha = float(np.float32(5.0)) if fault == "no_projection" else float(np.float32(1e-2))
    with pytest.raises(AssertionError):
        _run(shape, alpha, fault=fault)
    ac.kc._PENDING.clear()          # (the ratios of a run that is meant to fail are not a result)


def test_tree_depth_follows_the_header():
    assert ac.tree_depth(128, 768) == 2 * 2 * 8 + 6 + 2 + 0 + 6
    assert ac.tree_depth(1024, 2048) == 2 * 4 * 8 + 6 + 2 + 1 + 6
    assert ac.tree_depth(1, 8) == 16 + 14


# ------------------------------------------------------------------------------------------------ the API, without a device
def _tiny(n_emb=1):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import BertEmbeddings, BertModel
    cfg = BertConfig(64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, max_position_embeddings=16)
    m = BertModel(cfg)
    if n_emb == 2:
        m.more = BertEmbeddings(cfg)
    return m, cfg


def test_adversary_finds_its_embeddings_and_refuses_without_a_device():
    import icka_amd
    from icka_amd import adversarial
    from icka_amd.modeling import BertEmbeddings
    m, cfg = _tiny()
    adv = icka_amd.Adversary(m, epsilon=0.5)
    assert isinstance(adv.embeddings, BertEmbeddings) and adv.alpha == 0.5 and adv.steps == 1
    assert adv.delta is None and adv.grad is None and adv.norms is None
    fl = icka_amd.Adversary(m, epsilon=1.0, recipe="freelb", steps=3, alpha=0.3, init="uniform", seed=0)
    assert fl.steps == 3 and fl.alpha == 0.3
    two, _ = _tiny(2)
    with pytest.raises(ValueError, match="embeddings="):
        icka_amd.Adversary(two)
    assert icka_amd.Adversary(two, embeddings=two.more).embeddings is two.more
    with pytest.raises(ValueError, match="embeddings="):
        icka_amd.Adversary(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match="BertEmbeddings"):
        icka_amd.Adversary(m, embeddings=torch.nn.Linear(2, 2))
    for bad in (dict(recipe="pgd"), dict(init="normal"), dict(epsilon=0.0), dict(recipe="freelb", steps=0), dict(steps=2)):
        with pytest.raises(ValueError):
            icka_amd.Adversary(m, **bad)
    # the refusals
    ex, _ = _tiny()
    icka_amd.set_precision(ex, "fp32")
    with pytest.raises(NotImplementedError, match="fp32"):
        icka_amd.Adversary(ex)
    late, _ = _tiny()
    a2 = icka_amd.Adversary(late)
    icka_amd.set_precision(late, "fp32")
    with pytest.raises(NotImplementedError, match="fp32"):
        a2.clean().__enter__()
    assert late.embeddings._icka_adv is None and not adversarial.pass_open(late)
    pk, _ = _tiny()
    pk._icka_packed = object()                 # (what set_packed leaves on a model)
    with pytest.raises(NotImplementedError, match="packed"):
        icka_amd.Adversary(pk)
    odd, _ = _tiny()
    odd.embeddings.word_embeddings = torch.nn.Embedding(64, 36)
    with pytest.raises(NotImplementedError, match="hidden size"):
        icka_amd.Adversary(odd)

    class _Arena(object):
        reducer = object()
    dp, _ = _tiny()
    dp._icka_arena = _Arena()
    with pytest.raises(NotImplementedError, match="GradReducer"):
        icka_amd.Adversary(dp)
    # pass bookkeeping
    with adv.clean():
        assert m.embeddings._icka_adv is adv and adversarial.pass_open(m) and not adversarial.pass_open(two)
        with pytest.raises(RuntimeError, match="already open"):
            adv.perturbed().__enter__()
    assert m.embeddings._icka_adv is None and not adversarial.pass_open(m)
    with pytest.raises(TypeError):
        adv.ascend(torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        adv.ascend(torch.zeros(6, dtype=torch.int64))
