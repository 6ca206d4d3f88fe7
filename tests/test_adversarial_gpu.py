"""GPU: icka_amd.Adversary on the tiny tagger of tests/test_train_step_gpu.py (eval mode: dropout off).

  * Table-shift identity, the end-to-end oracle that needs no CPU model: for a batch whose ids are all distinct and non-zero, a
    perturbed forward with a fixed delta IS the plain forward of a copy whose word table holds fl(word[id_t] + delta_t) -- loss
    bitwise, ``adv.grad[b, t]`` the copy's word-gradient row id_t, every other gradient the copy's.  The gradient tolerance is
    what two plain backward runs of the copy differ by, measured here (bitwise if they agree bitwise).
  * The recipes against the same passes run by hand with the building blocks.
  * FGM inside TrainStep / GraphedStep against the same recipe launched eagerly (bars of tests/test_train_step_gpu.py).
  * GraphedModule, the refusals, and a model without an adversary."""
import copy

import numpy as np
import pytest
import torch

import icka_amd
import adversarial_check as ac
from test_train_step_gpu import NAMES, OPT_STEPS, _assert_close, _batches, _model, _optimizer

pytestmark = pytest.mark.gpu

EPS = 0.5
MASK = NAMES.index("input_mask")


def _distinct_batch():
    """the first synthetic batch with its ids replaced by 128 distinct non-zero ids (4 x 32 <= vocab - 1 = 511)"""
    b = list(_batches(1)[0])
    g = torch.Generator().manual_seed(5)
    b[0] = (torch.randperm(511, generator=g)[:128] + 1).reshape(4, 32).cuda()
    return tuple(b)


def _loss_of(model, b):
    return model(*b[:-1], labels=b[-1])


def _grads(model):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _plain(model, b):
    model.zero_grad()
    loss = _loss_of(model, b)
    loss.backward()
    return loss.detach().clone(), _grads(model)


def _noise(model, b):
    """per parameter: max |difference| of two plain backward runs of the same model on the same batch"""
    _, g1 = _plain(model, b)
    loss, g2 = _plain(model, b)
    return loss, g2, {n: float((g1[n] - g2[n]).abs().max()) for n in g1}


def _close(got, want, tol, what):
    for n in want:
        d = float((got[n] - want[n]).abs().max())
        assert d <= tol[n], "%s: %s differs by %.3e, two plain runs differ by %.3e" % (what, n, d, tol[n])


WORD = "bert.embeddings.word_embeddings.weight"


# ------------------------------------------------------------------------------------------------ table-shift identity
@pytest.mark.parametrize("precision", ["bf16", "mixed16"])
def test_table_shift_identity(precision):
    base = _model(precision)
    b = _distinct_batch()
    ids, mask = b[0], b[MASK]
    model, shifted = copy.deepcopy(base), copy.deepcopy(base)
    adv = icka_amd.Adversary(model, epsilon=EPS)
    adv.reset(mask)
    delta = torch.randn(4, 32, 128, generator=torch.Generator().manual_seed(9)).cuda() * 0.05
    adv.delta.copy_(delta)
    model.zero_grad()
    with adv.perturbed():
        loss = _loss_of(model, b)
        loss.backward()
    got = _grads(model)
    with torch.no_grad():
        W = shifted.bert.embeddings.word_embeddings.weight
        W[ids.reshape(-1)] = W[ids.reshape(-1)] + delta.reshape(-1, 128)          # one f32 add per element, as the kernel's
    want_loss, want, tol = _noise(shifted, b)
    assert torch.equal(loss.detach(), want_loss), (float(loss.detach()), float(want_loss))
    rows = want[WORD][ids.reshape(-1)]
    d = float((adv.grad.reshape(-1, 128) - rows).abs().max())
    assert d <= tol[WORD], "adv.grad against the shifted copy's word-gradient rows: %.3e (two plain runs: %.3e)" % (d, tol[WORD])
    assert float(rows.abs().max()) > 0
    _close(got, want, tol, "perturbed pass against the shifted copy")
    print("\n[table shift %s] loss %.6f bitwise; largest two-run difference %.3e" % (precision, float(loss.detach()), max(tol.values())))


# ------------------------------------------------------------------------------------------------ recipes
def test_fgm_is_the_clean_plus_the_adversarial_pass():
    base = _model("bf16")
    b = _distinct_batch()
    mask = b[MASK]
    model, hand = copy.deepcopy(base), copy.deepcopy(base)
    _, _, noise = _noise(copy.deepcopy(base), b)
    adv = icka_amd.Adversary(model, epsilon=EPS, recipe="fgm")
    model.zero_grad()
    loss = adv.run(lambda: _loss_of(model, b), input_mask=mask)
    total = _grads(model)
    # by hand
    a2 = icka_amd.Adversary(hand, epsilon=EPS)
    hand.zero_grad()
    with a2.clean():
        l2 = _loss_of(hand, b)
        l2.backward()
    g_clean = _grads(hand)
    g_rows = a2.grad.detach().clone()
    hand.zero_grad()
    a2.reset(mask)
    a2.ascend(mask, alpha=EPS)
    with a2.perturbed():
        _loss_of(hand, b).backward()
    g_adv = _grads(hand)
    assert torch.equal(loss.detach(), l2.detach()), "run returns the clean loss"
    if not any(noise.values()):        # (two runs of a pass agree bitwise: so do the two ascents)
        assert torch.equal(adv.delta, a2.delta)
    for n in total:
        want = g_clean[n] + g_adv[n]
        # one f32 rounding of the sum either way, plus what two runs of one pass differ by (twice: two passes)
        tol = 2.0 ** -22 * (g_clean[n].abs() + g_adv[n].abs()) + 2 * noise[n] + 1e-30
        assert bool(((total[n] - want).abs() <= tol).all()), n
    assert float((g_adv[WORD] - g_clean[WORD]).abs().max()) > 0, "the adversarial pass is another pass"
    # ||delta_b|| = epsilon for every non-empty sample, inside the oracle's bound for the recorded clean gradient
    refs = ac.ascend_refs(torch.zeros(4, 32, 128), g_rows.cpu(), mask.cpu(), float(np.float32(EPS)), float(np.float32(EPS)))
    n = a2.norms.cpu().double()
    st = refs["stepped"]
    assert bool(st.all()), "every sample of the batch has valid positions and a gradient"
    assert bool(((n[:, 1] - EPS).abs() <= refs["norms"][1][:, 1]).all()), n
    v = (mask != 0).cpu()
    dn = torch.sqrt((torch.where(v[:, :, None], a2.delta.cpu().double(), torch.zeros(1, dtype=torch.float64)) ** 2).sum((1, 2)))
    # the float64 norm of the stored delta: the kernel's n_g and its projection factor are each off by at most
    # adversarial_check.r_norm(32, 128) = 2e-6 relative, the products by 2^-23 each: 1e-5 holds all of them
    assert 4 * ac.r_norm(32, 128) < 1e-5
    assert bool(((dn - EPS).abs() <= 1e-5 * EPS).all()), dn
    assert not bool(a2.delta.cpu()[~v].ne(0).any())


def test_freelb_of_one_step_from_zero_is_a_plain_step():
    base = _model("bf16")
    b = _distinct_batch()
    model, plain = copy.deepcopy(base), copy.deepcopy(base)
    want_loss, want, tol = _noise(plain, b)
    adv = icka_amd.Adversary(model, epsilon=EPS, recipe="freelb", steps=1, init="zero")
    model.zero_grad()
    loss = adv.run(lambda: _loss_of(model, b), input_mask=b[MASK])
    assert torch.equal(loss, want_loss)
    _close(_grads(model), want, tol, "FreeLB(steps=1, init=zero) against a plain step")


# ------------------------------------------------------------------------------------------------ capture
def _step_fn(model, adv, k):
    def step_fn(ids, seg, mask, added, vmean, vatt, labels):
        return adv.run(lambda: model(ids, seg, mask, added, vmean, vatt, labels=labels) / k, input_mask=mask)
    return step_fn


def _eager(model, k, batches):
    adv = icka_amd.Adversary(model, epsilon=EPS, recipe="fgm")
    fn = _step_fn(model, adv, k)
    opt = _optimizer(model)
    model.zero_grad()
    losses = []
    for i, b in enumerate(batches):
        losses.append(fn(*b).item())
        if (i + 1) % k == 0:
            opt.step()
            model.zero_grad()
    torch.cuda.synchronize()
    return losses, {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("k", [1, 3])
def test_fgm_train_step_equals_the_eager_recipe(k):
    base = _model("bf16")
    batches = _batches(k * OPT_STEPS)
    eager_model, model = copy.deepcopy(base), copy.deepcopy(base)
    le, pe = _eager(eager_model, k, batches)
    adv = icka_amd.Adversary(model, epsilon=EPS, recipe="fgm")
    opt = _optimizer(model)
    ts = icka_amd.TrainStep(model, _step_fn(model, adv, k), opt, inputs=batches[0], accumulate=k)
    lg = [ts(*b).item() for b in batches]
    torch.cuda.synchronize()
    pg = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert ts.stats["replays"] == len(batches) > 0 and ts.stats["eager"] == 0
    assert opt.steps_taken() == OPT_STEPS and opt.skipped_steps() == 0
    assert abs(le[-1] - le[0]) > 1e-5, "the weights moved"
    worst = _assert_close(le, pe, lg, pg, 2e-4)
    print("\n[FGM TrainStep k=%d] losses eager %s graphed %s; worst parameter difference %.3e" % (k, le, lg, worst))
    ts.close()


def test_fgm_graphed_step_equals_the_eager_recipe():
    base = _model("bf16")
    batches = _batches(OPT_STEPS)
    eager_model, model = copy.deepcopy(base), copy.deepcopy(base)
    le, pe = _eager(eager_model, 1, batches)
    adv = icka_amd.Adversary(model, epsilon=EPS, recipe="fgm")
    opt = _optimizer(model)
    gs = icka_amd.GraphedStep(model, _step_fn(model, adv, 1), inputs=batches[0])
    lg = []
    for b in batches:
        model.zero_grad()
        lg.append(gs(*b).item())
        opt.step()
    torch.cuda.synchronize()
    pg = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert gs.stats["replays"] == len(batches) > 0 and gs.stats["eager_calls"] == 0
    _assert_close(le, pe, lg, pg, 2e-4)
    gs.close()


def test_uniform_start_is_fresh_per_replay_and_reproducible():
    base = _model("bf16")
    b = _batches(1)[0]

    def first_two(seed):
        model = copy.deepcopy(base)
        adv = icka_amd.Adversary(model, epsilon=EPS, recipe="freelb", steps=1, init="uniform", seed=seed)
        gs = icka_amd.GraphedStep(model, _step_fn(model, adv, 1), inputs=b)
        out = []
        for _ in range(2):
            model.zero_grad()
            gs(*b)
            torch.cuda.synchronize()
            out.append(adv.delta.detach().clone())           # steps = 1: no ascent, delta is still delta_0
        assert gs.stats["replays"] == 2
        gs.close()
        return out

    d1, d2 = first_two(7)
    assert not torch.equal(d1, d2), "two replays on one batch draw different starts"
    v = (b[MASK] != 0)
    assert not bool(d1[~v].ne(0).any()) and float(d1[v].abs().max()) > 0
    e1, e2 = first_two(7)
    assert torch.equal(d1, e1) and torch.equal(d2, e2), "the same seed reproduces the bits"
    f1, _ = first_two(8)
    assert not torch.equal(d1, f1)


# ------------------------------------------------------------------------------------------------ wrappers, refusals, no adversary
def test_graphed_module_call_inside_a_pass_is_eager():
    model = _model("bf16")
    b = _batches(1)[0]
    args, kw = b[:-1], {"labels": b[-1]}
    adv = icka_amd.Adversary(model, epsilon=EPS)
    with torch.no_grad():
        gm = icka_amd.GraphedModule(model, args, kw)
        want = gm(*args, **kw).clone()
        before = dict(gm.stats)
        assert before["replays"] >= 1
        with adv.clean():
            got = gm(*args, **kw)
        assert gm.stats["eager_calls"] == before["eager_calls"] + 1 and gm.stats["replays"] == before["replays"]
        assert torch.equal(got, want), "a clean pass computes the plain forward"
        gm(*args, **kw)
        assert gm.stats["replays"] == before["replays"] + 1


def test_refusals_raise_before_any_launch(monkeypatch):
    from icka_amd import kernels as K
    model = _model("bf16")
    b = _distinct_batch()
    adv = icka_amd.Adversary(model, epsilon=EPS)
    _plain(model, b)                                   # the arena exists
    launches = []
    for name in ("embed_fwd_adv", "embed_fwd", "adv_ascend", "adv_init_uniform", "zero_", "gemm"):
        monkeypatch.setattr(K, name, (lambda n: lambda *a, **k: launches.append(n))(name))
    model._icka_arena.reducer = object()               # (what GradReducer does when it attaches)
    try:
        with pytest.raises(NotImplementedError, match="GradReducer"):
            adv.run(lambda: _loss_of(model, b), input_mask=b[MASK])
    finally:
        model._icka_arena.reducer = None
    icka_amd.set_precision(model, "fp32")
    with pytest.raises(NotImplementedError, match="fp32"):
        adv.run(lambda: _loss_of(model, b), input_mask=b[MASK])
    icka_amd.set_precision(model, "bf16")
    model._icka_packed = object()
    try:
        with pytest.raises(NotImplementedError, match="packed"):
            adv.run(lambda: _loss_of(model, b), input_mask=b[MASK])
    finally:
        del model._icka_packed
    assert launches == [] and model.bert.embeddings._icka_adv is None
    monkeypatch.undo()
    model.zero_grad()
    with adv.clean():
        _loss_of(model, b).backward()
    with pytest.raises(ValueError, match="input_mask"):
        adv.ascend(b[MASK][:, :16].contiguous())
    with pytest.raises(ValueError, match="input_mask"):
        adv.run(lambda: _loss_of(model, b), input_mask=b[MASK][:2].contiguous())
    assert model.bert.embeddings._icka_adv is None


def test_a_model_without_an_adversary_is_unchanged(monkeypatch):
    from icka_amd import ops
    base = _model("bf16")
    b = _distinct_batch()
    never, used = copy.deepcopy(base), copy.deepcopy(base)
    want_loss, want, tol = _noise(never, b)
    adv = icka_amd.Adversary(used, epsilon=EPS)
    used.zero_grad()
    adv.run(lambda: _loss_of(used, b), input_mask=b[MASK])
    monkeypatch.setattr(ops.EmbeddingsAdvFn, "apply", lambda *a, **k: pytest.fail("the adversarial path ran outside a pass"))
    loss, got = _plain(used, b)
    assert torch.equal(loss, want_loss)
    _close(got, want, tol, "a model whose adversary is idle against one that never had any")
