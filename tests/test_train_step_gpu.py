"""GPU: icka_amd.TrainStep -- a whole accumulation cycle of the reference's recipe (My_cross_attention.py:797-844: k micro-batches
of loss / k + backward, then clip_grad_norm_(1.0), AdamW step, linear schedule step, zero_grad) replayed from captured graphs,
the update of a capturable ArenaAdamW included -- against the same recipe launched eagerly with the same step function, the
same kind of optimizer and the same schedule.  Bars are those of tests/test_recipe_gpu.py: 2e-6 in fp32 mode, 2e-4 in bf16
(dropout off: eval mode)."""
import copy

import pytest
import torch

import icka_amd
from icka_amd import synth

pytestmark = pytest.mark.gpu

OPT_STEPS = 2
NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")


def _model(precision):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36)
    synth.fill_module_(m)
    return icka_amd.set_precision(m.cuda().eval(), precision)


def _batches(n, B=4):
    out = []
    for i in range(n):
        b = synth.synthetic_batch(B, 32, 36, vocab_size=512, seed=100 + i)
        out.append(tuple(b[k].cuda() for k in NAMES))
    return out


def _optimizer(model, total=OPT_STEPS + 1, warm=1):
    from icka_amd.optim import ArenaAdamW
    return ArenaAdamW(model, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, capturable=True, schedule=("linear", warm, total))


def _micro_of(model, k):
    def micro(ids, seg, mask, added, vmean, vatt, labels):
        loss = model(ids, seg, mask, added, vmean, vatt, labels=labels) / k      # :821-822
        loss.backward()
        return loss
    return micro


def _eager_recipe(model, k, batches, total=OPT_STEPS + 1):
    """The reference's loop around the eager step function and a capturable optimizer."""
    opt = _optimizer(model, total)
    micro = _micro_of(model, k)
    model.zero_grad()
    losses = []
    for i, b in enumerate(batches):
        losses.append(micro(*b).item())
        if (i + 1) % k == 0:
            opt.step()
            model.zero_grad()
    torch.cuda.synchronize()
    return losses, {n: p.detach().clone() for n, p in model.named_parameters()}, opt


def _assert_close(le, pe, lg, pg, bar):
    for a, b in zip(le, lg):
        assert abs(a - b) <= bar * max(1.0, abs(a)), (le, lg)
    worst, wkey = 0.0, ""
    for n in pe:
        d = (pe[n] - pg[n]).abs().max().item() / (pe[n].abs().max().item() + 1e-6)
        if d > worst:
            worst, wkey = d, n
    assert worst <= bar, (worst, wkey)
    return worst


# ------------------------------------------------------------------------------------------------ 6. against the eager recipe
@pytest.mark.parametrize("k", [5, 1])
@pytest.mark.parametrize("precision,bar", [("fp32", 2e-6), ("bf16", 2e-4)])
def test_train_step_equals_the_eager_recipe(precision, bar, k):
    base = _model(precision)
    batches = _batches(k * OPT_STEPS)
    eager_model, model = copy.deepcopy(base), copy.deepcopy(base)
    le, pe, eopt = _eager_recipe(eager_model, k, batches)
    opt = _optimizer(model)
    ts = icka_amd.TrainStep(model, _micro_of(model, k), opt, inputs=batches[0], accumulate=k)
    assert ts.captures == (3 if k > 1 else 1) and ts.stats["captures"] == ts.captures
    lg = [ts(*b).item() for b in batches]
    torch.cuda.synchronize()
    pg = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert ts.stats["replays"] == len(batches) and ts.stats["eager"] == 0
    assert opt.steps_taken() == eopt.steps_taken() == OPT_STEPS and opt.skipped_steps() == 0
    assert opt.current_lr() == eopt.current_lr() and opt.current_lr()[0] > 0
    assert abs(le[-1] - le[0]) > 1e-5, "the weights moved"
    worst = _assert_close(le, pe, lg, pg, bar)
    print("\n[TrainStep %s k=%d] losses eager %s graphed %s; worst parameter difference %.3e (bar %.1e)"
          % (precision, k, ["%.6f" % x for x in le], ["%.6f" % x for x in lg], worst, bar))
    ts.close()


# ------------------------------------------------------------------------------------------------ 7. no trace
def test_construction_leaves_no_trace():
    model = _model("bf16")
    b = _batches(2)
    micro = _micro_of(model, 5)
    opt = _optimizer(model)
    micro(*b[0])
    opt.step()                              # moments and t are not trivial
    model.zero_grad()
    micro(*b[1])                            # gradients the caller holds
    torch.cuda.synchronize()
    A = model._icka_arena
    before = {"p": A.flat.clone(), "m": opt._m.clone(), "v": opt._v.clone(), "g": A.gflat.clone(), "bf16": A.shadow.clone()}
    held = [(p, p.grad, None if p.grad is None else p.grad.data_ptr()) for p in model.parameters()]
    live = [s.live for s in A.order]
    t, skipped = opt.steps_taken(), opt.skipped_steps()
    ts = icka_amd.TrainStep(model, micro, opt, inputs=b[0], accumulate=5)
    torch.cuda.synchronize()
    after = {"p": A.flat, "m": opt._m, "v": opt._v, "g": A.gflat, "bf16": A.shadow}
    for key in before:
        assert torch.equal(before[key], after[key]), key
    assert (opt.steps_taken(), opt.skipped_steps()) == (t, skipped) == (1, 0)
    for p, g, ptr in held:
        assert p.grad is g and (g is None or g.data_ptr() == ptr)
    assert [s.live for s in A.order] == live
    ts.close()


# ------------------------------------------------------------------------------------------------ 8. a short batch mid-cycle
def test_a_short_batch_runs_eagerly_at_its_position_of_the_cycle():
    k = 3
    base = _model("fp32")
    batches = _batches(2 * k)
    short = _batches(2 * k, B=3)
    batches[1] = short[1]                   # position 2 of the first cycle
    batches[2 * k - 1] = short[2 * k - 1]   # position k of the second one: the eager call also updates
    eager_model, model = copy.deepcopy(base), copy.deepcopy(base)
    le, pe, _ = _eager_recipe(eager_model, k, batches)
    opt = _optimizer(model)
    ts = icka_amd.TrainStep(model, _micro_of(model, k), opt, inputs=batches[0], accumulate=k)
    lg = [ts(*b).item() for b in batches]
    torch.cuda.synchronize()
    pg = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert ts.stats["eager"] == 2 and ts.stats["replays"] == 2 * k - 2 and ts.captures == 3
    assert opt.steps_taken() == 2
    _assert_close(le, pe, lg, pg, 2e-6)
    # the other train / eval mode: eager as well, never an exception
    model.train()
    assert torch.isfinite(ts(*batches[0])).item() and ts.stats["eager"] == 3
    model.eval()
    ts.reset_cycle()
    ts.close()


# ------------------------------------------------------------------------------------------------ 9. a NaN batch
def test_a_nan_micro_batch_skips_that_cycles_update_on_the_device():
    k = 2
    model = _model("bf16")
    batches = _batches(3 * k)
    bad = list(batches[2])
    vatt = bad[5].clone()
    vatt[1, 2, 3] = float("nan")
    bad[5] = vatt
    batches[2] = tuple(bad)                 # the first micro-batch of the second cycle
    opt = _optimizer(model, total=10, warm=0)      # (no warm-up: the first update already moves the weights)
    ts = icka_amd.TrainStep(model, _micro_of(model, k), opt, inputs=batches[0], accumulate=k)
    A = model._icka_arena
    p0 = A.flat.clone()
    for b in batches[:k]:
        ts(*b)
    p1, m1, v1, s1 = A.flat.clone(), opt._m.clone(), opt._v.clone(), A.shadow.clone()
    assert not torch.equal(p0, p1) and opt.steps_taken() == 1
    losses = [ts(*b).item() for b in batches[k:2 * k]]
    assert losses[0] != losses[0], "the loss of the NaN batch is NaN"
    assert opt.steps_taken() == 1 and opt.skipped_steps() == 1
    assert torch.equal(A.flat, p1) and torch.equal(opt._m, m1) and torch.equal(opt._v, v1) and torch.equal(A.shadow, s1)
    assert bool(torch.isfinite(A.flat).all())
    losses = [ts(*b).item() for b in batches[2 * k:]]
    assert all(x == x for x in losses)
    assert opt.steps_taken() == 2 and opt.skipped_steps() == 1
    assert not torch.equal(A.flat, p1) and bool(torch.isfinite(A.flat).all()) and bool(torch.isfinite(opt._v).all())
    assert ts.stats["eager"] == 0
    ts.close()


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_and_close():
    from icka_amd.optim import ArenaAdamW
    model = _model("bf16")
    b = _batches(1)[0]
    micro = _micro_of(model, 1)
    with pytest.raises(NotImplementedError, match="capturable"):
        icka_amd.TrainStep(model, micro, ArenaAdamW(model, lr=1e-3), inputs=b)
    with pytest.raises(NotImplementedError, match="capturable"):
        icka_amd.TrainStep(model, micro, torch.optim.AdamW(model.parameters()), inputs=b)
    opt = _optimizer(model)
    micro(*b)
    model.zero_grad()
    model._icka_arena.reducer = object()    # (what GradReducer does when it attaches)
    try:
        with pytest.raises(NotImplementedError, match="GradReducer"):
            icka_amd.TrainStep(model, micro, opt, inputs=b)
    finally:
        model._icka_arena.reducer = None
    with pytest.raises(ValueError):
        icka_amd.TrainStep(model, micro, opt, inputs=b, accumulate=0)
    ts = icka_amd.TrainStep(model, micro, opt, inputs=b, warmup=1)
    assert torch.isfinite(ts(*b)).item()
    with pytest.raises(TypeError):
        ts(*b[:-1])                         # wrong arity stays a TypeError: a wrong call, not a new shape
    ts.close()
    with pytest.raises(RuntimeError, match="closed"):
        ts(*b)
