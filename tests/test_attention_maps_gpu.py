"""GPU: attention maps.  icka_attn_probs against a float64 softmax of the same bf16 values (shapes across every instance, both flag
values, masks with an all-masked and a one-key sample, guard elements, determinism); the maps tied to what the forward used
(maps @ v == the module's context); the recorder on the fixture's ``cl`` model against the reference's own probabilities
(tests/golden/attention_maps_tiny.npz); no side effects on logits and gradients; refusals; the graphed wrapper's eager route."""
import numpy as np
import pytest
import torch

import icka_amd
from icka_amd import kernels as K
from icka_amd import synth
from attention_maps_oracle import (KERNEL_SHAPES as SHAPES, SENTINEL, build_model as _model, call_model as _call,
                                   kernel_case as _case, kernel_launch as _launch, kernel_ref as _ref, scale_qk_)

pytestmark = pytest.mark.gpu

# Kernel level: the error is f32 accumulation over 64 exact bf16 products, the f32 rounding of scale * s + mask and one exp.
# Measured maximum over the shapes and both flag values below on MI355X: KERNEL_ERR_MEASURED (profiles/attention_maps.txt);
# the bar is 4x that, as headroom for other inputs of the same scale, and must stay below 1e-4.
KERNEL_ERR_MEASURED = 7.945e-8
KERNEL_BAR = 4.0 * KERNEL_ERR_MEASURED
MODEL_BAR = 2e-2    # the project's bf16 parity bar; probabilities lie in [0, 1] and dP <= 1/4 d(score)

@pytest.mark.parametrize("mean", [False, True], ids=["all", "head_mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_against_float64_softmax(shape, mean):
    B, heads, Sq, Skv = shape
    qb, kb, add, H = _case(B, heads, Sq, Skv)
    ref = _ref(qb, kb, add, B, heads, Sq, Skv, H)
    if mean:
        ref = ref.mean(dim=1)
    P, before, after = _launch(qb, kb, add, B, heads, Sq, Skv, H, mean)
    torch.cuda.synchronize()
    err = (P.double().cpu() - ref).abs().max().item()
    rows = (P.double().sum(-1) - 1.0).abs().max().item()
    print("\n[attn_probs %s %s] max abs err %.3e, max |row sum - 1| %.3e" % (shape, "mean" if mean else "all", err, rows))
    assert torch.all(before == SENTINEL) and torch.all(after == SENTINEL), "guard elements around P were written"
    assert torch.isfinite(P).all()
    P2, _b, _a = _launch(qb, kb, add, B, heads, Sq, Skv, H, mean)
    assert torch.equal(P, P2), "two runs differ"
    assert KERNEL_BAR <= 1e-4
    assert err <= KERNEL_BAR, err
    assert rows <= 4e-6 + KERNEL_BAR


def test_kernel_unaligned_output_takes_the_scalar_stores():
    """Skv % 4 == 0 but P only 4-byte aligned: the same values as the 16-byte store path, guards untouched."""
    B, heads, Sq, Skv = 2, 2, 32, 32
    qb, kb, add, H = _case(B, heads, Sq, Skv, seed=1)
    for mean in (False, True):
        P0, _b, _a = _launch(qb, kb, add, B, heads, Sq, Skv, H, mean)
        P1, before, after = _launch(qb, kb, add, B, heads, Sq, Skv, H, mean, offset=1)
        assert P1.data_ptr() % 16 == 4
        assert torch.equal(P0, P1)
        assert torch.all(before == SENTINEL) and torch.all(after == SENTINEL)


def test_kernel_wrapper_refusals():
    qb, kb, add, H = _case(1, 1, 8, 513)
    with pytest.raises(ValueError, match="512"):
        K.attn_probs(qb.cuda()[:, 64:64 + H], kb.cuda()[:, H:2 * H], add.cuda(), 1, 1, 8, 513)
    qb, kb, add, H = _case(1, 1, 8, 16)
    with pytest.raises(TypeError):       # CPU tensors: no CPU path
        K.attn_probs(qb[:, 64:64 + H], kb[:, H:2 * H], add, 1, 1, 8, 16)
    q, k = qb.cuda()[:, 64:64 + H], kb.cuda()[:, H:2 * H]
    with pytest.raises(ValueError):      # too few key rows for B * Skv
        K.attn_probs(q, k, torch.zeros(1, 32, device="cuda"), 1, 1, 8, 32)
    with pytest.raises(ValueError):      # mask of another shape
        K.attn_probs(q, k, torch.zeros(1, 15, device="cuda"), 1, 1, 8, 16)
    with pytest.raises(ValueError):      # out of the wrong size
        K.attn_probs(q, k, add.cuda(), 1, 1, 8, 16, out=torch.zeros(7, device="cuda"))
    lib = K._lib.load()
    P, add_d = torch.zeros(8 * 16, device="cuda"), add.cuda()
    args = (q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), add_d.data_ptr(), P.data_ptr())
    assert lib.icka_attn_probs(*args, 1, 1, 8, 513, 0.125, 0, None) == -1          # ICKA_E_SHAPE
    assert lib.icka_attn_probs(*args, 1, 1, 8, 16, 0.125, 2, None) == -3           # unknown flag: ICKA_E_ARG
    assert lib.icka_attn_probs(None, q.stride(0), *args[2:], 1, 1, 8, 16, 0.125, 0, None) == -3
    assert lib.icka_attn_probs(q.data_ptr() + 2, *args[1:], 1, 1, 8, 16, 0.125, 0, None) == -2   # ICKA_E_ALIGN
    assert lib.icka_attn_probs(q.data_ptr(), 12, *args[2:], 1, 1, 8, 16, 0.125, 0, None) == -2
    torch.cuda.synchronize()
    assert torch.all(P == 0)


# ------------------------------------------------------------------------------------------ tied to the forward
def _tiny_config(hidden=128, heads=2):
    from icka_amd.config import BertConfig
    return BertConfig(512, hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=256,
                      max_position_embeddings=128)


@pytest.mark.parametrize("kind", ["self", "co", "fused"])
def test_maps_times_v_is_the_modules_context(kind, monkeypatch):
    """maps @ v, re-merged over heads, equals the module's context within 2^-7 max|v| (the bf16 roundings of v, P and the
    output, each <= 2^-9 relative): fails for a wrong head, a transposed map or a wrong mask row.  "fused": a self-attention
    at a shape that the one-launch projection + attention (icka_gemm_qkv_attn) takes -- 128 tokens per sample, 8192 rows,
    128 (256-row, head) tiles -- where the recorder reads q / k as column slices of the launch's qkv output."""
    from icka_amd import ops
    from icka_amd.modeling import BertCoAttention, BertSelfAttention
    B, S, T, H, heads = (64, 128, 0, 256, 4) if kind == "fused" else (3, 40, 49, 128, 2)
    cfg = _tiny_config(hidden=H, heads=heads)
    fused_calls = []
    real = ops.K.gemm_qkv_attn
    monkeypatch.setattr(ops.K, "gemm_qkv_attn", lambda *a, **kw: fused_calls.append(real(*a, **kw)) or fused_calls[-1])
    mod = (BertCoAttention if kind == "co" else BertSelfAttention)(cfg)
    synth.fill_module_(mod)
    scale_qk_(mod, 8.0)
    with torch.no_grad():
        mod.value.weight.mul_(20.0)      # values of unit order
    mod = mod.cuda().eval()
    g = torch.Generator().manual_seed(3)
    x = torch.empty(B, S, H).normal_(0, 1, generator=g).to(torch.bfloat16).cuda()
    Tk = T if kind == "co" else S
    src = torch.empty(B, T, H).normal_(0, 1, generator=g).to(torch.bfloat16).cuda() if kind == "co" else x
    m01 = torch.ones(B, Tk)
    m01[1, Tk // 2:] = 0
    m01[2] = 0
    m01[2, 3] = 1
    ext = ((1.0 - m01) * -10000.0)[:, None, None, :].cuda()
    with torch.no_grad(), icka_amd.attention_maps(mod, heads="all") as rec:
        ctx = mod(x, src, ext) if kind == "co" else mod(x, ext)
    assert fused_calls == ([True] if kind == "fused" else []), "the fused launch ran exactly where the case means it to"
    assert rec.names == [""] and len(rec[""]) == 1
    P = rec[""][0]
    assert tuple(P.shape) == (B, heads, S, Tk) and P.dtype == torch.float32 and not P.requires_grad
    with torch.no_grad():
        v = src.float().view(-1, H) @ mod.value.weight.to(torch.bfloat16).float().t() + mod.value.bias.float()
        vh = v.view(B, Tk, heads, 64).permute(0, 2, 1, 3)
        want = torch.matmul(P, vh).permute(0, 2, 1, 3).reshape(B, S, H)
    bound = 2.0 ** -7 * v.abs().max().item()
    err = (ctx.float() - want).abs().max().item()
    print("\n[%s] |maps @ v - context| max %.3e (bound %.3e, max|v| %.3f, mean row max %.3f)"
          % (kind, err, bound, v.abs().max().item(), P.max(-1).values.mean().item()))
    assert P.max(-1).values.mean().item() > 0.2      # peaked maps: a uniform map would not pass below
    assert err <= bound


# ------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("precision", ["bf16", "mixed16"])
def test_recorder_against_the_reference_fixture(precision):
    model, batch, exp, names = _model(precision)
    model.eval()
    worst = {}
    for heads in ("all", "mean"):
        with torch.no_grad(), icka_amd.attention_maps(model, heads=heads) as rec:
            _call(model, batch)
            _call(model, batch)
        assert rec.names == names                       # the reference's hooked modules, in its module order
        for n in names:
            assert len(rec[n]) == 2 and torch.equal(rec[n][0], rec[n][1])      # one entry per forward call, in call order
            want = exp[heads + "/" + n]
            got = rec[n][0]
            assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and not got.requires_grad
            worst[(heads, n)] = float(np.abs(got.cpu().numpy() - want).max())
    for k, v in worst.items():
        print("\n[%s] %-5s %-44s max abs err %.3e (bar %.0e)" % (precision, k[0], k[1], v, MODEL_BAR))
    assert max(worst.values()) < MODEL_BAR, worst


def test_select_by_name_predicate_and_unknown_name():
    model, batch, _exp, names = _model()
    model.eval()
    cross = "txt2img_attention.layer.0.attention.self"
    with torch.no_grad(), icka_amd.attention_maps(model, select=[cross]) as rec:
        _call(model, batch)
    assert rec.names == [cross] and tuple(rec[cross][0].shape) == (3, 32, 49)
    with torch.no_grad(), icka_amd.attention_maps(model, heads="all", select=lambda n: n.startswith("bert.")) as rec:
        _call(model, batch)
    assert rec.names == names[:2] and all(len(rec[n]) == 1 for n in rec.names)
    with pytest.raises(KeyError):
        with icka_amd.attention_maps(model, select=["bert.encoder.layer.7.attention.self"]):
            pass
    with pytest.raises(ValueError):
        icka_amd.attention_maps(model, heads="sum")
    from icka_amd.attention_maps import active
    assert not active()
    with icka_amd.attention_maps(model) as outer:       # nested: the innermost records, leaving restores the outer one
        with torch.no_grad(), icka_amd.attention_maps(model, select=[cross]) as inner:
            _call(model, batch)
        assert active() and len(inner[cross]) == 1 and all(len(outer[n]) == 0 for n in names)
    assert not active()


def test_no_side_effects_on_logits_and_gradients():
    model, batch, _exp, names = _model()
    model.eval()
    with torch.no_grad():
        plain = _call(model, batch).clone()
        with icka_amd.attention_maps(model) as rec:
            recorded = _call(model, batch).clone()
    assert torch.equal(plain, recorded) and len(rec[names[0]]) == 1
    model.train()
    A = model._icka_arena

    def step(record):
        model.zero_grad()
        A.set_seed(1234)
        if record:
            with icka_amd.attention_maps(model, heads="all") as r:
                loss = _call(model, batch, labels=True)
                loss.backward()
            assert all(len(r[n]) == 1 and not r[n][0].requires_grad for n in names)
        else:
            loss = _call(model, batch, labels=True)
            loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    l0, g0 = step(False)
    l1, g1 = step(True)
    l2, g2 = step(False)
    diff_rec = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    diff_plain = [k for k in g0 if not torch.equal(g0[k], g2[k])]
    print("\n[no side effects] losses %r %r %r; gradients differing with recorder: %s; between two plain steps: %s"
          % (l0.item(), l1.item(), l2.item(), diff_rec, diff_plain))
    assert torch.equal(l0, l1)
    assert sorted(g0) == sorted(g1) and not diff_rec
    with torch.no_grad():                  # train-mode logits (dropout on): same seeds -> same bits
        A.set_seed(99)
        t0 = _call(model, batch).clone()
        A.set_seed(99)
        with icka_amd.attention_maps(model) as rec:
            t1 = _call(model, batch).clone()
    assert torch.equal(t0, t1)
    for n in names:                        # pre-dropout probabilities: whole distributions also in train mode
        assert (rec[n][0].double().sum(-1) - 1.0).abs().max().item() < 1e-5


def test_refusals():
    from icka_amd.modeling import BertSelfAttention
    model, batch, _exp, _names = _model()
    model.eval()
    icka_amd.set_packed(model, 128)
    with pytest.raises(NotImplementedError, match="packed"):
        with icka_amd.attention_maps(model):
            pass
    icka_amd.set_packed(model, None)
    icka_amd.set_precision(model, "fp32")
    with pytest.raises(NotImplementedError, match="fp32"):
        with torch.no_grad(), icka_amd.attention_maps(model):
            _call(model, batch)
    small = BertSelfAttention(_tiny_config(hidden=64, heads=2))      # head size 32: the generic f32 attention path
    synth.fill_module_(small)
    small = small.cuda().eval()
    x = torch.zeros(2, 16, 64, dtype=torch.bfloat16, device="cuda")
    ext = torch.zeros(2, 1, 1, 16, device="cuda")
    with torch.no_grad():
        small(x, ext)                                                 # runs without a recorder
        with pytest.raises(NotImplementedError, match="head size"):
            with icka_amd.attention_maps(small):
                small(x, ext)
    from icka_amd.attention_maps import active
    assert not active()


def test_graphed_module_runs_eagerly_under_the_recorder():
    model, batch, _exp, names = _model()
    model.eval()
    args = (batch["input_ids"], batch["segment_ids"], batch["input_mask"], batch["added_attention_mask"],
            batch["visual_embeds_mean"], batch["visual_embeds_att"])
    with torch.no_grad():
        gm = icka_amd.GraphedModule(model, args)
        replayed = gm(*args).clone()
        captures, stats = gm.captures, dict(gm.stats)
        assert stats["replays"] == 1 and stats["eager_calls"] == 0
        with icka_amd.attention_maps(gm, heads="all") as rec:
            eager = gm(*args).clone()
        assert gm.captures == captures and gm.stats["eager_calls"] == 1 and gm.stats["replays"] == 1
        assert rec.names == names and all(len(rec[n]) == 1 for n in names)
        assert torch.equal(replayed, eager)
        again = gm(*args).clone()          # ... and replays again afterwards
        assert gm.stats["replays"] == 2 and torch.equal(again, replayed)
    gm.close()


# ------------------------------------------------------------------------------------------ captured steps take their eager route
STEP_NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")
STEP_BAR = 2e-4     # eager against replayed step in bf16 with dropout off: the bar of tests/test_recipe_gpu.py / test_train_step_gpu.py


def _grads(model):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _worst_rel(a, b):
    assert sorted(a) == sorted(b)
    return max((a[n].float() - b[n].float()).abs().max().item() / (a[n].float().abs().max().item() + 1e-6) for n in a)


def test_graphed_step_runs_eagerly_under_the_recorder():
    """A captured GraphedStep called inside a recorder -- as gs(*batch) and as gs() on its static buffers -- launches step_fn
    from Python: maps are recorded, no capture and no replay is made, loss and gradients are those of the replayed step."""
    model, batch, _exp, names = _model()
    model.eval()                                            # dropout off: replayed and eager steps compute the same function
    inputs = tuple(batch[k] for k in STEP_NAMES)

    def step_fn(ids, seg, mask, added, vmean, vatt, labels):
        loss = model(ids, seg, mask, added, vmean, vatt, labels=labels)
        loss.backward()
        return loss

    gs = icka_amd.GraphedStep(model, step_fn, inputs=inputs)
    model.zero_grad()
    loss_r = gs(*inputs).detach().clone()
    grads_r = _grads(model)
    captures, stats = gs.captures, dict(gs.stats)
    assert stats["replays"] == 1 and stats["eager_calls"] == 0
    for n_call, call_args in enumerate((inputs, ())):
        model.zero_grad()
        with icka_amd.attention_maps(model, heads="all") as rec:
            loss_e = gs(*call_args).detach().clone()
        grads_e = _grads(model)
        assert rec.names == names and all(len(rec[n]) == 1 and not rec[n][0].requires_grad for n in names)
        assert gs.captures == captures and gs.stats["captures"] == stats["captures"]
        assert gs.stats["replays"] == 1 and gs.stats["eager_calls"] == n_call + 1
        worst = _worst_rel(grads_r, grads_e)
        print("\n[GraphedStep under the recorder, %s] loss replayed %.7f eager %.7f; worst gradient difference %.3e (bar %.0e)"
              % ("gs(*batch)" if call_args else "gs()", loss_r.item(), loss_e.item(), worst, STEP_BAR))
        assert abs(loss_e.item() - loss_r.item()) <= STEP_BAR * max(1.0, abs(loss_r.item()))
        assert worst <= STEP_BAR
    model.zero_grad()
    assert torch.equal(gs(*inputs).detach(), loss_r) and gs.stats["replays"] == 2 and gs.captures == captures   # replays again
    gs.close()


def test_train_step_runs_eagerly_under_the_recorder():
    """Two cycles of k = 2: the update call of the first cycle and the first call of the second run inside a recorder.  They
    take TrainStep's eager route at their position of the cycle; losses, parameters, optimizer steps and the position are
    those of a TrainStep that replayed every call."""
    import copy
    from icka_amd.optim import ArenaAdamW
    base, _batch, _exp, names = _model()
    base.eval()
    k = 2
    batches = []
    for i in range(2 * k):
        b = synth.synthetic_batch(3, 32, 49, vocab_size=512, seed=100 + i)
        batches.append(tuple(b[n].cuda() for n in STEP_NAMES))

    def build(model):
        opt = ArenaAdamW(model, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, capturable=True, schedule=("linear", 1, 3))

        def micro(ids, seg, mask, added, vmean, vatt, labels):
            loss = model(ids, seg, mask, added, vmean, vatt, labels=labels) / k
            loss.backward()
            return loss
        return icka_amd.TrainStep(model, micro, opt, inputs=batches[0], accumulate=k), opt

    ref_model, model = copy.deepcopy(base), copy.deepcopy(base)
    ts_ref, opt_ref = build(ref_model)
    ref_losses, ref_pos = [], []
    for b in batches:
        ref_losses.append(ts_ref(*b).item())
        ref_pos.append(ts_ref._pos)
    assert ts_ref.stats["eager"] == 0 and ts_ref.stats["replays"] == 2 * k
    ts, opt = build(model)
    captures = ts.captures
    losses, pos, recorded = [], [], {n: 0 for n in names}
    for i, b in enumerate(batches):
        if i in (k - 1, k):
            with icka_amd.attention_maps(model) as rec:
                losses.append(ts(*b).item())
            for n in names:
                assert len(rec[n]) == 1
                recorded[n] += 1
        else:
            losses.append(ts(*b).item())
        pos.append(ts._pos)
    torch.cuda.synchronize()
    assert all(v == 2 for v in recorded.values())
    assert ts.stats["eager"] == 2 and ts.stats["replays"] == 2 * k - 2 and ts.captures == captures == ts.stats["captures"]
    assert pos == ref_pos == [1, 0, 1, 0]
    assert opt.steps_taken() == opt_ref.steps_taken() == 2 and opt.skipped_steps() == 0
    assert opt.current_lr() == opt_ref.current_lr()
    pr = {n: p.detach() for n, p in ref_model.named_parameters()}
    pg = {n: p.detach() for n, p in model.named_parameters()}
    worst = max((pr[n] - pg[n]).abs().max().item() / (pr[n].abs().max().item() + 1e-6) for n in pr)
    print("\n[TrainStep under the recorder] losses replayed %s, with two eager calls %s; worst parameter difference %.3e (bar %.0e)"
          % (["%.6f" % x for x in ref_losses], ["%.6f" % x for x in losses], worst, STEP_BAR))
    assert abs(ref_losses[-1] - ref_losses[0]) > 1e-5, "the weights moved"
    for a, b in zip(ref_losses, losses):
        assert abs(a - b) <= STEP_BAR * max(1.0, abs(a))
    assert worst <= STEP_BAR
    ts.close()
    ts_ref.close()
