"""GPU: ArenaAdamW(capturable=True) -- step count, learning-rate schedule and bias corrections held in a device block
(include/icka_hip.h: icka_optim_state), a non-finite guard on the device, step() capturable into a graph -- and the two
launches under it (icka_optim_prepare, icka_optim_adamw_dev) on flat buffers.

Bars are those of tests/test_optim_gpu.py: parameters within 2e-6 * max(1, |ref|max) of clip_grad_norm_ + torch.optim.AdamW
(+ the linear LambdaLR) after every update, the norm within 1e-5 relative, shadows equal to the 16-bit cast of the parameters.
Everything that compares two runs of the SAME kernels on the same data is bitwise."""
import copy

import pytest
import torch

from icka_amd import synth

pytestmark = pytest.mark.gpu

BAR = 2e-6


def _model():
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36)
    synth.fill_module_(m)
    g = {k: v.cuda() for k, v in synth.synthetic_batch(4, 32, 36, vocab_size=512, seed=5).items()}
    args = (g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
            g["visual_embeds_att"])
    return m.cuda().eval(), args, g["labels"]


def _twins(n=2):
    """n models with bitwise the same parameters, each with its own arena and p.grad attached to it (one forward + backward)."""
    base, args, labels = _model()
    models = [base] + [copy.deepcopy(base) for _ in range(n - 1)]
    for m in models:
        m(*args, labels=labels).backward()
    torch.cuda.synchronize()
    return models, args, labels


def _grad_sets(A, n, seed=0):
    """n different flat gradient buffers: the model's own gradient plus noise of a tenth of its mean magnitude."""
    g0 = A.gflat.clone()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    scale = 0.1 * g0.abs().mean()
    return [g0 + scale * torch.randn(g0.shape, generator=gen, device="cuda") for _ in range(n)]


def _state_of(model, opt):
    A = model._icka_arena
    out = {"p": A.flat.clone(), "m": opt._m.clone(), "v": opt._v.clone(), "bf16": A.shadow.clone()}
    if A.shadow16 is not None:
        out["f16"] = A.shadow16.clone()
    return out


def _assert_bitwise(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32).item()


# ------------------------------------------------------------------------------------------------ the two launches, flat buffers
CH = 8192
G0 = (0, CH + 8)                 # group 0 (decayed): one full chunk + an 8-element tail chunk
HOLE = (CH + 8, CH + 72)         # a parameter without gradient: in no table
G1 = (CH + 72, CH + 72 + 1000)   # group 1 (not decayed)
TOTAL = G1[1]


def _flat_case(fp16):
    gen = torch.Generator(device="cuda").manual_seed(3)
    r = lambda s=1.0: s * torch.randn(TOTAL, generator=gen, device="cuda")       # noqa: E731
    buf = {"p": r(), "g": r(0.02), "m": r(0.01), "v": r(0.001).abs(),
           "bf16": torch.full((TOTAL,), 7.0, dtype=torch.bfloat16, device="cuda"),
           "f16": torch.full((TOTAL,), 7.0, dtype=torch.float16, device="cuda") if fp16 else None}
    buf["p"][5] = 7e4            # beyond the fp16 range: the fp16 shadow clamps
    return buf


def _upload(state, t, lrs=(1e-2, 2e-2), wds=(0.01, 0.0), schedule=("linear", 1, 4)):
    from icka_amd import _lib, kernels as K
    h = _lib.OptimState()
    h.t, h.kind, h.warmup, h.total, h.n_groups = t, _lib.OPTIM_SCHEDULE_LINEAR, schedule[1], schedule[2], 2
    for i in range(2):
        h.base_lr[i], h.beta1[i], h.beta2[i], h.eps[i], h.weight_decay[i] = lrs[i], 0.9, 0.999, 1e-8, wds[i]
    K.optim_state_write(state, h, 0, _lib.OptimState.HOST_HI)
    return h


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16-shadow", "bf16+fp16-shadows"])
def test_prepare_and_adamw_dev_on_flat_buffers(fp16):
    from icka_amd import kernels as K
    from icka_amd.optim import schedule_factor
    b = _flat_case(fp16)
    norm_table = K.dp_chunk_table([G0, G1], "cuda")
    table3 = K.optim_chunk_table3([[G0], [G1]], "cuda")
    assert table3.tolist() == [[0, CH, 0], [CH, 8, 0], [G1[0], 1000, 1]]
    partials = torch.empty(norm_table.shape[0], device="cuda")
    state = K.optim_state_new("cuda")
    _upload(state, t=2)
    # reference: torch.optim.AdamW over the two ranges with the moments installed, fed the clipped gradient, rate set by hand
    ref = [b["p"][lo:hi].clone().requires_grad_(True) for lo, hi in (G0, G1)]
    topt = torch.optim.AdamW([{"params": [ref[0]], "weight_decay": 0.01, "lr": 1e-2},
                              {"params": [ref[1]], "weight_decay": 0.0, "lr": 2e-2}])
    for r, (lo, hi) in zip(ref, (G0, G1)):
        topt.state[r] = {"step": torch.tensor(2.0), "exp_avg": b["m"][lo:hi].clone(), "exp_avg_sq": b["v"][lo:hi].clone()}
    hole_before = {k: b[k][HOLE[0]:HOLE[1]].clone() for k in b if b[k] is not None}
    clip2 = torch.empty(2, device="cuda")
    for upd in range(2):                     # updates number 3 and 4 of a ("linear", 1, 4) schedule: factors 2/3 and 1/3
        t = 2 + upd
        for r, (lo, hi) in zip(ref, (G0, G1)):
            r.grad = b["g"][lo:hi].clone()
        tn = torch.nn.utils.clip_grad_norm_(ref, 0.05)
        for grp, base in zip(topt.param_groups, (1e-2, 2e-2)):
            grp["lr"] = base * schedule_factor("linear", 1, 4, t)
        topt.step()
        K.optim_sqnorm(b["g"], norm_table, partials)
        K.check(K._lib.load().icka_optim_clip(partials.data_ptr(), partials.numel(), 0.05, clip2.data_ptr(), K._stream()), "clip")
        K.optim_prepare(partials, partials.numel(), 0.05, state)
        K.optim_adamw_dev(b["p"], b["g"], b["m"], b["v"], b["bf16"], b["f16"], table3, state)
        st = K.optim_state_read(state)
        assert (st.t, st.skipped, st.skip) == (t + 1, 0, 0)
        assert [st.norm, st.coef] == clip2.tolist(), "the norm and coefficient of icka_optim_clip, bitwise"
        assert abs(st.norm - tn.item()) < 1e-5 * tn.item()
        assert [st.lr[0], st.lr[1]] == [_f32(1e-2 * schedule_factor("linear", 1, 4, t)), _f32(2e-2 * schedule_factor("linear", 1, 4, t))]
        assert st.bc1[0] == pytest.approx(1 - _f32(0.9) ** (t + 1), rel=1e-6)
        assert st.bc2_sqrt[1] == pytest.approx((1 - _f32(0.999) ** (t + 1)) ** 0.5, rel=1e-6)
        for r, (lo, hi) in zip(ref, (G0, G1)):
            d = (b["p"][lo:hi] - r.detach()).abs()           # (the bar per element: one value of this case is 7e4)
            assert bool((d <= BAR * r.detach().abs().clamp(min=1.0)).all()), (upd, lo, d.max().item())
            assert torch.equal(b["bf16"][lo:hi], b["p"][lo:hi].to(torch.bfloat16))
            if fp16:
                assert torch.equal(b["f16"][lo:hi], b["p"][lo:hi].clamp(-65504.0, 65504.0).to(torch.float16))
    for k, v in hole_before.items():
        assert torch.equal(b[k][HOLE[0]:HOLE[1]], v), "the parameter without gradient was touched: %s" % k
    # a dry prepare and a non-finite norm: the update launch behind them touches nothing; only the non-finite one is counted
    before = {k: v.clone() for k, v in b.items() if v is not None}
    K.optim_sqnorm(b["g"], norm_table, partials)
    K.optim_prepare(partials, partials.numel(), 0.05, state, dry=True)
    K.optim_adamw_dev(b["p"], b["g"], b["m"], b["v"], b["bf16"], b["f16"], table3, state)
    st = K.optim_state_read(state)
    assert (st.t, st.skipped, st.skip) == (4, 0, 1)
    b["g"][CH + 3] = float("inf")            # in the 8-element tail chunk
    before["g"] = b["g"].clone()
    for max_norm in (0.05, 0.0):
        K.optim_sqnorm(b["g"], norm_table, partials)
        K.optim_prepare(partials, partials.numel(), max_norm, state)
        K.optim_adamw_dev(b["p"], b["g"], b["m"], b["v"], b["bf16"], b["f16"], table3, state)
    st = K.optim_state_read(state)
    assert (st.t, st.skipped, st.skip) == (4, 2, 1)
    for k, v in before.items():
        assert torch.equal(b[k], v), k
    # max_norm <= 0: no clipping, coefficient 1
    b["g"][CH + 3] = 0.5
    K.optim_sqnorm(b["g"], norm_table, partials)
    K.optim_prepare(partials, partials.numel(), 0.0, state)
    st = K.optim_state_read(state)
    assert (st.t, st.skip, st.coef) == (5, 0, 1.0) and st.lr[0] == 0.0      # (update 5 of 4: rate 0)


# ------------------------------------------------------------------------------------------------ 1. against torch
def test_eight_updates_match_torch_adamw_with_clipping_and_linear_schedule():
    """Warm-up 2 of 6 updates, so updates 7 and 8 run at rate 0.  Measured on an MI355X: worst relative parameter difference
    against torch 3.2e-7; the capturable and the host mode of ArenaAdamW, fed the same gradients, were bitwise equal over all
    eight updates (asserted only within the bar: the two kernels are separate compilations of the same expressions)."""
    from icka_amd.optim import ArenaAdamW, reference_param_groups, schedule_factor
    (model, host_model), args, labels = _twins(2)
    A = model._icka_arena
    A.shadow_policy = "tracked"
    WARM, TOTAL_STEPS, LR = 2, 6, 1e-2
    opt = ArenaAdamW(model, lr=LR, weight_decay=0.01, max_grad_norm=0.05, capturable=True, schedule=("linear", WARM, TOTAL_STEPS))
    hopt = ArenaAdamW(host_model, lr=LR, weight_decay=0.01, max_grad_norm=0.05)
    lam = lambda s: float(s) / max(1, WARM) if s < WARM else max(0.0, float(TOTAL_STEPS - s) / max(1, TOTAL_STEPS - WARM))  # noqa: E731
    hsched = torch.optim.lr_scheduler.LambdaLR(hopt, lam)
    names = [n for n, _ in model.named_parameters()]
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
    idx = {id(p): n for n, p in model.named_parameters()}
    topt = torch.optim.AdamW([{"params": [ref[idx[id(p)]] for p in g["params"]], "weight_decay": g["weight_decay"]}
                              for g in reference_param_groups(model, 0.01)], lr=LR)
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, lam)
    hparams = dict(host_model.named_parameters())
    worst, bitwise = 0.0, True
    for it in range(8):
        model.zero_grad()
        model(*args, labels=labels).backward()
        for n, p in model.named_parameters():
            ref[n].grad = None if p.grad is None else p.grad.detach().clone()
            hparams[n].grad = None if p.grad is None else p.grad.detach().clone()
        tn = torch.nn.utils.clip_grad_norm_([ref[n] for n in names if ref[n].grad is not None], 0.05)
        topt.step(); tsched.step()
        hopt.step(); hsched.step()
        opt.step()
        torch.cuda.synchronize()
        assert abs(opt.grad_norm().item() - tn.item()) < 1e-5 * tn.item()
        assert opt.current_lr() == [_f32(LR * schedule_factor("linear", WARM, TOTAL_STEPS, it))] * 2
        for n, p in model.named_parameters():
            bound = BAR * max(1.0, ref[n].detach().abs().max().item())
            d = (p.detach() - ref[n].detach()).abs().max().item()
            worst = max(worst, d / (ref[n].detach().abs().max().item() + 1e-12))
            assert d <= bound, (it, n, d)
            dh = (p.detach() - hparams[n].detach()).abs().max().item()
            assert dh <= bound, ("capturable vs host mode", it, n, dh)
            bitwise = bitwise and dh == 0.0
        for lo, hi in A._cast_ranges:
            assert torch.equal(A.shadow[lo:hi], A.flat[lo:hi].to(torch.bfloat16)), it
    assert opt.steps_taken() == 8 and opt.skipped_steps() == 0
    print("\n[capturable ArenaAdamW vs clip_grad_norm_ + torch.optim.AdamW + linear LambdaLR, 8 updates] worst relative parameter "
          "difference %.2e; capturable vs host mode bitwise: %s" % (worst, bitwise))


# ------------------------------------------------------------------------------------------------ 2. captured step()
def test_step_captured_once_and_replayed_equals_the_eager_capturable_run():
    from icka_amd.optim import ArenaAdamW, schedule_factor
    (me, mg), _, _ = _twins(2)
    Ae, Ag = me._icka_arena, mg._icka_arena
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, capturable=True, schedule=("linear", 2, 5))
    oe, og = ArenaAdamW(me, **kw), ArenaAdamW(mg, **kw)
    grads = _grad_sets(Ae, 6)
    for g in grads:
        Ae.gflat.copy_(g)
        oe.step()
    og.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    assert og.steps_taken() == 0, "a capture executes nothing"
    for i, g in enumerate(grads):
        Ag.gflat.copy_(g)
        graph.replay()
        assert og.current_lr() == [_f32(1e-2 * schedule_factor("linear", 2, 5, i))] * 2, i
    torch.cuda.synchronize()
    _assert_bitwise(_state_of(me, oe), _state_of(mg, og), "replayed vs eager")
    assert og.steps_taken() == oe.steps_taken() == 6
    assert torch.equal(og.grad_norm(), oe.grad_norm())
    assert og.current_lr() == [0.0, 0.0]       # update 6 of a 5-update schedule


# ------------------------------------------------------------------------------------------------ 3. non-finite guard
@pytest.mark.parametrize("max_grad_norm", [0.05, None], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_is_refused_on_the_device(bad, max_grad_norm):
    from icka_amd.optim import ArenaAdamW
    (model, twin), _, _ = _twins(2)
    A, B = model._icka_arena, twin._icka_arena
    for X in (A, B):
        X.enable_fp16_shadow()
        X.sync(force=True)
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=max_grad_norm, capturable=True, skip_nonfinite=True)
    opt, topt = ArenaAdamW(model, **kw), ArenaAdamW(twin, **kw)
    g0, g1 = _grad_sets(A, 2)
    for X, o in ((A, opt), (B, topt)):
        X.gflat.copy_(g0)
        o.step()
    before = _state_of(model, opt)
    assert "f16" in before
    A.gflat.copy_(g1)
    A.gflat[A.slots[id(model.classifier.weight)].off + 3] = bad
    opt.step()
    _assert_bitwise(before, _state_of(model, opt), "after the refused update")
    assert opt.steps_taken() == 1 and opt.skipped_steps() == 1 and topt.skipped_steps() == 0
    for X, o in ((A, opt), (B, topt)):
        X.gflat.copy_(g1)
        o.step()
    _assert_bitwise(_state_of(twin, topt), _state_of(model, opt), "the next finite update vs a twin that never saw the bad gradient")
    assert opt.steps_taken() == topt.steps_taken() == 2 and opt.skipped_steps() == 1
    assert not torch.equal(before["p"], A.flat)


# ------------------------------------------------------------------------------------------------ 4. checkpoints
def test_state_dict_round_trip_between_capturable_and_host_mode():
    from icka_amd.optim import ArenaAdamW
    model, args, labels = _model()
    twin = copy.deepcopy(model)

    def run(m, opt, n):
        for _ in range(n):
            m.zero_grad()
            m(*args, labels=labels).backward()
            opt.step()
        torch.cuda.synchronize()

    def fresh_copy(m):
        c = copy.deepcopy(m)
        for mod in c.modules():
            object.__setattr__(mod, "_icka_arena", None)     # a fresh process would build its own arena on the first forward
        return c

    kw = dict(lr=1e-2, max_grad_norm=1.0)
    full = ArenaAdamW(model, capturable=True, **kw)
    run(model, full, 4)
    first = ArenaAdamW(twin, capturable=True, **kw)
    run(twin, first, 2)
    sd = first.state_dict()
    assert sd["icka_t"] == 2 and sd["icka_m"].abs().sum().item() > 0
    m2 = fresh_copy(twin)
    second = ArenaAdamW(m2, **kw)                             # host mode
    second.load_state_dict(sd)
    run(m2, second, 1)
    sd2 = second.state_dict()
    assert sd2["icka_t"] == 3
    m3 = fresh_copy(m2)
    third = ArenaAdamW(m3, capturable=True, **kw)
    third.load_state_dict(sd2)                                # before the arena is bound: t reaches the device at the first step
    run(m3, third, 1)
    worst = max((p.detach() - q.detach()).abs().max().item() for p, q in zip(model.parameters(), m3.parameters()))
    assert worst < 1e-6, worst
    assert third.state_dict()["icka_t"] == 4 and third.steps_taken() == 4
    third.load_state_dict(sd)                                 # after the arena is bound: t is written to the device at once
    assert third.steps_taken() == 2
    bad = dict(sd)
    bad["icka_layout"] = [("x", 0, 8)]
    with pytest.raises(ValueError, match="another parameter layout"):
        third.load_state_dict(bad)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    from icka_amd.optim import ArenaAdamW
    (model,), _, _ = _twins(1)
    ps = [p for p in model.parameters()]
    with pytest.raises(ValueError, match="at most 8"):
        ArenaAdamW(model, [{"params": [p]} for p in ps[:9]], capturable=True)
    ArenaAdamW(model, [{"params": [p]} for p in ps[:9]])      # host mode has no such limit
    with pytest.raises(ValueError, match="capturable"):
        ArenaAdamW(model, schedule=("linear", 1, 2))
    opt = ArenaAdamW(model, lr=1e-2, capturable=True)
    with pytest.raises(RuntimeError, match="capturable"):
        ArenaAdamW(model, lr=1e-2).skipped_steps()
    # a capture before the tables exist, and a gradient set that changed inside a capture
    for prepare in (False, True):
        if prepare:
            opt.prepare_capture()
            model.classifier.bias.grad = None
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="inside a capture|before capturing"):
            with torch.cuda.graph(graph):
                opt.step()
        torch.cuda.synchronize()
    opt.step()                                               # outside a capture the tables are rebuilt
    assert opt.steps_taken() == 1
