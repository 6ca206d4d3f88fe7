"""GPU: sharpness-aware minimisation on the parameter arena -- icka_sam_sqnorm, icka_sam_prepare, icka_sam_ascend and
icka_sam_restore on flat buffers, element by element against the float64 oracle of tests/sam_oracle.py, and icka_amd.SAM on the
two-layer tagger of tests/test_optim_capturable_gpu.py (eval mode: no dropout): run() against the hand-run launches and against a
twin placed at the perturbed weights, the optimizer step behind it, TrainStep with run() in the step function, the refusals.

Bars are the oracle's (its docstring derives them): the norm within 2^-24 times the depth of one chunk's summation tree (20
plain, 21 adaptive), p' within 2^-24 (k |e| + |p'|) + |e| * the norm's bar, k = 1 plain / 3 adaptive.  Measured on an MI355X at
the values below (N(0,1) * {1e-3, 1, 30}, gradients 0.02 of that): the norm reached 0.012 (plain) / 0.016 (adaptive) of its bar,
the per-chunk partials 0.08 / 0.13 of theirs, p' 0.989 / 0.987 of its bar -- the last rounding alone, p + e, reaches 2^-24 |p'|
for a mantissa just above a power of two, so that bar has no slack to give.  Everything that compares a copy, a restore, a
16-bit cast, an untouched element or two runs of the same launches on the same data is bitwise."""
import copy

import numpy as np
import pytest
import torch

import sam_oracle as SO
from test_optim_capturable_gpu import _model, _twins

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ flat buffers
CH = 8192
CHUNKS = [(64, 8), (128, 8184), (8448, CH), (20000, CH), (40944, 8)]      # (first element, count): ragged, not adjacent
TOTAL = 40960
P_OUT, G_OUT, BACKUP_FILL, SH_OUT = 777.0, 3e38, 555.0, 7.0               # sentinels; a gradient read outside the table -> inf norm
RHO = {False: 0.05, True: 1.0}


def _mask():
    m = torch.zeros(TOTAL, dtype=torch.bool, device="cuda")
    for lo, n in CHUNKS:
        m[lo:lo + n] = True
    return m


def _table():
    return torch.tensor(CHUNKS, dtype=torch.int64, device="cuda")


def _f64(t):
    return t.detach().double().cpu().numpy()


def _case(shadows, seed=11):
    """Parameters N(0,1) * {1e-3, 1, 30} by element, gradients 0.02 of that (of other draws), sentinels wherever the table does
    not reach; two parameters beyond the fp16 range (where |p| g is small: they do not carry the adaptive norm)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mask = _mask()
    scale = torch.tensor([1e-3, 1.0, 30.0], device="cuda")[torch.arange(TOTAL, device="cuda") % 3]
    p = scale * torch.randn(TOTAL, generator=gen, device="cuda")
    g = 0.02 * scale * torch.randn(TOTAL, generator=gen, device="cuda")
    p[129], p[132] = 7e4, -7e4
    p[~mask], g[~mask] = P_OUT, G_OUT
    b = {"p": p, "g": g, "backup": torch.full((TOTAL,), BACKUP_FILL, device="cuda"), "bf16": None, "f16": None, "mask": mask}
    if shadows >= 1:
        b["bf16"] = torch.where(mask, p.to(torch.bfloat16), torch.full_like(p, SH_OUT, dtype=torch.bfloat16))
    if shadows >= 2:
        b["f16"] = torch.where(mask, p.clamp(-65504.0, 65504.0).to(torch.float16), torch.full_like(p, SH_OUT, dtype=torch.float16))
    return b


def _clone(b):
    return {k: (None if v is None else v.clone()) for k, v in b.items()}


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)      # (a NaN equals itself bit for bit)


def _assert_same(a, b, what, keys=("p", "g", "backup", "bf16", "f16")):
    for k in keys:
        if a[k] is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("shadows", [0, 1, 2], ids=["no-shadow", "bf16-shadow", "bf16+fp16-shadows"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_ascent_and_restore_on_flat_buffers_against_float64(adaptive, shadows):
    from icka_amd import kernels as K
    rho = RHO[adaptive]
    b0 = _case(shadows)
    b = _clone(b0)
    mask, table = b["mask"], _table()
    m = mask.cpu().numpy()
    ref = SO.ascend(b0["p"].cpu().numpy(), b0["g"].cpu().numpy(), CHUNKS, rho, adaptive)
    state = K.sam_state_new("cuda")
    partials = torch.full((len(CHUNKS) + 1,), -1.0, device="cuda")
    # -- norm
    K.sam_sqnorm(b["p"], b["g"], table, partials, adaptive)
    assert partials[-1].item() == -1.0, "one partial per chunk"
    if not adaptive:
        want = torch.empty(len(CHUNKS), device="cuda")
        K.optim_sqnorm(b["g"], table, want)
        assert torch.equal(partials[:-1], want), "adaptive = 0: the partials of icka_optim_sqnorm, bitwise"
    pref = SO.partials(b0["p"].cpu().numpy(), b0["g"].cpu().numpy(), CHUNKS, adaptive)
    perr = np.abs(_f64(partials[:-1]) - pref) / pref
    pbar = np.array([2.0 ** -24 * SO.tree_depth(adaptive, n) for _, n in CHUNKS])
    assert (perr <= pbar).all(), (perr / pbar).tolist()
    K.sam_prepare(partials, len(CHUNKS), rho, state)
    st = K.sam_state_read(state)
    assert (st.skip, st.ascents, st.skipped) == (0, 1, 0)
    nerr = abs(float(st.norm) - ref["norm"]) / ref["norm"]
    assert nerr <= ref["norm_bar"], (nerr, ref["norm_bar"])
    assert st.scale == np.float32(float(np.float32(rho)) / (float(st.norm) + 1e-12)), "the scale of the header, from the f32 norm"
    _assert_same(b, b0, "norm and prepare only read")
    # -- ascend
    K.sam_ascend(b["p"], b["g"], b["backup"], b["bf16"], b["f16"], table, state, adaptive)
    err = np.abs(_f64(b["p"]) - ref["p_new"])[m]
    frac = err / ref["bar"][m]
    assert (frac <= 1.0).all(), float(frac.max())
    moved = (b["p"] != b0["p"])[mask].float().mean().item()
    assert moved > (0.3 if adaptive else 0.9), "the ascent moved the weights (%.2f of them)" % moved
    assert torch.equal(b["backup"][mask], b0["p"][mask]), "backup = the old p, bitwise"
    assert bool((b["backup"][~mask] == BACKUP_FILL).all()) and bool((b["p"][~mask] == P_OUT).all()), "outside the table"
    assert torch.equal(b["g"], b0["g"]), "the gradient is only read"
    if b["bf16"] is not None:
        assert torch.equal(b["bf16"][mask], b["p"][mask].to(torch.bfloat16)) and bool((b["bf16"][~mask] == SH_OUT).all())
    if b["f16"] is not None:
        assert torch.equal(b["f16"][mask], b["p"][mask].clamp(-65504.0, 65504.0).to(torch.float16))
        assert bool((b["f16"][~mask] == SH_OUT).all())
        assert b["f16"][129].item() == 65504.0 and b["f16"][132].item() == -65504.0, "the fp16 clamp"
    print("\n[%s, %d shadows] norm error / bar = %.3f; worst p' error / bar = %.3f; worst partial / bar = %.3f"
          % ("adaptive" if adaptive else "plain", shadows, nerr / ref["norm_bar"], float(frac.max()), float((perr / pbar).max())))
    # -- restore
    after_ascent = b["backup"].clone()
    K.sam_restore(b["p"], b["backup"], b["bf16"], b["f16"], table, state)
    _assert_same(b, b0, "after restore", keys=("p", "g", "bf16", "f16"))
    assert torch.equal(b["backup"], after_ascent), "restore only reads the backup"
    st = K.sam_state_read(state)
    assert (st.skip, st.ascents, st.skipped) == (0, 1, 0)


@pytest.mark.parametrize("why", ["zero", "inf", "nan", "dry"])
def test_refused_ascents_touch_nothing(why):
    from icka_amd import kernels as K
    table = _table()
    for adaptive in (False, True):
        b0 = _case(2, seed=5)
        if why == "zero":
            b0["g"][b0["mask"]] = 0.0
        elif why == "inf":
            b0["g"][9000] = float("inf")
        elif why == "nan":
            b0["g"][20007] = float("nan")
        b = _clone(b0)
        state = K.sam_state_new("cuda")
        partials = torch.empty(len(CHUNKS), device="cuda")
        if why == "dry":        # an applied ascent first, so that the counters and the scale have something to keep
            K.sam_sqnorm(b["p"], b["g"], table, partials, adaptive)
            K.sam_prepare(partials, len(CHUNKS), 0.05, state)
            before = K.sam_state_read(state)
            assert (before.skip, before.ascents, before.skipped) == (0, 1, 0)
        K.sam_sqnorm(b["p"], b["g"], table, partials, adaptive)
        K.sam_prepare(partials, len(CHUNKS), 0.05, state, dry=(why == "dry"))
        K.sam_ascend(b["p"], b["g"], b["backup"], b["bf16"], b["f16"], table, state, adaptive)
        _assert_same(b, b0, "%s, after the refused ascent" % why)
        K.sam_restore(b["p"], b["backup"], b["bf16"], b["f16"], table, state)
        _assert_same(b, b0, "%s, after the restore behind it" % why)
        assert bool((b["backup"] == BACKUP_FILL).all()), "the backup was never written"
        st = K.sam_state_read(state)
        assert st.skip == 1
        if why == "dry":
            assert (st.ascents, st.skipped, st.scale, st.norm) == (1, 0, before.scale, before.norm), "a dry prepare counts nothing"
        else:
            assert (st.ascents, st.skipped, st.scale) == (0, 1, 0.0)
            assert SO.ascend(b0["p"].cpu().numpy(), b0["g"].cpu().numpy(), CHUNKS, 0.05, adaptive)["skip"]
            assert (st.norm == 0.0) if why == "zero" else not np.isfinite(st.norm)


def test_wrapper_operand_checks():
    from icka_amd import kernels as K
    b, table, state = _case(2), _table(), K.sam_state_new("cuda")
    partials = torch.empty(len(CHUNKS), device="cuda")
    with pytest.raises(ValueError, match="rho"):
        K.sam_prepare(partials, len(CHUNKS), 0.0, state)
    with pytest.raises(ValueError, match="separate"):
        K.sam_ascend(b["p"], b["g"], b["p"], b["bf16"], b["f16"], table, state, False)
    with pytest.raises(TypeError):
        K.sam_ascend(b["p"], b["g"], b["backup"][:-8], b["bf16"], b["f16"], table, state, False)
    with pytest.raises(TypeError):
        K.sam_ascend(b["p"], b["g"], b["backup"], b["f16"], None, table, state, False)       # an fp16 tensor as the bf16 shadow
    with pytest.raises(TypeError):
        K.sam_restore(b["p"], b["backup"], b["bf16"], b["f16"], table.to(torch.int32), state)
    with pytest.raises(TypeError):
        K.sam_restore(b["p"], b["backup"], b["bf16"], b["f16"], table, K.optim_state_new("cuda"))   # another block
    with pytest.raises(TypeError):
        K.sam_sqnorm(b["p"], b["g"], table, partials[:2], True)


# ------------------------------------------------------------------------------------------------ the module
def _arena_state(model, opt=None):
    A = model._icka_arena
    out = {"p": A.flat.clone(), "g": A.gflat.clone()}
    for lo, hi in A._cast_ranges:                  # (embedding tables outside these ranges have no shadow to speak of)
        out["bf16 %d" % lo] = A.shadow[lo:hi].clone()
        if A.shadow16 is not None:
            out["f16 %d" % lo] = A.shadow16[lo:hi].clone()
    if opt is not None and opt._m is not None:
        out["m"], out["v"] = opt._m.clone(), opt._v.clone()
    return out


def _assert_bitwise(a, b, what, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@pytest.mark.parametrize("adaptive,rho", [(False, 0.05), (True, 1.0)], ids=["plain", "adaptive"])
def test_run_equals_the_hand_run_launches_and_a_twin_at_the_perturbed_weights(adaptive, rho, capturable):
    import icka_amd
    from icka_amd import kernels as K
    from icka_amd.optim import ArenaAdamW
    (m1, m2, m3), args, labels = _twins(3)
    if adaptive:                                   # the mixed16 mode: both shadows
        for m in (m1, m2, m3):
            m._icka_arena.enable_fp16_shadow()
            m(*args, labels=labels).backward()
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, capturable=capturable)
    o1, o2 = ArenaAdamW(m1, **kw), ArenaAdamW(m2, **kw)
    sam = icka_amd.SAM(m1, o1, rho=rho, adaptive=adaptive)
    A1, A2, A3 = m1._icka_arena, m2._icka_arena, m3._icka_arena
    # -- a snapshot inside perturbed(), from the clean gradient of this batch
    for m in (m1, m2, m3):
        m.zero_grad()
    m1(*args, labels=labels).backward()
    clean = _arena_state(m1)
    with sam.perturbed() as inside:
        assert inside is sam and o1._perturbed
        snap = {"p": A1.flat.clone(), "bf16": A1.shadow.clone(), "f16": None if A1.shadow16 is None else A1.shadow16.clone()}
    assert not o1._perturbed and not torch.equal(snap["p"], clean["p"]), "the weights were somewhere else in between"
    _assert_bitwise(clean, _arena_state(m1), "perturbed() leaves weights, shadows and gradients as they were")
    m1.zero_grad()
    before = _arena_state(m1)
    # -- run
    loss1 = sam.run(lambda: m1(*args, labels=labels))
    assert (sam.ascents(), sam.skipped_ascents()) == (2, 0) and not o1._perturbed
    after = _arena_state(m1)
    _assert_bitwise(before, after, "weights and shadows after run()", skip=("g",))
    assert not torch.equal(after["g"], clean["g"]), "the gradient after run() is not the clean one"
    # -- the same launches by hand on the first twin
    loss2 = m2(*args, labels=labels)
    loss2.backward()
    assert torch.equal(A2.gflat, clean["g"])
    o2._bind()
    o2._build(A2)
    table, state, backup = o2._norm_table, K.sam_state_new("cuda"), torch.zeros_like(A2.flat)
    assert not A2.pending_wgrad and not A2.pending_reductions
    K.sam_sqnorm(A2.flat, A2.gflat, table, o2._partials, adaptive)
    K.sam_prepare(o2._partials, table.shape[0], rho, state)
    K.sam_ascend(A2.flat, A2.gflat, backup, A2.shadow, A2.shadow16, table, state, adaptive)
    assert torch.equal(A2.flat, snap["p"]), "the hand-run ascent reaches the weights of the snapshot"
    for s in A2.order:
        s.live = False
    m2(*args, labels=labels).backward()
    K.sam_restore(A2.flat, backup, A2.shadow, A2.shadow16, table, state)
    assert torch.equal(loss1, loss2), "run() returns the clean loss"
    _assert_bitwise(after, _arena_state(m2), "run() vs the hand-run launches")
    assert torch.equal(sam.grad_norm(), state[0:4].view(torch.float32)[0]) and sam.grad_norm().item() > 0
    # -- the gradient a twin computes at the perturbed weights, from zeroed gradients
    A3.flat.copy_(snap["p"])
    A3.shadow.copy_(snap["bf16"])
    if A3.shadow16 is not None:
        A3.shadow16.copy_(snap["f16"])
    A3.gflat.zero_()
    m3(*args, labels=labels).backward()
    assert torch.equal(A3.gflat, after["g"]), "the gradient after run() is the gradient at w + e, and of the second pass alone"
    # -- the update behind it
    o1.step()
    o2.step()
    _assert_bitwise(_arena_state(m1, o1), _arena_state(m2, o2), "after optimizer.step()")
    assert not torch.equal(A1.flat, after["p"]) and o1.steps_taken() == 1


def _batches(n):
    from icka_amd import synth
    names = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")
    return [tuple(synth.synthetic_batch(4, 32, 36, vocab_size=512, seed=300 + i)[k].cuda() for k in names) for i in range(n)]


def _step_fn(model, sam):
    def step_fn(*batch):
        return sam.run(lambda: model(*batch[:-1], labels=batch[-1]))
    return step_fn


@pytest.mark.parametrize("adaptive,rho", [(False, 0.05), (True, 1.0)], ids=["plain", "adaptive"])
def test_train_step_captures_the_whole_sam_step_in_one_graph(adaptive, rho):
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    base, _, _ = _model()
    mg, me = copy.deepcopy(base), copy.deepcopy(base)
    kw = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, capturable=True)
    batches = _batches(3)
    og, oe = ArenaAdamW(mg, **kw), ArenaAdamW(me, **kw)
    sg, se = icka_amd.SAM(mg, og, rho=rho, adaptive=adaptive), icka_amd.SAM(me, oe, rho=rho, adaptive=adaptive)
    # one eager SAM step first: moments, t and the counters are not trivial when the graph is built
    for m, o, s in ((mg, og, sg), (me, oe, se)):
        m.zero_grad()
        s.run(lambda: m(*batches[0][:-1], labels=batches[0][-1]))
        o.step()
        m.zero_grad()
    _assert_bitwise(_arena_state(mg, og), _arena_state(me, oe), "the two models before the graph is built")
    before = _arena_state(mg, og)
    ts = icka_amd.TrainStep(mg, _step_fn(mg, sg), og, inputs=batches[0])
    assert ts.captures == 1 and ts.stats["captures"] == 1, "clean pass, ascent, second pass, restore and update: ONE graph"
    _assert_bitwise(before, _arena_state(mg, og), "construction leaves weights, shadows and moments as they were", skip=("g",))
    assert (og.steps_taken(), og.skipped_steps(), sg.ascents(), sg.skipped_ascents()) == (1, 0, 1, 0)
    step_e = _step_fn(me, se)
    for i, b in enumerate(batches):
        lg = ts(*b).clone()
        me.zero_grad()
        le = step_e(*b)
        oe.step()
        assert torch.equal(lg, le), "loss of step %d" % i
        _assert_bitwise(_arena_state(mg, og), _arena_state(me, oe), "replayed vs eager, step %d" % i)
    assert ts.stats == {"captures": 1, "replays": 3, "eager": 0}
    assert (og.steps_taken(), sg.ascents(), sg.skipped_ascents()) == (4, 4, 0) == (oe.steps_taken(), se.ascents(), se.skipped_ascents())
    assert not torch.equal(before["p"], mg._icka_arena.flat)
    ts.close()


def test_refusals_on_the_device():
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    (model,), args, labels = _twins(1)
    A = model._icka_arena
    opt = ArenaAdamW(model, lr=1e-2, capturable=True, average="ema")
    sam = icka_amd.SAM(model, opt)
    closure = lambda: model(*args, labels=labels)       # noqa: E731
    # a live gradient slot (_twins left the gradient of one backward attached)
    with pytest.raises(RuntimeError, match="already live"):
        sam.run(closure)
    before = _arena_state(model)
    # accumulation under TrainStep
    with pytest.raises(NotImplementedError, match="accumulate=1"):
        icka_amd.TrainStep(model, lambda *b: sam.run(closure), opt, inputs=args, accumulate=2)
    # step() and averaged_weights() inside perturbed(); the context restores after the exception
    with pytest.raises(RuntimeError, match="perturbation is in place"):
        with sam.perturbed():
            assert not torch.equal(A.flat, before["p"])
            opt.step()
    _assert_bitwise(before, _arena_state(model), "after the refused step()")
    assert not opt._perturbed and opt.steps_taken() == 0
    with pytest.raises(RuntimeError, match="perturbation is in place"):
        with sam.perturbed():
            with opt.averaged_weights():
                pass
    _assert_bitwise(before, _arena_state(model), "after the refused averaged_weights()")
    with pytest.raises(RuntimeError, match="already in place"):
        with sam.perturbed():
            sam.ascend()
    _assert_bitwise(before, _arena_state(model), "after the refused second ascent")
    # run() inside averaged_weights()
    model.zero_grad()
    with opt.averaged_weights():
        with pytest.raises(RuntimeError, match="averaged weights"):
            sam.run(closure)
    _assert_bitwise(before, _arena_state(model), "after the refused run()", skip=("g",))
    # a GradReducer that arrives after construction is refused at the ascent
    A.reducer = object()
    try:
        with pytest.raises(NotImplementedError, match="GradReducer"):
            sam.run(closure)
    finally:
        A.reducer = None
    # queued weight-gradient launches in front of the norm
    model.zero_grad()
    closure().backward()
    A.pending_wgrad.append(None)
    try:
        with pytest.raises(AssertionError, match="still queued"):
            sam.ascend()
    finally:
        A.pending_wgrad.clear()
    assert sam.ascents() == 3 and sam.skipped_ascents() == 0


def test_a_non_finite_gradient_skips_the_ascent_and_restore_leaves_everything():
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    (model,), args, labels = _twins(1)
    A = model._icka_arena
    opt = ArenaAdamW(model, lr=1e-2)
    sam = icka_amd.SAM(model, opt)
    A.gflat.fill_(float("inf"))
    before = _arena_state(model)
    sam.ascend()
    assert opt._perturbed
    _assert_bitwise(before, _arena_state(model), "after the skipped ascent")
    assert bool((sam._backup == 0).all()), "the backup was never written"
    sam.restore()
    assert not opt._perturbed
    _assert_bitwise(before, _arena_state(model), "after the restore behind it")
    assert (sam.ascents(), sam.skipped_ascents()) == (0, 1) and not np.isfinite(sam.grad_norm().item())
    sam.restore()                                   # nothing in place: nothing happens
    _assert_bitwise(before, _arena_state(model), "after a restore without a perturbation")
