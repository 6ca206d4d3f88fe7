"""GPU: the averaged weights of ArenaAdamW(average="ema" | "swa") -- icka_optim_average, icka_optim_average_prepare /
icka_optim_average_dev and icka_optim_swap on flat buffers, element by element against the float64 oracle of
tests/optim_average_oracle.py, and the optimizer, TrainStep and averaged_weights() on the two-layer model of
tests/test_optim_capturable_gpu.py.

The bar per element is the oracle's: sum over the averaged updates of 4 * 2^-24 * (|p_k| + |avg_{k-1}|) (four f32 roundings
per update -- 1 - d, p - avg, the product, the sum -- each on a value no larger than |p| + |avg|; an f32 NumPy restatement at
N(0,1) * {1e-3, 1, 30} values reached 0.5 of it).  Everything that compares two runs of the same kernels on the same data, a
copy, a swap or an untouched element is bitwise."""
import copy

import numpy as np
import pytest
import torch

import optim_average_oracle as AO
from test_optim_capturable_gpu import _grad_sets, _model, _twins

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ flat buffers
CH = 8192
CHUNKS = [(64, 8), (128, 8184), (8448, CH), (20000, CH), (40944, 8)]      # (first element, count): ragged, not adjacent
TOTAL = 40960
UPDATES = 12


def _mask():
    m = torch.zeros(TOTAL, dtype=torch.bool, device="cuda")
    for lo, n in CHUNKS:
        m[lo:lo + n] = True
    return m


def _table():
    return torch.tensor(CHUNKS, dtype=torch.int64, device="cuda")


def _snapshots(seed=11):
    """UPDATES parameter buffers: N(0,1) * {1e-3, 1, 30} by element, drifting by a tenth of that per update."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.tensor([1e-3, 1.0, 30.0], device="cuda")[torch.arange(TOTAL, device="cuda") % 3]
    p = scale * torch.randn(TOTAL, generator=gen, device="cuda")
    out = []
    for _ in range(UPDATES):
        p = p + 0.1 * scale * torch.randn(TOTAL, generator=gen, device="cuda")
        out.append(p.clone())
    return out


def _f64(t):
    return t.detach().double().cpu().numpy()


def _blocks(kind, decay, warmup, start=0, every=1, n=0):
    from icka_amd import _lib, kernels as K
    av, st = K.average_state_new("cuda"), K.optim_state_new("cuda")
    h = _lib.AverageState()
    h.n, h.kind, h.warmup, h.decay, h.start, h.every = n, (_lib.AVERAGE_SWA if kind == "swa" else _lib.AVERAGE_EMA), int(warmup), \
        decay, start, every
    K.average_state_write(av, h, 0, av.numel())
    return av, st


def _set_optim(st, t, skip):
    from icka_amd import _lib, kernels as K
    h = _lib.OptimState()
    h.t, h.skip = t, skip
    K.optim_state_write(st, h, 0, _lib.OptimState.HOST_LO)


MODES = [("swa", 0.0, False), ("ema", 0.999, True), ("ema", 0.9, False)]


@pytest.mark.parametrize("kind,decay,warmup", MODES, ids=["swa", "ema-warmup", "ema-plain"])
def test_average_launches_on_flat_buffers_against_float64(kind, decay, warmup):
    from icka_amd import kernels as K
    from icka_amd.optim import average_decay_at
    mask, table, snaps = _mask(), _table(), _snapshots()
    snaps64 = [_f64(s) for s in snaps]
    avg_h = torch.full((TOTAL,), 777.0, device="cuda")          # host mode; the sentinel also stands where the table will write
    avg_d = avg_h.clone()                                       # capturable mode
    av, st = _blocks(kind, decay, warmup)
    worst = 0.0
    for k, p in enumerate(snaps):
        before = p.clone()
        K.optim_average(p, avg_h, table, average_decay_at(kind, decay, warmup, k))
        _set_optim(st, k + 1, 0)
        K.optim_average_prepare(av, st)
        K.optim_average_dev(p, avg_d, table, av)
        got = K.average_state_read(av)
        assert (got.n, got.apply) == (k + 1, 1)
        assert got.decay_now == np.float32(AO.decay_at(kind, decay, warmup, k)), k
        assert torch.equal(p, before), "the parameters are only read"
        if k == 0:
            assert torch.equal(avg_h[mask], p[mask]) and torch.equal(avg_d[mask], p[mask]), "decay 0: a bitwise copy"
        ref, n, bound, _ = AO.run(kind, decay, warmup, 0, 1, snaps64[:k + 1])
        assert n == k + 1
        for name, a in (("icka_optim_average", avg_h), ("icka_optim_average_dev", avg_d)):
            err = np.abs(_f64(a) - ref)[mask.cpu().numpy()]
            bd = bound[mask.cpu().numpy()]
            assert (err <= bd).all(), (name, k, float((err / bd).max()))
            worst = max(worst, float((err / np.maximum(bd, 1e-300)).max()))
            assert bool((a[~mask] == 777.0).all()), "%s wrote outside its table (update %d)" % (name, k)
        assert torch.equal(avg_h, avg_d), "one kernel serves both forms"
    print("\n[%s decay %g warmup %s, %d updates] worst error / bound = %.3f" % (kind, decay, warmup, UPDATES, worst))


def test_decay_zero_copies_and_nothing_applies_when_told_not_to():
    from icka_amd import kernels as K
    mask, table = _mask(), _table()
    p, q = _snapshots(5)[:2]
    avg = torch.full((TOTAL,), 777.0, device="cuda")
    K.optim_average(p, avg, table, 0.0)
    assert torch.equal(avg[mask], p[mask]) and bool((avg[~mask] == 777.0).all())
    # apply == 0 (not yet started; between two averaged updates) and skip == 1: nothing is touched, n stays
    av, st = _blocks("ema", 0.5, False, start=2, every=2, n=3)
    before = avg.clone()
    for t, skip, want in ((2, 0, 0), (4, 0, 0), (3, 1, 0), (5, 1, 0)):
        _set_optim(st, t, skip)
        K.optim_average_prepare(av, st)
        K.optim_average_dev(q, avg, table, av)
        got = K.average_state_read(av)
        assert (got.n, got.apply) == (3, want), (t, skip)
        assert torch.equal(avg, before), (t, skip)
    _set_optim(st, 5, 0)                     # update 5 of start 2, every 2 is averaged: (5 - 2 - 1) % 2 == 0
    K.optim_average_prepare(av, st)
    K.optim_average_dev(q, avg, table, av)
    got = K.average_state_read(av)
    assert (got.n, got.apply, got.decay_now) == (4, 1, 0.5)
    assert not torch.equal(avg[mask], before[mask]) and bool((avg[~mask] == 777.0).all())
    # operand checks of the wrappers
    with pytest.raises(ValueError):
        K.optim_average(p, avg, table, 1.0)
    with pytest.raises(ValueError):
        K.optim_average(p, p, table, 0.5)
    with pytest.raises(TypeError):
        K.optim_average(p, avg[:-8], table, 0.5)
    with pytest.raises(TypeError):
        K.optim_average(p, avg, table.to(torch.int32), 0.5)
    with pytest.raises(TypeError):
        K.optim_swap(p, avg, torch.zeros(TOTAL, device="cuda"), None, table)
    with pytest.raises(TypeError):
        K.optim_average_dev(p, avg, table, st)               # the optimizer's block is not an average block


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16-shadow", "bf16+fp16-shadows"])
def test_swap_on_flat_buffers(fp16):
    from icka_amd import kernels as K
    mask, table = _mask(), _table()
    p0, a0 = _snapshots(7)[:2]
    p0[130], a0[131], a0[8450] = 7e4, -7e4, 1e-41            # beyond the fp16 range on both sides; an f32 denormal
    sh0 = torch.where(mask, p0.to(torch.bfloat16), torch.full_like(p0, 7.0, dtype=torch.bfloat16))
    sh16_0 = torch.where(mask, p0.clamp(-65504.0, 65504.0).to(torch.float16), torch.full_like(p0, 7.0, dtype=torch.float16)) \
        if fp16 else None
    p, a, sh, sh16 = p0.clone(), a0.clone(), sh0.clone(), (sh16_0.clone() if fp16 else None)
    K.optim_swap(p, a, sh, sh16, table)
    np_, na = AO.swap(p0.cpu().numpy(), a0.cpu().numpy())
    m = mask.cpu().numpy()
    assert np.array_equal(p.cpu().numpy()[m].view(np.uint32), np_[m].view(np.uint32)), "params <- avg, bitwise"
    assert np.array_equal(a.cpu().numpy()[m].view(np.uint32), na[m].view(np.uint32)), "avg <- params, bitwise"
    assert torch.equal(p[~mask], p0[~mask]) and torch.equal(a[~mask], a0[~mask]), "the gaps are untouched"
    assert torch.equal(sh[mask], p[mask].to(torch.bfloat16)) and bool((sh[~mask] == 7.0).all())
    if fp16:
        assert torch.equal(sh16[mask], p[mask].clamp(-65504.0, 65504.0).to(torch.float16)) and bool((sh16[~mask] == 7.0).all())
        assert sh16[131].item() == -65504.0
    K.optim_swap(p, a, sh, sh16, table)
    assert torch.equal(p, p0) and torch.equal(a, a0) and torch.equal(sh, sh0), "a second swap restores everything"
    if fp16:
        assert torch.equal(sh16, sh16_0)


# ------------------------------------------------------------------------------------------------ the optimizer
def _avg_of(opt):
    return opt._avg.clone()


def _check_against_oracle(opt, A, snaps, kind, decay, warmup, start=0, every=1, applied=None, what=""):
    ref, n, bound, used = AO.run(kind, decay, warmup, start, every, [_f64(s) for s in snaps], avg0=None, applied=applied)
    table = np.zeros(A.total, dtype=bool)
    for g in opt.param_groups:
        for p in g["params"]:
            s = A.slots[id(p)]
            table[s.off:s.off + s.numel] = True
    err = np.abs(_f64(opt._avg) - ref)[table]
    assert (err <= bound[table]).all(), (what, float((err / np.maximum(bound[table], 1e-300)).max()))
    return ref, n, bound, used


def test_host_mode_swa_is_the_mean_of_the_snapshots():
    from icka_amd.optim import ArenaAdamW
    (model,), _, _ = _twins(1)
    A = model._icka_arena
    opt = ArenaAdamW(model, lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, average="swa")
    snaps = []
    for g in _grad_sets(A, 6):
        A.gflat.copy_(g)
        opt.step()
        snaps.append(A.flat.clone())
    assert opt.average_count() == 6 and not torch.equal(snaps[0], snaps[5])
    _, _, bound, _ = _check_against_oracle(opt, A, snaps, "swa", 0.0, False, what="swa")
    mean = np.mean([_f64(s) for s in snaps], axis=0)
    sd, msd = opt.averaged_state_dict(), model.state_dict()
    assert list(sd) == list(msd)
    for name, p in model.named_parameters():
        s = A.slots[id(p)]
        err = np.abs(_f64(sd[name]).reshape(-1) - mean[s.off:s.off + s.numel])
        assert (err <= bound[s.off:s.off + s.numel] + 1e-12 * np.abs(mean[s.off:s.off + s.numel])).all(), name
    for name in msd:
        if name not in dict(model.named_parameters()):
            assert torch.equal(sd[name], msd[name]), "buffers pass through: %s" % name
    assert torch.equal(A.flat, snaps[-1]), "averaged_state_dict() does not swap"


def test_host_mode_start_and_every_select_the_updates_the_oracle_names():
    from icka_amd.optim import ArenaAdamW
    (model,), _, _ = _twins(1)
    A = model._icka_arena
    opt = ArenaAdamW(model, lr=1e-2, average="swa", average_start=2, average_every=2)
    snaps, counts = [], []
    for g in _grad_sets(A, 6):
        A.gflat.copy_(g)
        opt.step()
        snaps.append(A.flat.clone())
        counts.append(opt.average_count())
    _, n, _, used = _check_against_oracle(opt, A, snaps, "swa", 0.0, False, start=2, every=2, what="start 2 every 2")
    assert used == [3, 5] and n == 2 and counts == [0, 0, 1, 1, 2, 2]
    # a step() without any gradient returns early: update 7 would be averaged, but there is no update
    avg = _avg_of(opt)
    model.zero_grad()
    opt.step()
    assert opt.average_count() == 2 and opt.steps_taken() == 6 and torch.equal(opt._avg, avg)


def test_capturable_against_host_mode_with_a_refused_update_in_the_middle():
    from icka_amd.optim import ArenaAdamW
    (mc, mh), _, _ = _twins(2)
    Ac, Ah = mc._icka_arena, mh._icka_arena
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, average="ema", average_decay=0.999, average_warmup=True)
    oc, oh = ArenaAdamW(mc, capturable=True, **kw), ArenaAdamW(mh, **kw)
    grads = _grad_sets(Ac, 8)
    sc, sh = [], []
    for i, g in enumerate(grads):
        if i == 4:                               # a NaN gradient set in the middle, seen by the capturable optimizer only
            before, n_before = _avg_of(oc), oc.average_count()
            Ac.gflat.copy_(g)
            Ac.gflat[Ac.slots[id(mc.classifier.weight)].off + 3] = float("nan")
            oc.step()
            assert torch.equal(oc._avg, before), "a refused update is not averaged"
            assert oc.average_count() == n_before == 4 and oc.skipped_steps() == 1 and oc.steps_taken() == 4
        Ac.gflat.copy_(g)
        oc.step()
        sc.append(Ac.flat.clone())
        Ah.gflat.copy_(g)
        oh.step()
        sh.append(Ah.flat.clone())
    assert oc.average_count() == oh.average_count() == 8 and oc.skipped_steps() == 1
    rc, _, bc, _ = _check_against_oracle(oc, Ac, sc, "ema", 0.999, True, what="capturable")
    rh, _, bh, _ = _check_against_oracle(oh, Ah, sh, "ema", 0.999, True, what="host")
    # each is within the bar of the oracle of its own parameters, so the two agree within both bars plus what the oracles
    # differ by (the parameters of the two modes are separate compilations of the same expressions)
    gap = np.abs(_f64(oc._avg) - _f64(oh._avg))
    assert (gap <= bc + bh + np.abs(rc - rh)).all()
    print("\n[capturable vs host mode EMA, 8 updates] averages bitwise equal: %s" % torch.equal(oc._avg, oh._avg))


def _micro_of(model, k):
    def micro(ids, seg, mask, added, vmean, vatt, labels):
        loss = model(ids, seg, mask, added, vmean, vatt, labels=labels) / k
        loss.backward()
        return loss
    return micro


def _batches(n):
    from icka_amd import synth
    names = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att", "labels")
    return [tuple(synth.synthetic_batch(4, 32, 36, vocab_size=512, seed=200 + i)[k].cuda() for k in names) for i in range(n)]


def test_train_step_captures_the_average_with_the_update():
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    base, _, _ = _model()
    mg, me = copy.deepcopy(base), copy.deepcopy(base)
    kw = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, capturable=True, average="swa")
    batches = _batches(4)
    og = ArenaAdamW(mg, **kw)
    ts = icka_amd.TrainStep(mg, _micro_of(mg, 2), og, inputs=batches[0], accumulate=2)
    Ag = mg._icka_arena
    assert og.average_count() == 0 and og.steps_taken() == 0, "the dry warm-up launches count nothing"
    assert torch.equal(og._avg, Ag.flat), "right after construction the average is the parameters"
    sg = []
    for i, b in enumerate(batches):
        ts(*b)
        if i % 2 == 1:
            sg.append(Ag.flat.clone())
    assert ts.stats["replays"] == 4 and ts.stats["eager"] == 0
    assert og.average_count() == 2 and og.steps_taken() == 2
    rg, _, bg, _ = _check_against_oracle(og, Ag, sg, "swa", 0.0, False, what="TrainStep")
    # the same loop launched eagerly (eval mode: dropout off)
    oe = ArenaAdamW(me, **kw)
    micro = _micro_of(me, 2)
    se = []
    me.zero_grad()
    for i, b in enumerate(batches):
        micro(*b)
        if i % 2 == 1:
            oe.step()
            me.zero_grad()
            se.append(me._icka_arena.flat.clone())
    assert oe.average_count() == 2
    re_, _, be, _ = _check_against_oracle(oe, me._icka_arena, se, "swa", 0.0, False, what="eager loop")
    # an average is a convex combination of its snapshots: the two differ by no more than their bars plus what the oracles of
    # their own snapshots differ by
    gap = np.abs(_f64(og._avg) - _f64(oe._avg))
    assert (gap <= bg + be + np.abs(rg - re_)).all()
    assert float(np.abs(rg - re_).max()) <= 2e-4 * max(1.0, float(np.abs(re_).max())), "replayed and eager parameters (bf16 bar)"
    ts.close()


def _fresh_copy(m):
    c = copy.deepcopy(m)
    for mod in c.modules():
        object.__setattr__(mod, "_icka_arena", None)     # a fresh process would build its own arena on the first forward
    return c


@pytest.mark.parametrize("policy", ["tracked", "always"])
def test_averaged_weights_context(policy, monkeypatch):
    from icka_amd import kernels as K
    from icka_amd.graph import GraphedModule
    from icka_amd.optim import ArenaAdamW
    (model,), args, _ = _twins(1)
    A = model._icka_arena
    A.shadow_policy = policy
    if policy == "always":
        A.enable_fp16_shadow()
    opt = ArenaAdamW(model, lr=1e-2, average="ema", average_decay=0.5, average_warmup=False)
    for g in _grad_sets(A, 3):
        A.gflat.copy_(g)
        opt.step()
    with torch.no_grad():
        gm = GraphedModule(model, args)                      # the dev pass, captured on the trained weights
        trained = gm(*args).clone()
        assert torch.equal(model(*args), trained)
    twin = _fresh_copy(model)
    twin.load_state_dict(opt.averaged_state_dict())
    with torch.no_grad():
        want = twin(*args).clone()
    assert not torch.equal(want, trained), "the averaged weights are other weights"
    before = {"p": A.flat.clone(), "avg": opt._avg.clone(), "bf16": A.shadow.clone(),
              "f16": None if A.shadow16 is None else A.shadow16.clone()}
    casts = []
    for name in ("cast_f32_to_bf16", "cast_f32_to_bf16_f16"):
        monkeypatch.setattr(K, name, (lambda f: lambda *a, **k: (casts.append(1), f(*a, **k))[1])(getattr(K, name)))
    synced = A._synced
    with opt.averaged_weights() as inside:
        assert inside is opt
        assert torch.equal(A.flat, before["avg"]) and torch.equal(opt._avg, before["p"])
        swapped_shadow = A.shadow.clone()
        for lo, hi in A._cast_ranges:
            assert torch.equal(A.shadow[lo:hi], A.flat[lo:hi].to(torch.bfloat16))
            if A.shadow16 is not None:
                assert torch.equal(A.shadow16[lo:hi], A.flat[lo:hi].clamp(-65504.0, 65504.0).to(torch.float16))
        sd, asd = model.state_dict(), opt.averaged_state_dict()
        for name, _ in model.named_parameters():
            assert torch.equal(sd[name], asd[name]), name
        with torch.no_grad():
            assert torch.equal(model(*args), want), "eager forward inside the context"
            assert torch.equal(gm(*args), want), "a capture made before the context, replayed inside it"
        assert torch.equal(A.shadow, swapped_shadow), "a re-cast reproduces the bits the swap wrote"
        with pytest.raises(RuntimeError, match="already active"):
            with opt.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
        assert torch.equal(A.flat, before["avg"]), "the refusals touched nothing"
    with torch.no_grad():
        assert torch.equal(gm(*args), trained) and torch.equal(model(*args), trained)
    assert torch.equal(A.flat, before["p"]) and torch.equal(opt._avg, before["avg"])
    for lo, hi in A._cast_ranges:                            # (embedding tables outside these ranges have no shadow to speak of)
        assert torch.equal(A.shadow[lo:hi], before["bf16"][lo:hi])
        if before["f16"] is not None:
            assert torch.equal(A.shadow16[lo:hi], before["f16"][lo:hi])
    if policy == "tracked":
        assert casts == [] and A._synced == synced, "neither entry nor exit re-casts under the tracked policy"
    else:
        assert casts, "the 'always' policy re-cast (and reproduced the same bits)"
    # an exception inside the context still swaps back
    with pytest.raises(ZeroDivisionError):
        with opt.averaged_weights():
            1 / 0
    assert torch.equal(A.flat, before["p"]) and torch.equal(opt._avg, before["avg"]) and not opt._swapped
    A.attach_grads()                                         # (the capture's construction dropped p.grad)
    A.gflat.copy_(_grad_sets(A, 1)[0])
    opt.step()                                               # and the optimizer steps again
    assert opt.average_count() == 4 and not torch.equal(A.flat, before["p"])
    gm.close()


def test_train_step_refuses_while_the_average_is_swapped_in():
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    model, _, _ = _model()
    b = _batches(1)[0]
    opt = ArenaAdamW(model, lr=1e-2, capturable=True, average="ema")
    ts = icka_amd.TrainStep(model, _micro_of(model, 1), opt, inputs=b, warmup=1)
    ts(*b)
    assert opt.average_count() == 1
    p = model._icka_arena.flat.clone()
    with opt.averaged_weights():
        with pytest.raises(RuntimeError, match="swapped in"):
            ts(*b)
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
    assert opt.average_count() == 1 and opt.steps_taken() == 1 and ts.stats["replays"] == 1
    assert torch.equal(model._icka_arena.flat, p)
    ts(*b)
    assert opt.average_count() == 2
    ts.close()


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
def test_state_dict_round_trip_continues_the_average_bitwise(capturable):
    from icka_amd.optim import ArenaAdamW
    (full_model, half_model), args, labels = _twins(2)
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, capturable=capturable, average="ema", average_decay=0.9,
              average_start=1)
    grads = _grad_sets(full_model._icka_arena, 6)

    def run(m, opt, gs):
        # every p.grad a view of the arena's gradient buffer, so that the sets installed here are the gradients of every
        # parameter in all three models (step() copies a gradient held in a tensor of its own over its slot)
        m._icka_arena.attach_grads()
        for g in gs:
            m._icka_arena.gflat.copy_(g)
            opt.step()

    full = ArenaAdamW(full_model, **kw)
    run(full_model, full, grads)
    first = ArenaAdamW(half_model, **kw)
    run(half_model, first, grads[:3])
    sd = first.state_dict()
    assert sd["icka_avg_n"] == 2 and sd["icka_t"] == 3 and sd["icka_avg"].shape == (half_model._icka_arena.total,)
    resumed_model = _fresh_copy(half_model)
    resumed_model(*args, labels=labels).backward()           # builds the arena and attaches the gradients
    second = ArenaAdamW(resumed_model, **kw)
    second.load_state_dict(sd)                               # before the arena is bound: installed at the first step
    assert second.average_count() == 2
    run(resumed_model, second, grads[3:])
    A, B = full_model._icka_arena, resumed_model._icka_arena
    assert [(s.name, s.off, s.numel) for s in A.order] == [(s.name, s.off, s.numel) for s in B.order]
    # element by element over the parameters: the alignment padding behind a slot is no parameter (these gradient sets carry
    # noise there too, the update kernels walk whole 8-element groups, and a model built anew starts its padding at zero)
    real = torch.zeros(A.total, dtype=torch.bool, device="cuda")
    for s in A.order:
        real[s.off:s.off + s.numel] = True
    for what, a, b in (("parameters", A.flat, B.flat), ("exp_avg", full._m, second._m), ("exp_avg_sq", full._v, second._v),
                       ("average", full._avg, second._avg)):
        assert torch.equal(a[real], b[real]), what
    assert second.average_count() == full.average_count() == 5 and second.steps_taken() == 6
    # after the arena is bound: installed at once; another layout is refused before anything is copied
    second.load_state_dict(sd)
    assert second.average_count() == 2 and torch.equal(second._avg.cpu(), sd["icka_avg"])
    bad = dict(sd)
    bad["icka_layout"] = [("x", 0, 8)]
    with pytest.raises(ValueError, match="another parameter layout"):
        second.load_state_dict(bad)
    # a state without an average restarts it from the parameters
    plain = {k: v for k, v in sd.items() if k not in ("icka_avg", "icka_avg_n")}
    second.load_state_dict(plain)
    assert second.average_count() == 0 and torch.equal(second._avg, B.flat)
