"""GPU: the constrained CRF (icka_crf_constrained_llh / _grad / _decode, CRF.constrained_llh / constrained_decode) against the
float64 oracle of tests/crf_constrained_oracle.py.

Bars (those of tests/test_crf_gpu.py, doubled where a result is the difference of two such quantities):
  log_z, log_za     rtol 2e-5, atol 2e-4 each;  llh = log_za - log_z: the sum of the two bars
  d_emissions       2e-3 absolute
  parameter grads   1e-3 (max|G_A| + max|G|) + 4e-5 with G_A, G the oracle's restricted and free expected counts: the difference
                    can cancel, so the bar scales with the two terms
Decoding on grids (multiples of 1/8: every f32 sum exact) is compared bit for bit; on ordinary inputs within
``crf_check.viterbi_tol``."""
import functools
import math

import pytest
import torch

import crf_check as cc
import crf_constrained_oracle as CO
import kernel_check as kc

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
SHAPES = [(4, 6, 3), (5, 37, 13), (3, 70, 17), (2, 9, 64)]      # enumeration size | C <= 16 | C > 16, two mask words | bit 63
BIG = (32, 128, 13)
MASKS = ["none", "prefix", "holes", "first_off"]
KINDS = ["random", "partial", "all", "single"]


def _crf(C, params, batch_first=True):
    from icka_amd.crf import CRF
    crf = CRF(C, batch_first=batch_first).cuda()
    with torch.no_grad():
        for p, v in zip((crf.start_transitions, crf.end_transitions, crf.transitions), params):
            p.copy_(v)
    return crf


def _cu(t):
    return None if t is None else t.cuda()


@functools.lru_cache(maxsize=None)
def _case(B, S, C, mask_kind, kind, grid=None, empty_at=None):
    """(e, mask, allowed, (start, end, trans), [oracle Sample]) -- computed once, shared, never modified.  ``empty_at``: that
    sample gets an empty set at its LAST on-position (at C < 64 a word whose only bit is bit C, which is ignored)."""
    seed = B * 1000 + S * 10 + C + 7 * MASKS.index(mask_kind) + 100 * KINDS.index(kind)
    e, st, en, tr = CO.inputs(B, S, C, seed, grid=grid)
    mask = CO.make_mask(mask_kind, B, S, seed + 1)
    allowed = CO.allowed_sets(kind, B, S, C, seed + 2)
    if empty_at is not None:
        last = S - 1 if mask is None else max([0] + [t for t in range(1, S) if mask[empty_at, t]])
        allowed[empty_at, last] = 0 if C == 64 else (1 << C)
    return e, mask, allowed, (st, en, tr), CO.batch(e, mask, allowed, st, en, tr)


def _bar_lz(ref):
    return 2e-4 + 2e-5 * abs(ref)


def _run_llh(e, mask, allowed, P):
    """the launcher -> (llh, log_z, log_za, infeasible count) on the host"""
    from icka_amd import kernels as K
    B = e.shape[0]
    out = torch.empty(3, B, dtype=F32, device="cuda")
    cnt = torch.zeros(1, dtype=I32, device="cuda")
    K.crf_constrained_llh(e.cuda(), _cu(mask), allowed.cuda(), *[p.cuda() for p in P], out[0], out[1], out[2], cnt)
    return out[0].cpu().double(), out[1].cpu().double(), out[2].cpu().double(), int(cnt.item())


def _check_values(llh, log_z, log_za, samples, what):
    for b, s in enumerate(samples):
        print("%s sample %d: log_z %.6f (ref %.6f) log_za %.6f (ref %.6f) llh %.6f (ref %.6f)"
              % (what, b, log_z[b], s.log_z, log_za[b], s.log_za, llh[b], s.llh))
        assert abs(float(log_z[b]) - s.log_z) <= _bar_lz(s.log_z), (what, b)
        if not s.feasible:
            assert float(llh[b]) == -math.inf and float(log_za[b]) == -math.inf, (what, b)
            continue
        assert abs(float(log_za[b]) - s.log_za) <= _bar_lz(s.log_za), (what, b)
        assert abs(float(llh[b]) - s.llh) <= _bar_lz(s.log_z) + _bar_lz(s.log_za), (what, b)
        assert float(llh[b]) <= _bar_lz(s.log_z) + _bar_lz(s.log_za), (what, b)


def _check_grads(de, pgrads, samples, w, what):
    """d_emissions [B,S,C] and the three parameter gradients of sum_b w_b llh_b against the oracle"""
    ref = torch.stack([float(w[b]) * s.d_e for b, s in enumerate(samples)])
    err = (de.cpu().double() - ref).abs().max().item()
    print("%s: d_emissions max err %.3e (bar 2e-3)" % (what, err))
    assert err < 2e-3, (what, err)
    ga, gf = CO.param_grads(samples, w)
    for name, mine, a, f in zip(("start", "end", "trans"), pgrads, ga, gf):
        bar = 1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5
        err = (mine.cpu().double() - (a - f)).abs().max().item()
        print("%s: d_%s max err %.3e (bar %.3e)" % (what, name, err, bar))
        assert err < bar, (what, name, err, bar)


def _llh_and_grads(crf, e, mask, allowed, w, batch_first=True):
    eg = e.cuda().requires_grad_(True)
    out = crf.constrained_llh(eg, allowed.cuda(), mask=_cu(mask), reduction="none")
    crf.zero_grad(set_to_none=True)
    (out * w.cuda()).sum().backward()
    return out.detach(), eg.grad, [p.grad.clone() for p in (crf.start_transitions, crf.end_transitions, crf.transitions)]


# ------------------------------------------------------------------------------------------------ 1. the oracle
def _against_oracle(B, S, C, mask_kind, kind):
    e, mask, allowed, P, samples = _case(B, S, C, mask_kind, kind)
    what = "[%d,%d,%d] %s %s" % (B, S, C, mask_kind, kind)
    llh, log_z, log_za, n_inf = _run_llh(e, mask, allowed, P)
    assert n_inf == 0
    _check_values(llh, log_z, log_za, samples, what)
    if B == 4 and S == 6:      # the enumeration size: the oracle itself against all C^L paths
        for b, s in enumerate(samples):
            ref = CO.enumerate_sample(e[b].double(), None if mask is None else mask[b], allowed[b], *[p.double() for p in P])
            assert abs(s.log_za - ref["log_za"]) < 1e-9 and abs(s.log_z - ref["log_z"]) < 1e-9
            assert torch.allclose(s.marg_a, ref["marg_a"], atol=1e-12) and torch.allclose(s.pair_a, ref["pair_a"], atol=1e-12)
    crf = _crf(C, P)
    w = torch.linspace(0.5, 1.5, B)
    out, de, pg = _llh_and_grads(crf, e, mask, allowed, w)
    assert torch.equal(out.cpu().double(), llh)          # the module's value is the launcher's
    assert not torch.isnan(de).any()
    _check_grads(de, pg, samples, w, what)
    if mask is not None:                                 # off-positions: exact +0.0 in every column
        off = (mask == 0)
        off[:, 0] = False
        rows = de.cpu()[off]
        assert torch.equal(rows.view(I32), torch.zeros_like(rows).view(I32))
    if kind == "all":                                    # 3. nothing is constrained: 0 within the bars
        for b, s in enumerate(samples):
            assert abs(float(llh[b])) <= _bar_lz(s.log_z) + _bar_lz(s.log_za)
        assert de.abs().max().item() < 2e-3
        ga, gf = CO.param_grads(samples, w)
        for mine, a, f in zip(pg, ga, gf):
            assert mine.abs().max().item() < 1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_llh_and_gradients_against_the_oracle(B, S, C, mask_kind, kind):
    _against_oracle(B, S, C, mask_kind, kind)


def test_llh_and_gradients_against_the_oracle_at_the_benchmark_shape():
    _against_oracle(*BIG, "prefix", "partial")


# --------------------------------------------------------------------------------------------- 2. singletons
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_singletons_of_a_path_give_the_gold_path_likelihood(B, S, C):
    e, mask, allowed, P, samples = _case(B, S, C, "prefix", "single")
    tags = torch.tensor([[CO.tag_set(allowed[b, t], C)[0] for t in range(S)] for b in range(B)])
    w = torch.linspace(0.5, 1.5, B)
    crf = _crf(C, P)
    out, de, pg = _llh_and_grads(crf, e, mask, allowed, w)
    gold = _crf(C, P)
    eg = e.cuda().requires_grad_(True)
    ref = gold(eg, tags.cuda(), mask=mask.cuda(), reduction="none")
    (ref * w.cuda()).sum().backward()
    for b, s in enumerate(samples):
        assert abs(float(out[b]) - float(ref[b].detach())) <= _bar_lz(s.log_z) + _bar_lz(s.log_za), (b, out[b], ref[b])
    assert (de - eg.grad).abs().max().item() < 2e-3
    ga, gf = CO.param_grads(samples, w)
    for mine, theirs, a, f in zip(pg, (gold.start_transitions, gold.end_transitions, gold.transitions), ga, gf):
        assert (mine - theirs.grad).abs().max().item() < 1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5


# --------------------------------------------------------------------------------------------- 4. infeasible
@pytest.mark.parametrize("mask_kind", ["none", "holes"])
@pytest.mark.parametrize("B,S,C", [(4, 6, 3), (5, 37, 13), (2, 9, 64)])
def test_an_infeasible_sample_is_reported_and_leaves_the_others_alone(B, S, C, mask_kind):
    bad = B - 1
    e, mask, allowed, P, samples = _case(B, S, C, mask_kind, "random", None, bad)
    assert not samples[bad].feasible and all(s.feasible for s in samples[:bad])
    llh, log_z, log_za, n_inf = _run_llh(e, mask, allowed, P)
    assert n_inf == 1
    assert float(llh[bad]) == -math.inf and float(log_za[bad]) == -math.inf and math.isfinite(float(log_z[bad]))
    _check_values(llh, log_z, log_za, samples, "infeasible")
    assert not (torch.isnan(llh).any() or torch.isnan(log_z).any() or torch.isnan(log_za).any())
    w = torch.linspace(0.5, 1.5, B)
    out, de, pg = _llh_and_grads(_crf(C, P), e, mask, allowed, w)
    assert torch.equal(de[bad].view(I32), torch.zeros_like(de[bad]).view(I32))          # exact zeros, every row
    assert not torch.isnan(de).any() and not any(torch.isnan(g).any() for g in pg) and not torch.isnan(out).any()
    _check_grads(de, pg, samples, w, "infeasible")
    # the same batch without that sample
    keep = [b for b in range(B) if b != bad]
    out2, de2, pg2 = _llh_and_grads(_crf(C, P), e[keep], None if mask is None else mask[keep], allowed[keep], w[keep])
    assert torch.equal(out[keep], out2) and torch.equal(de[keep], de2)
    ga, gf = CO.param_grads(samples, w)
    for g1, g2, a, f in zip(pg, pg2, ga, gf):
        assert (g1 - g2).abs().max().item() < 1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5


# ------------------------------------------------------------------------------------------------- 5., 6. decode
def _decode(crf, e, mask, allowed):
    out = crf.constrained_decode(e.cuda(), allowed.cuda(), mask=_cu(mask))
    return out, out.host()


@pytest.mark.parametrize("grid", ["coarse", "fine"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_decode_on_exact_grids(B, S, C, mask_kind, kind, grid):
    e, mask, allowed, P, samples = _case(B, S, C, mask_kind, kind, grid)
    crf = _crf(C, P)
    out, h = _decode(crf, e, mask, allowed)
    assert h["infeasible"] == 0 and h["lens"] == [s.L for s in samples]
    for b, s in enumerate(samples):
        path, score = s.viterbi()
        assert h["paths"][b] == path, (b, h["paths"][b], path)
        got, want = torch.tensor(h["scores"][b], dtype=F32), torch.tensor(score, dtype=torch.float64).to(F32)
        assert torch.equal(got.view(I32), want.view(I32)), (b, got, want)
        if kind == "single":
            assert path == [CO.tag_set(allowed[b, t], C)[0] for t in s.pos]
    if kind == "all" and mask_kind in ("none", "prefix"):
        assert h["paths"] == crf.decode(e.cuda(), mask=_cu(mask))
    if B == 4 and S == 6:
        for b in range(B):
            ref = CO.enumerate_sample(e[b].double(), None if mask is None else mask[b], allowed[b], *[p.double() for p in P])
            assert (h["paths"][b], h["scores"][b]) == ref["best"]


def test_decode_on_an_exact_grid_at_the_benchmark_shape():
    B, S, C = BIG
    e, mask, allowed, P, samples = _case(B, S, C, "prefix", "partial", "coarse")
    out, h = _decode(_crf(C, P), e, mask, allowed)
    assert h["lens"] == [s.L for s in samples] and h["infeasible"] == 0
    for b, s in enumerate(samples):
        path, score = s.viterbi()
        assert h["paths"][b] == path and h["scores"][b] == score, b


@pytest.mark.parametrize("kind", ["random", "partial"])
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_decode_on_ordinary_inputs(B, S, C, mask_kind, kind):
    bad = B - 1
    e, mask, allowed, P, samples = _case(B, S, C, mask_kind, kind, None, bad)
    out, h = _decode(_crf(C, P), e, mask, allowed)
    assert h["infeasible"] == 1 and h["lens"] == [s.L for s in samples]
    assert h["paths"][bad] is None and h["scores"][bad] == -math.inf and out.tolist()[bad] is None
    n = sum(h["lens"])
    flat = out.tags.tags_flat.cpu()[:n].tolist()
    assert flat[n - samples[bad].L:] == [-1] * samples[bad].L
    for b, s in enumerate(samples[:bad]):
        path = h["paths"][b]
        assert len(path) == s.L and all(path[i] in s.sets[i] for i in range(s.L)), b
        best, best_score = s.viterbi()
        x = e[b][s.pos]
        tol = cc.viterbi_tol(s.L, cc.path_terms(path, x, *P), cc.path_terms(best, x, *P))
        mine = s.score(path)
        print("sample %d: score %.6f, optimum %.6f, returned %.6f, tol %.3e" % (b, mine, best_score, h["scores"][b], tol))
        assert best_score - mine <= tol and mine <= best_score + 1e-9
        assert abs(h["scores"][b] - mine) <= tol


# ------------------------------------------------------------------------------------------------ 7. guard bands
def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("mask_kind", ["none", "holes"])
@pytest.mark.parametrize("B,S,C", [(4, 6, 3), (3, 70, 17), (2, 9, 64)])
def test_guard_bands_and_row_strides(B, S, C, mask_kind):
    """through the C ABI (the only way ld and ldd can differ from C): emissions at ld = C + 3 inside NaN bands, d_emissions at
    ldd = C + 5, every output inside sentinel bands; the results equal the contiguous launchers' bit for bit"""
    from icka_amd import _lib
    from icka_amd import kernels as K
    lib = _lib.load()
    bad = B - 1
    e, mask, allowed, P, samples = _case(B, S, C, mask_kind, "random", None, bad)
    st, en, tr = [p.cuda() for p in P]
    m, al = _cu(mask), allowed.cuda()
    ld, ldd = C + 3, C + 5
    eg = kc.guarded_input(e.reshape(B * S, C), ld=ld)
    s = torch.cuda.current_stream().cuda_stream
    # llh
    (llh, c1), (lz, c2), (lza, c3) = kc.guarded(1, B, F32), kc.guarded(1, B, F32), kc.guarded(1, B, F32)
    cnt, c4 = kc.guarded(1, 1, I32, init=0)
    assert lib.icka_crf_constrained_llh(_ptr(eg), ld, _ptr(m), _ptr(al), _ptr(st), _ptr(en), _ptr(tr), _ptr(llh), _ptr(lz),
                                        _ptr(lza), _ptr(cnt), B, S, C, s) == 0
    # grad
    w = torch.linspace(0.5, 1.5, B).cuda()
    de = kc.Guarded(B * S, C, F32, ld=ldd)
    (ds, c5), (dn, c6), (dt, c7) = kc.guarded(1, C, F32, init=0.0), kc.guarded(1, C, F32, init=0.0), kc.guarded(C, C, F32, init=0.0)
    assert lib.icka_crf_constrained_grad(_ptr(eg), ld, _ptr(m), _ptr(al), _ptr(st), _ptr(en), _ptr(tr), _ptr(w), _ptr(de.view),
                                         ldd, _ptr(ds), _ptr(dn), _ptr(dt), B, S, C, s) == 0
    # decode
    cap = B * S + 5
    (lens, c8), (flat, c9), (sc, c10) = kc.guarded(1, B, I32), kc.guarded(1, cap, I32), kc.guarded(1, B, F32)
    cnt2, c11 = kc.guarded(1, 1, I32, init=0)
    assert lib.icka_crf_constrained_decode(_ptr(eg), ld, _ptr(m), _ptr(al), _ptr(st), _ptr(en), _ptr(tr), _ptr(lens), _ptr(flat),
                                           cap, _ptr(sc), _ptr(cnt2), B, S, C, s) == 0
    torch.cuda.synchronize()
    for chk in (c1, c2, c3, c4, c5, c6, c7, c8, c9, c10, c11, de.check):
        chk()
    n = int(lens[0].sum())
    assert n == sum(x.L for x in samples) and int(cnt[0, 0]) == 1 and int(cnt2[0, 0]) == 1
    assert bool((flat[0, n:] == kc.SENTINEL[I32]).all()), "entries past sum(lens) were written"
    assert bool((flat[0, :n] != kc.SENTINEL[I32]).all())
    assert not torch.isnan(de.view).any() and not torch.isnan(dt).any() and not torch.isnan(llh).any()
    # the contiguous launchers
    ec = e.cuda()
    o = torch.empty(3, B, dtype=F32, device="cuda")
    K.crf_constrained_llh(ec, m, al, st, en, tr, o[0], o[1], o[2])
    assert torch.equal(o[0], llh[0]) and torch.equal(o[1], lz[0]) and torch.equal(o[2], lza[0])
    de2 = torch.empty(B, S, C, dtype=F32, device="cuda")
    g2 = [torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, C, device="cuda")]
    K.crf_constrained_grad(ec, m, al, st, en, tr, w, de2, *g2)
    assert torch.equal(de2.reshape(B * S, C).view(I32), de.view.view(I32))
    _check_grads(de.view.reshape(B, S, C), [ds[0], dn[0], dt], samples, w.cpu(), "guarded")
    l2, f2, s2 = torch.empty(B, dtype=I32, device="cuda"), torch.empty(B * S, dtype=I32, device="cuda"), torch.empty(B, device="cuda")
    K.crf_constrained_decode(ec, m, al, st, en, tr, l2, f2, s2)
    assert torch.equal(l2, lens[0]) and torch.equal(f2[:n], flat[0, :n]) and torch.equal(s2, sc[0])


# ---------------------------------------------------------------------------------------- 8., 9. the module's ways
def test_a_second_backward_accumulates_and_zero_grad_overwrites():
    B, S, C = 5, 37, 13
    e, mask, allowed, P, samples = _case(B, S, C, "prefix", "partial")
    crf = _crf(C, P)
    ones = torch.ones(B)
    ga, gf = CO.param_grads(samples, ones)
    ref = [a - f for a, f in zip(ga, gf)]
    bars = [1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5 for a, f in zip(ga, gf)]
    ps = (crf.start_transitions, crf.end_transitions, crf.transitions)
    eg = e.cuda().requires_grad_(True)
    crf.constrained_llh(eg, allowed.cuda(), mask=mask.cuda(), reduction="sum").backward()
    for p, r, bar in zip(ps, ref, bars):
        assert (p.grad.cpu().double() - r).abs().max().item() < bar
    crf.constrained_llh(eg, allowed.cuda(), mask=mask.cuda(), reduction="sum").backward()          # adds
    for p, r, bar in zip(ps, ref, bars):
        assert (p.grad.cpu().double() - 2 * r).abs().max().item() < 2 * bar
    crf.zero_grad()
    crf.constrained_llh(eg, allowed.cuda(), mask=mask.cuda(), reduction="sum").backward()          # overwrites
    for p, r, bar in zip(ps, ref, bars):
        assert (p.grad.cpu().double() - r).abs().max().item() < bar
    # the reductions of forward
    n_tok = float(mask.sum())
    want = {"sum": sum(s.llh for s in samples), "mean": sum(s.llh for s in samples) / B,
            "token_mean": sum(s.llh for s in samples) / n_tok}
    bar = sum(_bar_lz(s.log_z) + _bar_lz(s.log_za) for s in samples)
    for red, v in want.items():
        got = crf.constrained_llh(e.cuda(), allowed.cuda(), mask=mask.cuda(), reduction=red).item()
        assert abs(got - v) <= bar / (1.0 if red == "sum" else B if red == "mean" else n_tok), (red, got, v)


@pytest.mark.parametrize("form", ["bits", "bool", "uint8"])
def test_sequence_first_layout_and_boolean_sets(form):
    B, S, C = 5, 37, 13
    e, mask, allowed, P, samples = _case(B, S, C, "holes", "random")
    if form == "bits":
        al_sf = allowed.t()
    else:
        bits = torch.tensor([[[(int(allowed[b, t]) >> j) & 1 for j in range(C)] for t in range(S)] for b in range(B)])
        al_sf = bits.transpose(0, 1).to(torch.bool if form == "bool" else torch.uint8)
    w = torch.linspace(0.5, 1.5, B)
    bf = _crf(C, P)
    out, de, pg = _llh_and_grads(bf, e, mask, allowed, w)
    sf = _crf(C, P, batch_first=False)
    eg = e.transpose(0, 1).cuda().requires_grad_(True)
    out2 = sf.constrained_llh(eg, al_sf.cuda(), mask=mask.t().cuda().bool(), reduction="none")
    (out2 * w.cuda()).sum().backward()
    assert torch.equal(out2.detach(), out) and torch.equal(eg.grad.transpose(0, 1), de)
    _check_grads(eg.grad.transpose(0, 1), [p.grad for p in (sf.start_transitions, sf.end_transitions, sf.transitions)],
                 samples, w, "sequence first")
    h = bf.constrained_decode(e.cuda(), allowed.cuda(), mask=mask.cuda()).host()
    h2 = sf.constrained_decode(e.transpose(0, 1).cuda(), al_sf.cuda(), mask=mask.t().cuda()).host()
    assert h == h2 and h["lens"] == [s.L for s in samples]


# -------------------------------------------------------------------------------------------- 10. graph capture
def test_llh_backward_and_decode_are_capturable():
    B, S, C = 5, 37, 13
    cases = [_case(B, S, C, "prefix", "partial"), _case(B, S, C, "holes", "random"), _case(B, S, C, "first_off", "random", None, 2)]
    P = cases[0][3]
    crf = _crf(C, P)
    ps = (crf.start_transitions, crf.end_transitions, crf.transitions)
    w = torch.linspace(0.5, 1.5, B).cuda()
    st_e = cases[0][0].cuda().requires_grad_(True)
    st_m, st_a = cases[0][1].cuda().clone(), cases[0][2].cuda().clone()
    (crf.constrained_llh(st_e, st_a, mask=st_m, reduction="none") * w).sum().backward()      # warm-up outside the capture
    crf.constrained_decode(st_e.detach(), st_a, mask=st_m)
    torch.cuda.synchronize()
    crf.zero_grad(set_to_none=True)
    st_e.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        llh = crf.constrained_llh(st_e, st_a, mask=st_m, reduction="none")
        (llh * w).sum().backward()
        paths = crf.constrained_decode(st_e.detach(), st_a, mask=st_m)
    for e2, mask2, al2, _, _ in cases[1:]:
        samples = CO.batch(e2, mask2, al2, *P)           # (the cases were drawn with parameters of their own)
        with torch.no_grad():
            st_e.copy_(e2.cuda()); st_m.copy_(mask2.cuda()); st_a.copy_(al2.cuda())
        graph.replay()
        torch.cuda.synchronize()
        eager = _crf(C, P)
        out, de, pg = _llh_and_grads(eager, e2, mask2, al2, w.cpu())
        assert torch.equal(llh.detach().view(I32), out.view(I32)) and torch.equal(st_e.grad.view(I32), de.view(I32))
        ga, gf = CO.param_grads(samples, w.cpu())
        for p, g, a, f in zip(ps, pg, ga, gf):
            bar = 1e-3 * (a.abs().max().item() + f.abs().max().item()) + 4e-5
            assert (p.grad - g).abs().max().item() < bar
            assert (p.grad.cpu().double() - (a - f)).abs().max().item() < bar
        h, he = paths.host(), eager.constrained_decode(e2.cuda(), al2.cuda(), mask=mask2.cuda()).host()
        assert h == he and h["lens"] == [s.L for s in samples]
        assert h["infeasible"] == sum(1 for s in samples if not s.feasible)


# ---------------------------------------------------------------------------------------------- 11. composition
def test_paths_compose_with_the_posterior_and_the_chunk_evaluator():
    from icka_amd import metrics
    C = len(metrics.REFERENCE_LABEL_LIST)
    B, S = 6, 40
    e, mask, allowed, P, samples = _case(B, S, C, "prefix", "partial")
    crf = _crf(C, P)
    paths = crf.constrained_decode(e.cuda(), allowed.cuda(), mask=mask.cuda())
    post = crf.posterior(e.cuda(), paths.tags, mask.cuda())
    h, hp = paths.host(), post.host()
    assert hp["bad"] == 0 and hp["lens"] == h["lens"]
    off = 0
    for b, s in enumerate(samples):
        assert abs(hp["seq_logp"][b] - (s.score(h["paths"][b]) - s.log_z)) <= 2 * _bar_lz(s.log_z) + 1e-5 * abs(h["scores"][b])
        assert hp["seq_logp"][b] <= s.llh + 2 * _bar_lz(s.log_z) + _bar_lz(s.log_za)     # one path of A weighs less than all of A
        assert hp["tags_flat"][off:off + s.L] == h["paths"][b]
        off += s.L
    labels = torch.randint(0, C, (B, S), generator=torch.Generator().manual_seed(1))
    ev, ev2 = metrics.ChunkEvaluator.for_label_list(metrics.REFERENCE_LABEL_LIST), metrics.ChunkEvaluator.for_label_list(metrics.REFERENCE_LABEL_LIST)
    ev.update(paths.tags, labels.cuda(), mask.cuda())
    ev2.update(paths.tolist(), labels.cuda(), mask.cuda())
    assert ev.compute().counts == ev2.compute().counts and ev.compute().counts["kept_tokens"] > 0


# ------------------------------------------------------------------------------------------------- 12. refusals
@pytest.mark.parametrize("B,S,C,entry,word", [(1, 193, 64, "llh", "12288"), (1, 193, 64, "grad", "12288"), (1, 193, 64, "decode", "12288"),
                                              (2049, 1, 2, "decode", "2048")])
def test_refusals_name_the_limit_and_write_nothing(B, S, C, entry, word):
    from icka_amd import _lib
    from icka_amd import kernels as K
    dev = "cuda"
    e, al = torch.zeros(B, S, C, device=dev), torch.full((B, S), -1, dtype=I64, device=dev)
    st, en, tr = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, C, device=dev)
    fill = lambda *s: torch.full(s, 7.0, device=dev)
    ifill = lambda *s: torch.full(s, 7, dtype=I32, device=dev)
    outs = {"llh": [fill(B), fill(B), fill(B), ifill(1)], "grad": [fill(B, S, C), fill(C), fill(C), fill(C, C)],
            "decode": [ifill(B), ifill(B * S), fill(B), ifill(1)]}[entry]
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    with pytest.raises(ValueError, match=word):
        if entry == "llh":
            K.crf_constrained_llh(e, None, al, st, en, tr, *outs)
        elif entry == "grad":
            K.crf_constrained_grad(e, None, al, st, en, tr, fill(B), *outs)
        else:
            K.crf_constrained_decode(e, None, al, st, en, tr, *outs)
    # the C entry itself refuses too: ICKA_E_SHAPE, nothing launched
    if entry == "llh":
        rc = lib.icka_crf_constrained_llh(_ptr(e), C, None, _ptr(al), _ptr(st), _ptr(en), _ptr(tr), *[_ptr(o) for o in outs], B, S, C, s)
    elif entry == "grad":
        rc = lib.icka_crf_constrained_grad(_ptr(e), C, None, _ptr(al), _ptr(st), _ptr(en), _ptr(tr), _ptr(fill(B)), _ptr(outs[0]), C,
                                           _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), B, S, C, s)
    else:
        rc = lib.icka_crf_constrained_decode(_ptr(e), C, None, _ptr(al), _ptr(st), _ptr(en), _ptr(tr), _ptr(outs[0]), _ptr(outs[1]),
                                             B * S, _ptr(outs[2]), _ptr(outs[3]), B, S, C, s)
    assert rc == -1
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    if entry == "decode":
        from icka_amd.crf import CRF
        with pytest.raises(ValueError, match=word):
            CRF(C, batch_first=True).cuda().constrained_decode(e, al)
