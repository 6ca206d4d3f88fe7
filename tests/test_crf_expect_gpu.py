"""GPU: the CRF expectations (icka_crf_expect / icka_crf_expect_grad; CRF.log_partition / entropy / kl_divergence / expected /
expected_cost) against the float64 oracle of tests/crf_expect_oracle.py.

Bars.  ``log_z`` keeps the bar of tests/test_crf_gpu.py: rtol 2e-5, atol 2e-4.  Every other quantity is held to 2 x the largest
error measured on the MI355X over exactly the cases of this file, each error divided by the scale its f32 rounding grows with:

  quantity   scale                                                           measured    bar
  expect     max(1, |expect|)                                                4.59e-5     9.2e-5
  H          max(1, |log Z|)         (H = log Z - expect: two such terms)     1.23e-7     2.5e-7
  KL         max(1, |log Z_p|, |log Z_q|, |expect|)    (three such terms)     1.92e-7     3.9e-7
  d_e        max(1, largest oracle cell)   d_emissions of either lattice      1.74e-5     3.5e-5
  d_par      max(1, largest oracle cell)   the six parameter gradients        1.83e-5     3.7e-5

The largest unscaled errors behind them: expect 1.4e-4 at |expect| = 338 (the benchmark shape) and 4.6e-5 at |expect| = 0.03
(where log Z = 250: the filtering weights carry the rounding of alpha), H 4.0e-5 at log Z = 334, KL 4.8e-5 at log Z = 253,
d_emissions 4.3e-5 (cells up to 3.2) and parameter gradients 2.7e-4 (cells up to 103), both at the benchmark shape.
(d_emissions, unscaled, stays 40 x below the 2e-3 the existing CRF gradients are held to.)  A parameter gradient sums B samples with
atomics in any order; two runs of one call agree within the d_par bar, not bit for bit."""
import functools
import math

import pytest
import torch

import crf_constrained_oracle as CO
import crf_expect_oracle as EO
import kernel_check as kc

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
SHAPES = [(4, 6, 3), (5, 37, 13), (3, 70, 17), (2, 9, 64)]      # enumeration size | C <= 16 | C > 16, two mask words | 64 lanes
BIG = (32, 128, 13)
MASKS = ["none", "prefix", "holes", "first_off"]
# which parts of the second lattice are given: none | the emissions only | all four
COMBOS = [(False, "all"), (True, "all"), (False, "e"), (True, "e")]      # (relative, parts), one per mask kind; + (True, "none")
BARS = {"expect": 9.2e-5, "H": 2.5e-7, "KL": 3.9e-7, "d_e": 3.5e-5, "d_par": 3.7e-5}


def _note(q, err, scale, what):
    n = err / max(1.0, scale)
    print("MEASURE %-6s %.3e  (err %.3e, scale %.3e, bar %.1e)  %s" % (q, n, err, scale, BARS[q], what))
    assert math.isfinite(err) and n <= BARS[q], (q, what, err, scale, BARS[q])


def _bar_lz(ref):
    return 2e-4 + 2e-5 * abs(ref)


def _cu(t):
    return None if t is None else t.cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _case(B, S, C, mask_kind, variant="plain"):
    """(p = (e, start, end, trans), mask, q = the second lattice) f32 on the host -- computed once, shared, never modified.
    ``forbid``: a third of the transitions of p are -1e4."""
    seed = B * 1000 + S * 10 + C + 7 * MASKS.index(mask_kind)
    p = list(CO.inputs(B, S, C, seed))
    q = list(EO.second_lattice(B, S, C, seed + 2))
    if variant == "forbid":
        g = torch.Generator().manual_seed(seed + 3)
        p[3] = torch.where(torch.rand(C, C, generator=g) < 0.33, torch.full((C, C), -1e4), p[3])
    return tuple(p), CO.make_mask(mask_kind, B, S, seed + 1), tuple(q)


def _second(q, parts):
    return {"none": [None] * 4, "e": [q[0], None, None, None], "all": list(q)}[parts]


@functools.lru_cache(maxsize=None)
def _ref(B, S, C, mask_kind, relative, parts, variant="plain"):
    """the oracle of one launcher case: (log_z, expect, the eight gradients of sum_b (v_b log_z_b + w_b expect_b), v, w)"""
    p32, mask, q32 = _case(B, S, C, mask_kind, variant)
    p, q = EO.leaves(*p32), EO.leaves(*_second(q32, parts))
    lz, ex = EO.expect(p, q, relative, mask)
    v, w = torch.linspace(-0.5, 1.5, B, dtype=F64), torch.linspace(0.75, 1.25, B, dtype=F64)
    g = EO.grads((v * lz + w * ex).sum(), p + q)
    return lz.detach(), ex.detach(), g, v, w


def _cell(ref):
    return ref.abs().max().item()


def _check_grads(got, ref, what):
    """got / ref: eight tensors (first lattice e, start, end, trans; second likewise), None where not given"""
    for n, (mine, r) in enumerate(zip(got, ref)):
        if r is None:
            assert mine is None
            continue
        name = ("e", "start", "end", "trans")[n % 4] + ("" if n < 4 else "2")
        assert not torch.isnan(mine).any(), (what, name)
        _note("d_e" if n % 4 == 0 else "d_par", (mine.detach().cpu().double() - r).abs().max().item(), _cell(r),
              "%s d_%s" % (what, name))


def _off_rows_are_zero(d, mask):
    if mask is None or d is None:
        return
    off = (mask == 0)
    off[:, 0] = False
    rows = d.cpu()[off]
    assert torch.equal(rows.view(I32), torch.zeros_like(rows).view(I32))


# --------------------------------------------------------------------------------------------------- 1. launchers
def _launchers(B, S, C, mask_kind, relative, parts, variant="plain"):
    """both entries through the C ABI: the operands at row strides of their own inside NaN bands, every output inside sentinel
    bands; then the contiguous launchers, bit for bit"""
    from icka_amd import _lib
    from icka_amd import kernels as K
    lib = _lib.load()
    p32, mask, q32 = _case(B, S, C, mask_kind, variant)
    sec = _second(q32, parts)
    lz_ref, ex_ref, g_ref, v, w = _ref(B, S, C, mask_kind, relative, parts, variant)
    what = "[%d,%d,%d] %s %s %s %s" % (B, S, C, mask_kind, "relative" if relative else "given", parts, variant)
    st, en, tr = [t.cuda() for t in p32[1:]]
    s_st, s_en, s_tr = [_cu(t) for t in sec[1:]]
    m = _cu(mask)
    ld, ld2, ldd, ldd2 = C + 3, C + 1, C + 5, C + 2
    eg = kc.guarded_input(p32[0].reshape(B * S, C), ld=ld)
    sg = None if sec[0] is None else kc.guarded_input(sec[0].reshape(B * S, C), ld=ld2)
    s = torch.cuda.current_stream().cuda_stream
    (lz, c1), (ex, c2) = kc.guarded(1, B, F32), kc.guarded(1, B, F32)
    assert lib.icka_crf_expect(_ptr(eg), ld, _ptr(m), _ptr(st), _ptr(en), _ptr(tr), _ptr(sg), ld2, _ptr(s_st), _ptr(s_en),
                               _ptr(s_tr), int(relative), _ptr(lz), _ptr(ex), B, S, C, s) == 0
    vg, wg = v.float().cuda(), w.float().cuda()
    de = kc.Guarded(B * S, C, F32, ld=ldd)
    d2 = None if sg is None else kc.Guarded(B * S, C, F32, ld=ldd2)
    (ds, c3), (dn, c4), (dt, c5) = kc.guarded(1, C, F32, init=0.0), kc.guarded(1, C, F32, init=0.0), kc.guarded(C, C, F32, init=0.0)
    second_par = [None if t is None else kc.guarded(*shape, F32, init=0.0)
                  for t, shape in zip(sec[1:], ((1, C), (1, C), (C, C)))]
    d2s, d2n, d2t = [None if x is None else x[0] for x in second_par]
    assert lib.icka_crf_expect_grad(_ptr(eg), ld, _ptr(m), _ptr(st), _ptr(en), _ptr(tr), _ptr(sg), ld2, _ptr(s_st), _ptr(s_en),
                                    _ptr(s_tr), int(relative), _ptr(vg), _ptr(wg), _ptr(de.view), ldd, _ptr(ds), _ptr(dn),
                                    _ptr(dt), None if d2 is None else _ptr(d2.view), ldd2, _ptr(d2s), _ptr(d2n), _ptr(d2t),
                                    B, S, C, s) == 0
    torch.cuda.synchronize()
    for chk in [c1, c2, c3, c4, c5, de.check] + ([] if d2 is None else [d2.check]) + [x[1] for x in second_par if x is not None]:
        chk()
    for b in range(B):
        print("%s sample %d: log_z %.6f (ref %.6f) expect %.6f (ref %.6f)" % (what, b, lz[0, b], lz_ref[b], ex[0, b], ex_ref[b]))
        assert abs(float(lz[0, b]) - float(lz_ref[b])) <= _bar_lz(float(lz_ref[b])), (what, b)
        _note("expect", abs(float(ex[0, b]) - float(ex_ref[b])), abs(float(ex_ref[b])), what)
    got = [de.view.reshape(B, S, C), ds[0], dn[0], dt, None if d2 is None else d2.view.reshape(B, S, C),
           None if d2s is None else d2s[0], None if d2n is None else d2n[0], d2t]
    _check_grads(got, g_ref, what)
    _off_rows_are_zero(got[0], mask)
    _off_rows_are_zero(got[4], mask)
    # the contiguous launchers
    ec, sc = p32[0].cuda(), _cu(sec[0])
    o = torch.empty(2, B, dtype=F32, device="cuda")
    kw = dict(second=sc, second_start=s_st, second_end=s_en, second_trans=s_tr, relative=relative)
    K.crf_expect(ec, m, st, en, tr, o[0], o[1], **kw)
    assert torch.equal(o[0], lz[0]) and torch.equal(o[1], ex[0])
    o2 = torch.empty(B, dtype=F32, device="cuda")
    K.crf_expect(ec, m, st, en, tr, o2, None, **kw)                        # log Z alone
    assert torch.equal(o2, lz[0])
    de2 = torch.empty(B, S, C, dtype=F32, device="cuda")
    dd2 = None if sc is None else torch.empty(B, S, C, dtype=F32, device="cuda")
    K.crf_expect_grad(ec, m, st, en, tr, vg, wg, de2, None, None, None, d_second=dd2, **kw)
    assert torch.equal(de2.reshape(B * S, C).view(I32), de.view.view(I32))
    if dd2 is not None:
        assert torch.equal(dd2.reshape(B * S, C).view(I32), d2.view.view(I32))
    return got, (ec, m, st, en, tr, vg, wg, kw)


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_launchers_against_the_oracle(B, S, C, mask_kind):
    _launchers(B, S, C, mask_kind, True, "none")                            # the entropy's call
    _launchers(B, S, C, mask_kind, *COMBOS[MASKS.index(mask_kind)])


def test_launchers_against_the_oracle_at_the_benchmark_shape():
    _launchers(*BIG, "prefix", True, "all")


def test_one_position():
    """S = 1, and a sample with L = 1 among longer ones: start, the row and end are the whole path"""
    for relative, parts in COMBOS:
        _launchers(3, 1, 13, "none", relative, parts)
    p32, mask, _ = _case(5, 37, 13, "prefix")
    assert int(mask[1].sum()) == 1
    _launchers(5, 37, 13, "prefix", True, "all")


def test_null_gradient_buffers_skip_their_side_and_change_nothing_else():
    from icka_amd import kernels as K
    B, S, C = 5, 37, 13
    for relative in (False, True):
        got, (ec, m, st, en, tr, vg, wg, kw) = _launchers(B, S, C, "holes", relative, "all")
        g_ref = _ref(B, S, C, "holes", relative, "all")[2]
        z = lambda *shape: torch.zeros(*shape, dtype=F32, device="cuda")
        sent = lambda *shape: torch.full(shape, 7.0, dtype=F32, device="cuda")
        # the first lattice detached: only the second's gradients, bit for bit (the covariance is skipped)
        d2, p2 = torch.empty(B, S, C, device="cuda"), [z(C), z(C), z(C, C)]
        K.crf_expect_grad(ec, m, st, en, tr, vg, wg, None, None, None, None, d_second=d2, d_second_start=p2[0],
                          d_second_end=p2[1], d_second_trans=p2[2], **kw)
        assert torch.equal(d2.view(I32), got[4].view(I32))
        _check_grads([None] * 4 + [d2] + p2, [None] * 4 + g_ref[4:], "first lattice detached")
        # the second lattice detached
        de, p1 = torch.empty(B, S, C, device="cuda"), [z(C), z(C), z(C, C)]
        K.crf_expect_grad(ec, m, st, en, tr, vg, wg, de, *p1, **kw)
        assert torch.equal(de.view(I32), got[0].view(I32))
        _check_grads([de] + p1 + [None] * 4, g_ref[:4] + [None] * 4, "second lattice detached")
        # single buffers
        only = z(C, C)
        K.crf_expect_grad(ec, m, st, en, tr, vg, wg, None, None, None, only, **kw)
        _check_grads([None, None, None, only] + [None] * 4, [None, None, None, g_ref[3]] + [None] * 4, "d_trans alone")
        # no upstream gradient of expect: log Z's gradient, and exact zeros for the second lattice
        lz_only = EO.leaves(ec.cpu(), st.cpu(), en.cpu(), tr.cpu())
        g_lz = EO.grads((vg.cpu().double() * EO.log_z(*lz_only, None if m is None else m.cpu())).sum(), lz_only)
        de, p1, d2 = torch.empty(B, S, C, device="cuda"), [z(C), z(C), z(C, C)], sent(B, S, C)
        K.crf_expect_grad(ec, m, st, en, tr, vg, None, de, *p1, d_second=d2, **kw)
        _check_grads([de] + p1 + [None] * 4, g_lz + [None] * 4, "g_expect = None")
        assert not d2.any()


# ------------------------------------------------------------------------------------------------ 2. the module
def _crf(C, params, batch_first=True):
    from icka_amd.crf import CRF
    crf = CRF(C, batch_first=batch_first).cuda()
    with torch.no_grad():
        for p, v in zip((crf.start_transitions, crf.end_transitions, crf.transitions), params):
            p.copy_(v)
    return crf


def _pars(crf):
    return (crf.start_transitions, crf.end_transitions, crf.transitions)


def _backward(out, w, mods, tensors):
    """d sum_b w_b out_b -> ([grad of each tensor], [[the three parameter gradients] of each module])"""
    for mod in mods:
        mod.zero_grad(set_to_none=True)
    (out * w.float().cuda()).sum().backward()
    return [t.grad for t in tensors], [[None if p.grad is None else p.grad.clone() for p in _pars(mod)] for mod in mods]


W = lambda B: torch.linspace(0.5, 1.5, B, dtype=F64)
METHOD_SHAPES = [(5, 37, 13, "holes"), (3, 70, 17, "prefix"), (2, 9, 64, "first_off")]


@pytest.mark.parametrize("B,S,C,mask_kind", METHOD_SHAPES)
def test_log_partition_and_entropy(B, S, C, mask_kind):
    p32, mask, _ = _case(B, S, C, mask_kind)
    w = W(B)
    p = EO.leaves(*p32)
    lz_ref = EO.log_z(*p, mask)
    g_lz = EO.grads((w * lz_ref).sum(), p)
    H_ref = EO.entropy(p, mask)
    g_H = EO.grads((w * H_ref).sum(), p)
    crf = _crf(C, p32[1:])
    eg = p32[0].cuda().requires_grad_(True)
    lz = crf.log_partition(eg, mask=_cu(mask))
    for b in range(B):
        assert abs(float(lz[b]) - float(lz_ref[b])) <= _bar_lz(float(lz_ref[b]))
    (ge,), (gp,) = _backward(lz, w, [crf], [eg])
    _check_grads([ge] + gp + [None] * 4, g_lz + [None] * 4, "log_partition")
    _off_rows_are_zero(ge, mask)
    eg = p32[0].cuda().requires_grad_(True)
    H = crf.entropy(eg, mask=_cu(mask))
    on = EO.on_mask(mask, B, S)
    for b in range(B):
        _note("H", abs(float(H[b]) - float(H_ref[b])), abs(float(lz_ref[b])), "entropy sample %d" % b)
        bar = BARS["H"] * max(1.0, abs(float(lz_ref[b])))
        assert -bar <= float(H[b]) <= int(on[b].sum()) * math.log(C) + bar
    (ge,), (gp,) = _backward(H, w, [crf], [eg])
    _check_grads([ge] + gp + [None] * 4, g_H + [None] * 4, "entropy")
    _off_rows_are_zero(ge, mask)


def _kl_ref(p32, q32, mask, w, shared):
    """the oracle of KL(p || q): value, log Z's, expect and the gradients (e, p's three, e2, q's three -- with ``shared`` the
    parameters are p's own and their gradient holds both roles)"""
    p = EO.leaves(*p32)
    q = EO.leaves(q32[0]) + (p[1:] if shared else EO.leaves(*q32[1:]))
    lz, ex = EO.expect(p, q, True, mask)
    lzq = EO.log_z(*q, mask)
    kl = ex - lz + lzq
    g = EO.grads((w * kl).sum(), p + ([q[0], None, None, None] if shared else q))
    scale = [max(abs(float(a)), abs(float(b)), abs(float(c))) for a, b, c in zip(lz.detach(), lzq.detach(), ex.detach())]
    return kl.detach(), scale, g


@pytest.mark.parametrize("detach", ["none", "self", "other"])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,S,C,mask_kind", METHOD_SHAPES)
def test_kl_divergence(B, S, C, mask_kind, shared, detach):
    p32, mask, q32 = _case(B, S, C, mask_kind)
    w = W(B)
    kl_ref, scale, g = _kl_ref(p32, q32, mask, w, shared)
    crf = _crf(C, p32[1:])
    other = None if shared else _crf(C, q32[1:])
    eg, e2 = p32[0].cuda().requires_grad_(True), q32[0].cuda().requires_grad_(True)
    kl = crf.kl_divergence(eg, e2, mask=_cu(mask), other=other, detach=detach)
    what = "kl %s %s" % ("shared" if shared else "other", detach)
    for b in range(B):
        _note("KL", abs(float(kl[b]) - float(kl_ref[b])), scale[b], "%s sample %d" % (what, b))
        assert float(kl[b]) >= -BARS["KL"] * max(1.0, scale[b])
    mods = [crf] + ([] if shared else [other])
    (ge, ge2), pg = _backward(kl, w, mods, [eg, e2])
    # slots: e, p's three, e2, q's three; shared parameters hold both roles in p's slots
    if detach == "self":                  # p is a constant: q's gradients alone
        assert ge is None
        if shared:
            p = EO.leaves(*p32)
            qe = EO.leaves(q32[0])[0]
            q = [qe] + p[1:]
            lz, ex = EO.expect([t.detach() for t in p], q, True, mask)
            gq = EO.grads((w * (ex - lz + EO.log_z(*q, mask))).sum(), p[1:] + [qe])
            g, got = [None] + gq[:3] + [gq[3], None, None, None], [None] + pg[0] + [ge2, None, None, None]
        else:
            assert all(x is None for x in pg[0])
            g, got = [None] * 4 + g[4:], [None] * 4 + [ge2] + pg[1]
    elif detach == "other":               # q is a constant: p's gradients alone
        assert ge2 is None
        if shared:
            p = EO.leaves(*p32)
            q = [q32[0].double()] + [t.detach() for t in p[1:]]
            lz, ex = EO.expect(p, q, True, mask)
            g = EO.grads((w * (ex - lz + EO.log_z(*q, mask))).sum(), p) + [None] * 4
        else:
            assert all(x is None for x in pg[1])
            g = g[:4] + [None] * 4
        got = [ge] + pg[0] + [None] * 4
    else:
        got = [ge] + pg[0] + [ge2] + ([None] * 3 if shared else pg[1])
    _check_grads(got, g, what)
    _off_rows_are_zero(ge, mask)
    _off_rows_are_zero(ge2, mask)


@pytest.mark.parametrize("B,S,C,mask_kind", METHOD_SHAPES)
def test_expected_and_expected_cost(B, S, C, mask_kind):
    p32, mask, q32 = _case(B, S, C, mask_kind)
    w = W(B)
    p, q = EO.leaves(*p32), EO.leaves(*q32)
    ex_ref = EO.expect(p, q, False, mask)[1]
    g = EO.grads((w * ex_ref).sum(), p + q)
    crf = _crf(C, p32[1:])
    eg = p32[0].cuda().requires_grad_(True)
    pay = [t.cuda().requires_grad_(True) for t in q32]
    ex = crf.expected(eg, pay[0], mask=_cu(mask), payoff_start=pay[1], payoff_end=pay[2], payoff_transitions=pay[3])
    for b in range(B):
        _note("expect", abs(float(ex[b]) - float(ex_ref[b])), abs(float(ex_ref[b])), "expected sample %d" % b)
    got, (gp,) = _backward(ex, w, [crf], [eg] + pay)
    _check_grads([got[0]] + gp + got[1:], g, "expected")
    # the expected Hamming cost, and a cost matrix of one's own
    tags = torch.randint(0, C, (B, S), generator=torch.Generator().manual_seed(B + S))
    tags[:, -1] = -100                                                       # a pad label is clamped where it is read
    for cost in (None, q32[3].abs()):
        cm = (1.0 - torch.eye(C)) if cost is None else cost
        payoff = cm.double()[tags.clamp(0, C - 1)]
        p = EO.leaves(*p32)
        ref = EO.expect(p, [payoff, None, None, None], False, mask)[1]
        g = EO.grads((w * ref).sum(), p)
        eg = p32[0].cuda().requires_grad_(True)
        ec = crf.expected_cost(eg, tags.cuda(), mask=_cu(mask), cost=_cu(cost))
        on = EO.on_mask(mask, B, S)
        for b in range(B):
            _note("expect", abs(float(ec[b]) - float(ref[b])), abs(float(ref[b])), "expected_cost sample %d" % b)
            if cost is None:
                assert -BARS["expect"] * S <= float(ec[b]) <= int(on[b].sum()) * (1 + BARS["expect"])
        (ge,), (gp,) = _backward(ec, w, [crf], [eg])
        _check_grads([ge] + gp + [None] * 4, g + [None] * 4, "expected_cost")


def test_sequence_first_layout_reductions_and_accumulation():
    B, S, C = 5, 37, 13
    p32, mask, q32 = _case(B, S, C, "holes")
    w = W(B)
    bf, sf = _crf(C, p32[1:]), _crf(C, p32[1:], batch_first=False)
    on = EO.on_mask(mask, B, S)
    tags = torch.randint(0, C, (B, S), generator=torch.Generator().manual_seed(3))
    calls = {
        "log_partition": lambda crf, e, e2, m, t: crf.log_partition(e, mask=m),
        "entropy": lambda crf, e, e2, m, t: crf.entropy(e, mask=m),
        "kl_divergence": lambda crf, e, e2, m, t: crf.kl_divergence(e, e2, mask=m),
        "expected": lambda crf, e, e2, m, t: crf.expected(e, e2, mask=m),
        "expected_cost": lambda crf, e, e2, m, t: crf.expected_cost(e, t, mask=m),
    }
    for name, call in calls.items():
        e1, e2 = p32[0].cuda().requires_grad_(True), q32[0].cuda().requires_grad_(True)
        out = call(bf, e1, e2, mask.cuda(), tags.cuda())
        (g1, g2), (gp,) = _backward(out, w, [bf], [e1, e2])
        t1, t2 = p32[0].transpose(0, 1).cuda().requires_grad_(True), q32[0].transpose(0, 1).cuda().requires_grad_(True)
        out2 = call(sf, t1, t2, mask.t().cuda().bool(), tags.t().cuda())
        (h1, h2), (hp,) = _backward(out2, w, [sf], [t1, t2])
        assert torch.equal(out2.detach(), out.detach()) and torch.equal(h1.transpose(0, 1), g1), name
        assert (g2 is None and h2 is None) or torch.equal(h2.transpose(0, 1), g2), name
        for a, b in zip(gp, hp):                                            # atomics: any order
            assert (a - b).abs().max().item() <= BARS["d_par"] * max(1.0, a.abs().max().item()), name
    # every reduction, on the entropy and the KL
    n_tok = float(on.sum())
    for name in ("entropy", "kl_divergence"):
        e1, e2 = p32[0].cuda(), q32[0].cuda()
        none = calls[name](bf, e1, e2, mask.cuda(), None).double().cpu()
        for red, want in (("sum", none.sum()), ("mean", none.sum() / B), ("token_mean", none.sum() / n_tok)):
            kw = dict(mask=mask.cuda(), reduction=red)
            got = bf.entropy(e1, **kw) if name == "entropy" else bf.kl_divergence(e1, e2, **kw)
            assert got.dim() == 0 and abs(float(got) - float(want)) <= 1e-5 * abs(float(want)) + 1e-5, (name, red)
    with pytest.raises(ValueError, match="invalid reduction"):
        bf.entropy(p32[0].cuda(), reduction="max")
    # a second backward adds, zero_grad starts over
    p = EO.leaves(*p32)
    g = EO.grads(EO.entropy(p, mask).sum(), p)
    e1 = p32[0].cuda().requires_grad_(True)
    bf.zero_grad(set_to_none=True)
    bf.entropy(e1, mask=mask.cuda(), reduction="sum").backward()
    _check_grads([e1.grad] + [x.grad for x in _pars(bf)] + [None] * 4, g + [None] * 4, "first backward")
    bf.entropy(e1, mask=mask.cuda(), reduction="sum").backward()
    _check_grads([0.5 * e1.grad] + [0.5 * x.grad for x in _pars(bf)] + [None] * 4, g + [None] * 4, "second backward / 2")
    bf.zero_grad()
    e1.grad = None
    bf.entropy(e1, mask=mask.cuda(), reduction="sum").backward()
    _check_grads([e1.grad] + [x.grad for x in _pars(bf)] + [None] * 4, g + [None] * 4, "after zero_grad")


# ------------------------------------------------------------------------------------------------- 3. hard cases
def test_a_near_deterministic_distribution():
    """emissions x 30: the entropy is a difference of two numbers of size |log Z| ~ 4000 and stays >= -bar and finite"""
    B, S, C = 5, 37, 13
    p32, mask, _ = _case(B, S, C, "prefix")
    e = (p32[0] * 30.0)
    lz_ref = EO.log_z(e.double(), *[t.double() for t in p32[1:]], mask)
    crf = _crf(C, p32[1:])
    eg = e.cuda().requires_grad_(True)
    H = crf.entropy(eg, mask=mask.cuda())
    (ge,), (gp,) = _backward(H, W(B), [crf], [eg])
    for b in range(B):
        print("x30 sample %d: H %.4e, log Z %.1f" % (b, float(H[b]), float(lz_ref[b])))
        assert math.isfinite(float(H[b])) and float(H[b]) >= -BARS["H"] * max(1.0, abs(float(lz_ref[b])))
    assert torch.isfinite(ge).all() and all(torch.isfinite(x).all() for x in gp)


@pytest.mark.parametrize("B,S,C,mask_kind", [(5, 37, 13, "holes"), (3, 70, 17, "none")])
def test_forbidden_transitions(B, S, C, mask_kind):
    """-1e4 in a third of the transitions: finite and within the bars, values and gradients"""
    got, _ = _launchers(B, S, C, mask_kind, True, "none", "forbid")
    assert all(torch.isfinite(x).all() for x in got if x is not None)
    got, _ = _launchers(B, S, C, mask_kind, False, "all", "forbid")
    assert all(torch.isfinite(x).all() for x in got if x is not None)
    p32, mask, q32 = _case(B, S, C, mask_kind, "forbid")
    w = W(B)
    kl_ref, scale, g = _kl_ref(p32, q32, mask, w, True)        # two views through the one CRF with forbidden transitions
    crf = _crf(C, p32[1:])
    eg, e2 = p32[0].cuda().requires_grad_(True), q32[0].cuda().requires_grad_(True)
    kl = crf.kl_divergence(eg, e2, mask=_cu(mask))
    for b in range(B):
        _note("KL", abs(float(kl[b]) - float(kl_ref[b])), scale[b], "forbid kl sample %d" % b)
    (ge, ge2), (gp,) = _backward(kl, w, [crf], [eg, e2])
    _check_grads([ge] + gp + [ge2, None, None, None], g, "forbid kl")


def test_two_near_equal_views():
    """other_emissions = emissions + 1e-3 noise: KL ~ 1e-6 is the difference of numbers of size |log Z|; the gradient, which is
    what a training step uses, stays within the bars"""
    B, S, C = 5, 37, 13
    p32, mask, q32 = _case(B, S, C, "holes")
    w = W(B)
    near = (p32[0] + 1e-3 * q32[0],) + tuple(q32[1:])
    kl_ref, scale, g = _kl_ref(p32, near, mask, w, True)
    crf = _crf(C, p32[1:])
    eg, e2 = p32[0].cuda().requires_grad_(True), near[0].cuda().requires_grad_(True)
    kl = crf.kl_divergence(eg, e2, mask=mask.cuda())
    for b in range(B):
        _note("KL", abs(float(kl[b]) - float(kl_ref[b])), scale[b], "near views sample %d (ref %.3e)" % (b, float(kl_ref[b])))
        assert float(kl[b]) >= -BARS["KL"] * max(1.0, scale[b])
    (ge, ge2), (gp,) = _backward(kl, w, [crf], [eg, e2])
    _check_grads([ge] + gp + [ge2, None, None, None], g, "near views")


# ------------------------------------------------------------------------------------- 4. validation and capture
def test_every_refusal_comes_before_a_launch():
    from icka_amd import _lib
    from icka_amd import kernels as K
    from icka_amd.crf import CRF
    dev = "cuda"
    B, S, C = 2, 5, 4
    e = torch.zeros(B, S, C, device=dev)
    st, en, tr = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, C, device=dev)
    lz, ex = torch.full((B,), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
    ok = dict(second=e.clone(), second_start=st.clone(), second_end=en.clone(), second_trans=tr.clone(), relative=True)
    bad = [dict(ok, second=e[:, :4]), dict(ok, second=e.double()), dict(ok, second_start=torch.zeros(C + 1, device=dev)),
           dict(ok, second_end=torch.zeros(C, 1, device=dev)), dict(ok, second_trans=torch.zeros(C, C + 1, device=dev)),
           dict(ok, relative=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            K.crf_expect(e, None, st, en, tr, lz, ex, **kw)
        with pytest.raises(ValueError):
            K.crf_expect_grad(e, None, st, en, tr, lz, ex, torch.empty_like(e), None, None, None, **kw)
    with pytest.raises(ValueError, match="log_z"):
        K.crf_expect(e, None, st, en, tr, None, ex)
    with pytest.raises(ValueError, match="expect"):
        K.crf_expect(e, None, st, en, tr, lz, ex[:1])
    with pytest.raises(ValueError, match="mask"):
        K.crf_expect(e, torch.ones(B, S, device=dev), st, en, tr, lz, ex)
    with pytest.raises(ValueError, match="d_trans"):
        K.crf_expect_grad(e, None, st, en, tr, lz, ex, None, None, None, torch.zeros(C, device=dev))
    with pytest.raises(ValueError, match="g_logz"):
        K.crf_expect_grad(e, None, st, en, tr, lz.double(), ex, None, None, None, None)
    with pytest.raises(TypeError):
        K.crf_expect(e, None, st, en, tr, lz, ex, second=e.cpu())
    with pytest.raises(TypeError):
        K.crf_expect_grad(e, None, st, en, tr, lz, ex, e.cpu().clone(), None, None, None)
    # the S * C limit: the launchers, the C entries (ICKA_E_SHAPE, nothing written) and the module
    Sb, Cb = 65, 64
    eb = torch.zeros(1, Sb, Cb, device=dev)
    pb = [torch.zeros(Cb, device=dev), torch.zeros(Cb, device=dev), torch.zeros(Cb, Cb, device=dev)]
    outs = [torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev), torch.full((1, Sb, Cb), 7.0, device=dev),
            torch.full((Cb,), 7.0, device=dev), torch.full((Cb, Cb), 7.0, device=dev)]
    with pytest.raises(ValueError, match="4096"):
        K.crf_expect(eb, None, *pb, outs[0], outs[1])
    with pytest.raises(ValueError, match="4096"):
        K.crf_expect_grad(eb, None, *pb, outs[0], outs[1], outs[2], outs[3], None, outs[4])
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    assert lib.icka_crf_expect(_ptr(eb), Cb, None, *[_ptr(t) for t in pb], None, Cb, None, None, None, 1, _ptr(outs[0]),
                               _ptr(outs[1]), 1, Sb, Cb, s) == -1
    assert lib.icka_crf_expect_grad(_ptr(eb), Cb, None, *[_ptr(t) for t in pb], None, Cb, None, None, None, 1, _ptr(outs[0]),
                                    _ptr(outs[1]), _ptr(outs[2]), Cb, _ptr(outs[3]), None, _ptr(outs[4]), None, Cb, None, None,
                                    None, 1, Sb, Cb, s) == -1
    assert lib.icka_crf_expect(_ptr(e), C, None, _ptr(st), _ptr(en), _ptr(tr), None, C, None, None, None, 2, _ptr(lz), _ptr(ex),
                               B, S, C, s) == -3                              # a mode that is neither
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + [lz, ex])
    big = CRF(Cb, batch_first=True).cuda()
    for call in (lambda: big.entropy(eb), lambda: big.log_partition(eb), lambda: big.kl_divergence(eb, eb),
                 lambda: big.expected(eb, eb), lambda: big.expected_cost(eb, torch.zeros(1, Sb, dtype=I64, device=dev))):
        with pytest.raises(ValueError, match="4096"):
            call()
    # the module's own checks
    crf = CRF(C, batch_first=True).cuda()
    tags = torch.zeros(B, S, dtype=I64, device=dev)
    for call in (lambda: crf.kl_divergence(e, e, other=CRF(C + 1, batch_first=True).cuda()),
                 lambda: crf.kl_divergence(e, e, other="crf"),
                 lambda: crf.kl_divergence(e, e, detach="both"),
                 lambda: crf.kl_divergence(e, e[:, :4]),
                 lambda: crf.kl_divergence(e, e, reduction="max"),
                 lambda: crf.expected(e, e[:, :, :3]),
                 lambda: crf.expected(e, tags),
                 lambda: crf.expected(e, e, payoff_start=torch.zeros(C + 1, device=dev)),
                 lambda: crf.expected(e, e, payoff_transitions=torch.zeros(C, device=dev)),
                 lambda: crf.expected_cost(e, tags.float()),
                 lambda: crf.expected_cost(e, tags[:, :4]),
                 lambda: crf.expected_cost(e, tags, cost=torch.zeros(C, C + 1, device=dev)),
                 lambda: crf.expected_cost(e, tags, cost=torch.zeros(C, C, dtype=F64, device=dev)),
                 lambda: crf.entropy(e[0]),
                 lambda: crf.entropy(e, mask=torch.ones(B, S + 1, device=dev))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: crf.entropy(e.cpu()), lambda: crf.log_partition(e.cpu()), lambda: crf.kl_divergence(e, e.cpu()),
                 lambda: crf.expected(e, e.cpu()), lambda: crf.kl_divergence(e, e, other=CRF(C, batch_first=True))):
        with pytest.raises((TypeError, RuntimeError)):
            call()


def test_entropy_forward_and_backward_are_capturable():
    B, S, C = 5, 37, 13
    first, second = _case(B, S, C, "prefix"), _case(B, S, C, "holes")
    P = first[0][1:]
    crf = _crf(C, P)
    w = W(B).float().cuda()
    st_e, st_m = first[0][0].cuda().requires_grad_(True), first[1].cuda().clone()
    (crf.entropy(st_e, mask=st_m) * w).sum().backward()                     # warm-up outside the capture
    torch.cuda.synchronize()
    crf.zero_grad(set_to_none=True)
    st_e.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H = crf.entropy(st_e, mask=st_m)
        (H * w).sum().backward()
    with torch.no_grad():
        st_e.copy_(second[0][0].cuda())
        st_m.copy_(second[1].cuda())
    graph.replay()
    torch.cuda.synchronize()
    eager = _crf(C, P)
    eg = second[0][0].cuda().requires_grad_(True)
    He = eager.entropy(eg, mask=second[1].cuda())
    (ge,), (gp,) = _backward(He, W(B), [eager], [eg])
    assert torch.equal(H.detach().view(I32), He.detach().view(I32)) and torch.equal(st_e.grad.view(I32), ge.view(I32))
    p = EO.leaves(second[0][0], *P)
    g = EO.grads((W(B) * EO.entropy(p, second[1])).sum(), p)
    _check_grads([st_e.grad] + [x.grad for x in _pars(crf)] + [None] * 4, g + [None] * 4, "replayed")
