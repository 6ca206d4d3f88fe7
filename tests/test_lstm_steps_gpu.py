"""GPU: every recurrence kernel of csrc/lstm.hip, step by step against float64 (tests/lstm_check.py: teacher-forced references
with bounds derived from the number formats), at the smallest shapes that reach each of the 26 instantiations the host code
launches, with guard bands round every operand, each call made twice (bitwise-equal outputs; the second call reads gates_x /
writes dgates through a padded row stride, with the operands the ABI asks no alignment of one element off it) and the hand-off
error word read after each.  tests/test_lstm_gpu.py stays the
check against ATen; this file checks what that one cannot see: single elements, the saved intermediates, the dispatch."""
import functools

import pytest
import torch

import kernel_check as kc
import lstm_check as lc
from kernel_check import BF16, F32

pytestmark = pytest.mark.gpu


def assert_dispatch_coverage(cases=lc.CASES):
    """The union over the case list is every instantiation launched in lstm.hip (also called by tests/test_lstm_check_cpu.py)."""
    return lc.assert_dispatch_coverage(cases)


def _cus():
    """CUs of this device minus the ones reserved (icka_lstm_set_reserved_cus): what the host dispatch compares grids with."""
    from icka_amd import kernels as K
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count - K._LSTM_RESERVED[0]


def _skip_unless_reachable(phase, B, H, fl):
    """On a partitioned device (fewer CUs than a whole MI355X) a case whose instantiation can no longer be reached is skipped;
    on a whole device nothing is."""
    want, got = lc.dispatch(phase, B, H, fl), lc.dispatch(phase, B, H, fl, cus=_cus())
    if got != want:
        pytest.skip("%d CUs: %s<%s> (grid.z %d) is unreachable, the call would take %s<%s>" % (
            _cus(), want[1], want[2], want[3], got[1], got[2]))
    return want


def _inputs(B, S, H):
    g = torch.Generator().manual_seed(B * 1000 + S * 10 + H)
    whh = (torch.randn(8 * H, H, generator=g) * H ** -0.5).to(BF16)          # [2][4H][H]
    gx = torch.randn(B * S, 8 * H, generator=g) * 0.7
    dy = (torch.randn(B * S, 2 * H, generator=g) * 0.3).to(BF16)
    return whh, gx, dy


def _gin(values, ld=None, offset=0):
    """An operand inside NaN bands and NaN pad columns (kc.guarded_input, keeping the object for its check())."""
    return kc.Guarded(values.shape[0], values.shape[1], values.dtype, ld=ld, offset=offset, fill=kc.NAN_FILL[values.dtype],
                      init=values.cuda())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b, what):
    ne = _bits(a) != _bits(b)
    assert not bool(ne.any()), "%s: %d elements differ bitwise between two calls" % (what, int(ne.sum()))


def _err_word(form):
    from icka_amd import _lib
    torch.cuda.synchronize()
    rc = _lib.load().icka_lstm_barrier_error()
    assert rc == 0, "icka_lstm_barrier_error() = %d after a %s launch: a hand-off wait gave up" % (rc, form)


def _fwd_call(B, S, H, fl, gx, whh, want_hprev=True, offset=0):
    """One icka_lstm_fwd into fresh guarded outputs -> {"y", "c_all", "act", "hprev"} (Guarded objects).  ``offset`` moves
    c_all, act and hprev that many elements off the allocation's alignment (the ABI asks 16 bytes of w_hh and y only)."""
    from icka_amd import kernels as K
    M = B * S
    o = {"y": kc.Guarded(M, 2 * H, BF16), "c_all": kc.Guarded(M, 2 * H, F32, offset=offset),
         "act": kc.Guarded(M, 8 * H, BF16, offset=offset), "hprev": kc.Guarded(M, 2 * H, BF16, offset=offset)}
    K.lstm_fwd(gx.view, whh.view, o["y"].view, o["c_all"].view, o["act"].view, o["hprev"].view if want_hprev else None,
               B, S, H, flags=fl)
    torch.cuda.synchronize()
    for n, g in list(o.items()) + [("gates_x", gx), ("w_hh", whh)]:
        g.check(what="forward " + n)
    if not want_hprev:
        assert bool(torch.isnan(o["hprev"].view).all()), "hprev = NULL was written to"
    return o


@functools.lru_cache(maxsize=None)
def _forward(case):
    """The forward of a case, twice: contiguous gates_x, then gates_x with row stride 8H + 4 and every operand the ABI does not
    ask 16 bytes of (gates_x, c_all, act, hprev) one element off it.  Shared by the forward and the backward test of the case
    and left unchanged."""
    B, S, H, fl = case
    whh, gx, dy = _inputs(B, S, H)
    whh_g = _gin(whh)
    a = _fwd_call(B, S, H, fl, _gin(gx), whh_g)
    b = _fwd_call(B, S, H, fl, _gin(gx, ld=8 * H + 4, offset=1), whh_g, offset=1)
    return {"whh": whh_g, "gx": gx.cuda(), "dy": dy, "first": a, "second": b}


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_forward_steps(case):
    B, S, H, fl = case
    form = _skip_unless_reachable("fwd", B, H, fl)[0]
    f = _forward(case)
    if form != "step":
        _err_word(form)
    a, b = f["first"], f["second"]
    for n in ("y", "c_all", "act", "hprev"):
        _same(a[n].view, b[n].view, "%s forward %s (second call: gates_x with ld = 8H + 4)" % (lc.case_id(case), n))
    lc.check_fwd("fwd " + form, f["gx"], f["whh"].view, a["y"].view, a["c_all"].view, a["act"].view, a["hprev"].view, B, S, H)
    kc.report("lstm_fwd " + lc.case_id(case))


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_backward_steps(case):
    from icka_amd import _lib
    from icka_amd import kernels as K
    B, S, H, fl = case
    form = _skip_unless_reachable("bwd", B, H, fl)[0]
    f = _forward(case)
    M = B * S
    whh_t = _gin(f["whh"].view.reshape(2, 4 * H, H).transpose(1, 2).reshape(2 * H, 4 * H).cpu())     # W_hh^T [2][H][4H]
    outs = []
    for ld in (8 * H, 8 * H + 8):
        # second call: dgates with a padded row stride; dy, dc_carry and the forward's act / c_all one element off alignment
        off = 0 if ld == 8 * H else 1
        fw = f["first" if off == 0 else "second"]
        dy = _gin(f["dy"], offset=off)
        dg, carry = kc.Guarded(M, 8 * H, BF16, ld=ld), kc.Guarded(2 * B, H, F32, offset=off)
        if ld == 8 * H:
            K.lstm_bwd(dy.view, whh_t.view, fw["act"].view, fw["c_all"].view, dg.view, carry.view, B, S, H, flags=fl)
        else:           # the wrapper refuses a strided dgates; the C ABI takes ldg >= 8H, ldg % 8 == 0
            rc = _lib.load().icka_lstm_bwd(dy.view.data_ptr(), whh_t.view.data_ptr(), fw["act"].view.data_ptr(),
                                           fw["c_all"].view.data_ptr(), dg.view.data_ptr(), ld, carry.view.data_ptr(), B, S, H,
                                           int(fl), K._stream())
            assert rc == 0, rc
        torch.cuda.synchronize()
        for n, g in (("dgates", dg), ("dc_carry", carry), ("dy", dy), ("w_hh_t", whh_t), ("act", fw["act"]), ("c_all", fw["c_all"])):
            g.check(what="backward %s (ldg %d)" % (n, ld))
        if form != "step":
            _err_word(form)
        outs.append((dg, carry))
    _same(outs[0][0].view, outs[1][0].view, "%s dgates (second call: ldg = 8H + 8)" % lc.case_id(case))
    if form == "step":
        _same(outs[0][1].view, outs[1][1].view, "%s dc_carry" % lc.case_id(case))
    else:       # the persistent kernels keep the carry in registers: an untouched workspace is what tells the forms apart here
        assert bool(torch.isnan(outs[0][1].view).all()), "dc_carry was written: the call took the per-step launches, not %s" % form
    fw = f["first"]
    lc.check_bwd("bwd " + form, f["dy"].cuda(), f["whh"].view, fw["act"].view, fw["c_all"].view, outs[0][0].view,
                 outs[0][1].view if form == "step" else None, B, S, H, rs=form == "rs")
    kc.report("lstm_bwd " + lc.case_id(case))


@pytest.mark.parametrize("case", [(17, 3, 256, 0), (20, 5, 384, 0), (33, 3, 288, 0)], ids=lc.case_id)
def test_forward_without_hprev_is_bitwise_the_same(case):
    B, S, H, fl = case
    _skip_unless_reachable("fwd", B, H, fl)
    f = _forward(case)
    whh, gx, _ = _inputs(B, S, H)
    o = _fwd_call(B, S, H, fl, _gin(gx), f["whh"], want_hprev=False)
    for n in ("y", "c_all", "act"):
        _same(o[n].view, f["first"][n].view, "%s %s with hprev = NULL" % (lc.case_id(case), n))


@pytest.mark.parametrize("case", [c for c in lc.CASES if c[3] & lc.NO_BATCH_SPLIT], ids=lc.case_id)
def test_no_batch_split_is_bitwise_the_split_launch(case):
    """Batch rows are independent recurrences and a row's arithmetic does not depend on the tile it sits in."""
    B, S, H, fl = case
    _skip_unless_reachable("fwd", B, H, fl)
    assert _skip_unless_reachable("fwd", B, H, 0)[3] == 2
    f = _forward(case)
    whh, gx, _ = _inputs(B, S, H)
    o = _fwd_call(B, S, H, 0, _gin(gx), f["whh"])
    _err_word("ll")
    for n in ("y", "c_all", "act", "hprev"):
        _same(o[n].view, f["first"][n].view, "%s %s: two tiles of 16 rows against one block" % (lc.case_id(case), n))


@pytest.mark.parametrize("case", [(17, 3, 256, 0), (32, 5, 512, 0), (9, 5, 768, 0), (16, 3, 1024, 0)], ids=lc.case_id)
def test_ticket_forward_agrees_with_the_ll_forward_within_the_step_bounds(case):
    """ICKA_LSTM_TICKETS sums each gate's product in one chain, the LL kernel in four per-wave partial sums: the two need not be
    bitwise equal (the test prints whether they are), both must be inside the step bounds."""
    B, S, H, fl = case
    _skip_unless_reachable("fwd", B, H, fl)
    assert _skip_unless_reachable("fwd", B, H, lc.TICKETS)[0] == "ticket"
    f = _forward(case)
    whh, gx, _ = _inputs(B, S, H)
    o = _fwd_call(B, S, H, lc.TICKETS, _gin(gx), f["whh"])
    _err_word("ticket")
    lc.check_fwd("fwd ticket", f["gx"], f["whh"].view, o["y"].view, o["c_all"].view, o["act"].view, o["hprev"].view, B, S, H)
    ne = {n: int((_bits(o[n].view) != _bits(f["first"][n].view)).sum()) for n in ("y", "c_all", "act")}
    dmax = float((o["y"].view.float() - f["first"]["y"].view.float()).abs().max())
    print("\nLL_VS_TICKET %s elements that differ bitwise: %s; max |y_ticket - y_ll| = %.3g" % (lc.case_id(case), ne, dmax))
    kc.report("lstm_fwd tickets " + lc.case_id(case))


def test_case_list_reaches_every_instantiation():
    got = assert_dispatch_coverage()
    print("\n%d (kernel, template arguments, grid.z) combinations over %d cases" % (len(got), len(lc.CASES)))


# ------------------------------------------------------------------------------------------------ the module's wiring
def _lstm_node(fn):
    seen, stack = set(), [fn]
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if "_LstmFn" in type(n).__name__:
            return n
        stack.extend(f for f, _ in n.next_functions)
    raise AssertionError("no _LstmFn node behind the output")


@pytest.mark.parametrize("B,S,H", [(20, 3, 256), (40, 3, 64)])
def test_bilstm_gradients_are_the_products_of_the_saved_tensors(B, S, H):
    """BiLSTM's wiring round the recurrence: every parameter gradient and dx, element-wise against float64 products of the
    tensors the backward itself reads (x, hprev saved by the forward; dgates recomputed by icka_lstm_bwd under the same flags,
    bitwise reproducible by the tests above), after one backward (beta = 0) and after a second one without zero_grad
    (beta = 1: the accumulate path)."""
    from icka_amd import kernels as K
    from icka_amd.lstm import BiLSTM
    _skip_unless_reachable("fwd", B, H, 0)
    _skip_unless_reachable("bwd", B, H, 0)
    torch.manual_seed(B + H)
    m = BiLSTM(H, H).cuda()
    M = B * S
    x = (torch.randn(B, S, H) * 0.5).cuda().requires_grad_(True)
    w = (torch.randn(B, S, 2 * H) * 0.3).to(BF16).cuda()          # dy: exact in bf16
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    cat = lambda n: torch.cat((getattr(m, n).grad, getattr(m, n + "_reverse").grad), 0).clone()
    old = None
    for rep in (0, 1):
        x.grad = None
        out, _ = m(x)
        xs, c_all, act, hprev = _lstm_node(out.grad_fn).saved_tensors
        (out.float() * w.float()).sum().backward()
        A = m._arena()
        whh = A.w_cat((m.weight_hh_l0, m.weight_hh_l0_reverse))
        wih = A.w_cat((m.weight_ih_l0, m.weight_ih_l0_reverse))
        whh_t = K.transpose_bf16(whh, torch.empty(2 * H, 4 * H, dtype=BF16, device="cuda"), 2, 4 * H, H)
        assert torch.equal(whh_t.view(2, H, 4 * H), whh.view(2, 4 * H, H).transpose(1, 2))
        dg = torch.empty(M, 8 * H, dtype=BF16, device="cuda")
        K.lstm_bwd(w.reshape(M, 2 * H), whh_t, act, c_all, dg, torch.empty(2 * B, H, dtype=F32, device="cuda"), B, S, H,
                   flags=m.recurrence_flags)
        torch.cuda.synchronize()
        got = {n: cat(n) for n in names}
        d64, x64, h64 = dg.double(), xs.double(), hprev.double()
        ref = {"weight_ih_l0": (d64.t() @ x64, kc.gemm_acc_bound(d64.abs().t() @ x64.abs(), M))}
        r = [d64[:, d * 4 * H:(d + 1) * 4 * H].t() @ h64[:, d * H:(d + 1) * H] for d in (0, 1)]
        e = [d64[:, d * 4 * H:(d + 1) * 4 * H].abs().t() @ h64[:, d * H:(d + 1) * H].abs() for d in (0, 1)]
        ref["weight_hh_l0"] = (torch.cat(r, 0), kc.gemm_acc_bound(torch.cat(e, 0), M))
        ref["bias_ih_l0"] = ref["bias_hh_l0"] = (d64.sum(0), kc.gemm_acc_bound(d64.abs().sum(0), M))
        tag = "first backward" if rep == 0 else "accumulated"
        for n in names:
            rn, en = ref[n]
            if rep == 1:
                rn, en = kc.with_beta(en, rn, 1.0, old[n])
            kc.assert_within(got[n], rn, kc.stored(en, rn, F32), "d%s, %s" % (n, tag), verbose=False)
        rdx = d64 @ wih.double()
        edx = kc.gemm_acc_bound(d64.abs() @ wih.double().abs(), 8 * H)
        kc.assert_within(x.grad.reshape(M, H), rdx, kc.stored(edx, rdx, BF16), "dx, %s" % tag, verbose=False)
        old = got
    kc.report("bilstm_wiring B%d S%d H%d" % (B, S, H))
