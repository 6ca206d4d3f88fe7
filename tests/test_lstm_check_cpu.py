"""CPU: the step-wise LSTM bounds of tests/lstm_check.py hold for an honest emulation of one icka_lstm_fwd / icka_lstm_bwd call
in the kernels' arithmetic (f32, with h, act and dgates rounded to bf16 where the kernels store them, the four per-wave
partial sums of the LL forward and the bf16 partial tiles of the rs backward) and are MISSED by each seeded fault -- the proof
that tests/test_lstm_steps_gpu.py fails on a subtly wrong kernel.  A condition, not a measurement.

Where a fault cannot be seeded: "two batch rows of the second 16-row tile swapped" needs two live rows in that tile; (4, 6, 64)
has no second tile and (17, 3, 256) has one row in it, so that fault runs at (18, 3, 64).  The stale hand-off needs S >= 3 and
the dropped carry S >= 2: both shapes have them."""
import pytest
import torch

import kernel_check as kc
import lstm_check as lc
from kernel_check import BF16, F32

SHAPES = [(4, 6, 64), (17, 3, 256)]
FWD_FAULTS = ["stale_h", "k_tail", "swap_if", "rows", "hprev_shift", "rev_index"]
BWD_FAULTS = ["carry_drop", "rs_tile_drop"]


def _inputs(B, S, H, seed=0):
    g = torch.Generator().manual_seed(seed + B * 1000 + S * 10 + H)
    whh = (torch.randn(2, 4 * H, H, generator=g) * H ** -0.5).to(BF16)
    gx = torch.randn(B * S, 8 * H, generator=g) * 0.7
    dy = (torch.randn(B * S, 2 * H, generator=g) * 0.3).to(BF16)
    return whh, gx, dy


def emul_fwd(gx, whh, B, S, H, ll=False, fault=None):
    """One forward call -> (y, c_all, act, hprev) in the layouts of the kernels."""
    gx5 = gx.reshape(B, S, 2, 4 * H)
    W = whh.float()
    y = torch.zeros(B, S, 2, H, dtype=BF16)
    hprev = torch.zeros(B, S, 2, H, dtype=BF16)
    c_all = torch.zeros(B, S, 2, H, dtype=F32)
    act = torch.zeros(B, S, 2, 4, H, dtype=BF16)
    for d in (0, 1):
        hist = [torch.zeros(B, H, dtype=BF16)]          # hist[k]: h after k steps of this direction
        c = torch.zeros(B, H)
        for step in range(S):
            tt = step if d == 0 else S - 1 - step
            tg = step if (fault == "rev_index" and d == 1) else tt     # the reverse direction reads gx at the forward's index
            hin = hist[-1].float()
            if fault == "stale_h" and d == 0 and step == S - 1 and step >= 2:
                hin = hist[-2].float()                                 # h of step t-2: a stale hand-off word
            Wd = W[d]
            if fault == "k_tail":
                Wd = Wd.clone(); Wd[:, H - 32:] = 0                    # the last k-fragment dropped
            if fault == "rows" and step > 0:
                hin = hin.clone(); hin[[16, 17]] = hin[[17, 16]]       # two rows of the second tile swapped
            if ll:
                q = H // 4
                p = [hin[:, j * q:(j + 1) * q] @ Wd[:, j * q:(j + 1) * q].t() for j in range(4)]
                acc = (p[0] + p[1]) + (p[2] + p[3])
            else:
                acc = hin @ Wd.t()
            z = gx5[:, tg, d] + acc
            if fault == "swap_if":                                     # gate blocks i and f of units 16..31 swapped
                z = z.clone()
                zi = z[:, 16:32].clone()
                z[:, 16:32] = z[:, H + 16:H + 32]
                z[:, H + 16:H + 32] = zi
            i, f, g, o = z[:, :H].sigmoid(), z[:, H:2 * H].sigmoid(), z[:, 2 * H:3 * H].tanh(), z[:, 3 * H:].sigmoid()
            c = f * c + i * g
            h = (o * c.tanh()).to(BF16)
            y[:, tt, d], c_all[:, tt, d] = h, c
            act[:, tt, d] = torch.stack((i, f, g, o), 1).to(BF16)
            hprev[:, tt, d] = h if fault == "hprev_shift" else hist[-1]
            hist.append(h)
    return y, c_all, act, hprev


def emul_bwd(dy, whh, act, c_all, B, S, H, rs=False, fault=None):
    """One backward call -> (dgates [B, S, 2, 4, H] bf16, dc_carry [2, B, H] f32)."""
    W = whh.float()
    dy4 = dy.float().reshape(B, S, 2, H)
    dg = torch.zeros(B, S, 2, 4, H, dtype=BF16)
    carry_out = torch.zeros(2, B, H)
    for d in (0, 1):
        carry = torch.zeros(B, H)
        nxt = None
        for step in range(S - 1, -1, -1):
            tt = step if d == 0 else S - 1 - step
            tp = tt - 1 if d == 0 else tt + 1
            rec = torch.zeros(B, H)
            if nxt is not None:
                x = nxt.float().reshape(B, 4 * H)
                if rs:
                    for n in range(H // 16):                           # producer block n: its 4 x 16 gate columns
                        cols = torch.cat([torch.arange(q * H + 16 * n, q * H + 16 * n + 16) for q in range(4)])
                        if fault == "rs_tile_drop" and d == 0 and n == 1 and step == S - 2:
                            continue
                        rec = rec + (x[:, cols] @ W[d][cols]).to(BF16).float()
                else:
                    p = [x[:, q * H:(q + 1) * H] @ W[d][q * H:(q + 1) * H] for q in range(4)]
                    rec = p[0] + p[1] + p[2] + p[3]
            dh = dy4[:, tt, d] + rec
            i, f, g, o = act[:, tt, d].float().unbind(1)
            c = c_all[:, tt, d]
            cp = c_all[:, tp, d] if step > 0 else torch.zeros(B, H)
            tc = c.tanh()
            cin = torch.zeros(B, H) if (fault == "carry_drop" and d == 0 and step == S - 2) else carry
            dc = dh * o * (1 - tc * tc) + cin
            carry = dc * f
            nxt = torch.stack((dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), 1).to(BF16)
            dg[:, tt, d] = nxt
        carry_out[d] = carry
    return dg, carry_out


def _outside(out, ref, bound):
    return int((~((out.double() - ref).abs() <= bound)).sum())


def fwd_violations(gx, whh, y, c_all, act, hprev, B, S, H):
    r = lc.fwd_refs(gx, whh, y, c_all, B, S, H)
    v = {"y": _outside(y, *r["y"]), "c_all": _outside(c_all, *r["c_all"]), "act": _outside(act, *r["act"])}
    v["hprev"] = int((hprev.view(torch.int16) != r["hprev"].view(torch.int16)).sum())
    return v


def bwd_violations(dy, whh, act, c_all, dg, carry, B, S, H, rs):
    r = lc.bwd_refs(dy, whh, act, c_all, dg, B, S, H, rs=rs)
    v = {"dgates_" + q: _outside(dg[:, :, :, k], *r["dgates_" + q]) for k, q in enumerate(lc.GATES)}
    v["dc_carry"] = _outside(carry, *r["dc_carry"])
    return v


@pytest.mark.parametrize("ll", [False, True], ids=["one_chain", "ll_partial_sums"])
@pytest.mark.parametrize("B,S,H", SHAPES + [(18, 3, 64)])
def test_forward_emulation_is_inside_every_bound_and_every_fault_is_outside_one(B, S, H, ll):
    whh, gx, _ = _inputs(B, S, H)
    y, c_all, act, hprev = emul_fwd(gx, whh, B, S, H, ll=ll)
    assert float(act.float().abs().max()) < 0.9995, "saturated gates: the faults would hide in the flat part of the sigmoid"
    name = "cpu lstm fwd %s B%d S%d H%d" % ("ll" if ll else "chain", B, S, H)
    lc.check_fwd(name, gx, whh, y, c_all, act, hprev, B, S, H)
    v = fwd_violations(gx, whh, y, c_all, act, hprev, B, S, H)
    assert not any(v.values()), "honest emulation outside a bound: %s" % v
    kc.report(name)
    for fault in FWD_FAULTS:
        if fault == "rows" and B < 18:
            continue                    # no two live rows in a second tile (module docstring)
        out = emul_fwd(gx, whh, B, S, H, ll=ll, fault=fault)
        v = fwd_violations(gx, whh, *out, B, S, H)
        assert any(v.values()), "fault %s at (%d, %d, %d) stays inside every bound (y, c_all, act, hprev): %s" % (fault, B, S, H, v)
        want = "hprev" if fault == "hprev_shift" else "act"
        assert v[want] > 0, "fault %s: quantity %s did not leave its bound: %s" % (fault, want, v)
        print("fault %-12s outside: %s" % (fault, v))


@pytest.mark.parametrize("rs", [False, True], ids=["one_product", "rs_partial_tiles"])
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_backward_emulation_is_inside_every_bound_and_every_fault_is_outside_one(B, S, H, rs):
    whh, gx, dy = _inputs(B, S, H)
    y, c_all, act, _ = emul_fwd(gx, whh, B, S, H)
    dg, carry = emul_bwd(dy, whh, act, c_all, B, S, H, rs=rs)
    name = "cpu lstm bwd %s B%d S%d H%d" % ("rs" if rs else "product", B, S, H)
    lc.check_bwd(name, dy, whh, act, c_all, dg, carry, B, S, H, rs=rs)
    v = bwd_violations(dy, whh, act, c_all, dg, carry, B, S, H, rs)
    assert not any(v.values()), "honest emulation outside a bound: %s" % v
    kc.report(name)
    # the rs bound is the wider one (bf16 partial tiles); it must still be MISSED by the plain kernel's faults, and the plain
    # bound must be missed by ... the rs arithmetic itself, or the 2^-8 sum |P_n| term would be slack
    if rs:
        vv = bwd_violations(dy, whh, act, c_all, dg, carry, B, S, H, False)
        assert any(vv.values()), "the bf16 partial tiles stay inside the bound of the f32 product: %s" % vv
    for fault in BWD_FAULTS:
        if fault == "rs_tile_drop" and not rs:
            continue
        out = emul_bwd(dy, whh, act, c_all, B, S, H, rs=rs, fault=fault)
        v = bwd_violations(dy, whh, act, c_all, *out, B, S, H, rs)
        assert any(v.values()), "fault %s at (%d, %d, %d) stays inside every dgates bound: %s" % (fault, B, S, H, v)
        want = "dgates_o" if fault == "rs_tile_drop" else "dgates_g"
        assert v[want] > 0, "fault %s: quantity %s did not leave its bound: %s" % (fault, want, v)
        print("fault %-12s outside: %s" % (fault, v))


def test_case_list_reaches_every_instantiation_lstm_hip_launches():
    """The dispatch-coverage assertion of tests/test_lstm_steps_gpu.py, run here too: a case list that misses an instantiation
    fails without a GPU."""
    import test_lstm_steps_gpu as G
    got = G.assert_dispatch_coverage()
    assert len({(n, t) for n, t, z in got}) == 26
    with pytest.raises(AssertionError, match="never launched"):
        lc.assert_dispatch_coverage([c for c in lc.CASES if not (c[3] & lc.NO_BATCH_SPLIT)])


def test_dispatch_on_a_partitioned_device_takes_other_forms():
    assert lc.dispatch("fwd", 32, 1024, 0, cus=256) == ("ll", "lstm_fwd_ll_kernel", (1, 8), 2)
    assert lc.dispatch("fwd", 32, 1024, 0, cus=128) == ("ll", "lstm_fwd_ll_kernel", (2, 8), 1)
    assert lc.dispatch("fwd", 32, 1024, 0, cus=64)[0] == "step"
    assert lc.dispatch("bwd", 32, 1024, 0, cus=128) == ("ticket", "lstm_bwd_persistent_kernel", (2, 32), 1)
    assert lc.dispatch("bwd", 17, 384, 0) == ("ticket", "lstm_bwd_persistent_kernel", (2, 24), 1)
    assert lc.dispatch("fwd", 17, 1056, 0) == ("step", "lstm_fwd_step_kernel", (2, 24), 1)
