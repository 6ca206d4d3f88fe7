"""Helpers of the step-wise LSTM kernel tests (no test functions): a TEACHER-FORCED float64 reference of every time step of
icka_lstm_fwd / icka_lstm_bwd, error bounds derived from the number formats (the builders of tests/kernel_check.py; no fitted
constant), a restatement of the host dispatch of csrc/lstm.hip and the case list that reaches every instantiation.

Why step-wise.  A recurrence compared end to end needs a tolerance that grows with S.  Here step t is recomputed in float64
from what the kernel itself stored for step t-1 (y: exact bf16 = the operand the kernel read; c_all: exact f32 = the value
the kernel kept in its register), so one step's roundings are all that separates the two, and the bound does not depend on
S.  By induction from the zero initial state a call that is inside the bound at every step is right as a whole.

Layouts (include/icka_hip.h): gates_x f32 [B*S, ld >= 8H], column = dir*4H + gate*H + unit (gates i, f, g, o); W_hh bf16
[2][4H][H]; y / hprev bf16 [B, S, 2, H]; c_all f32 [B, S, 2, H]; act bf16 [B, S, 2, 4, H]; dgates bf16 [B*S, ld >= 8H] with
the columns of gates_x; dc_carry f32 [2, B, H].  Direction 1 walks the time index downwards: its "previous" step is t + 1.
"""
import os
import re

import torch

import kernel_check as kc
from kernel_check import BF16, EPS, F32, LIP_SIGMOID, SIGMOID_ABS, TANH_ABS, TINY, U_ACC, gemm_acc_bound, stored

PER_STEP, TICKETS, NO_BATCH_SPLIT = 1, 2, 4     # ICKA_LSTM_* (include/icka_hip.h)
GATES = "ifgo"


def shift_prev(x, d):
    """x [B, S, ...] -> its value at the PREVIOUS step of direction d (t - 1 forward, t + 1 reverse); zero at the first."""
    out = torch.zeros_like(x)
    if x.shape[1] > 1:
        if d == 0:
            out[:, 1:] = x[:, :-1]
        else:
            out[:, :-1] = x[:, 1:]
    return out


def shift_next(x, d):
    """... at the NEXT step of direction d; zero at the direction's last step."""
    return shift_prev(x, 1 - d)


# ---------------------------------------------------------------------------------------------------------- forward
def fwd_refs(gx, whh, y, c_all, B, S, H):
    """-> {"y", "c_all", "act": (float64 reference, bound)} of every step, and "hprev": the tensor hprev must equal bitwise.

    Inputs of step t, all exact: h' = y[t-1] (bf16), c' = c_all[t-1] (f32), gx[t] (f32), W_hh (bf16); zero state at the
    direction's first step.  With u = U_ACC, eps = 2^-8:
      z_q   = gx_q + sum_k h'_k W_qk     E_z = (H + 4) u (sum_k |h'_k||W_qk| + |gx_q|)          (gemm_acc_bound, K = H)
              The bound holds for a length-H f32 sum in ANY order, so it covers each kernel's summation form: one MFMA chain
              per gate (per-step and ticket kernels; the per-step kernels in blocks of UB fragments) and, in the LL kernel,
              four per-wave partial sums over H/4 each, added as (p0 + p1) + (p2 + p3) and then to gx: the H - 1 additions of
              the bound are the H - 4 inside the waves, the 3 that join them, and the +4 pays the add of gx.
      i,f,o = sigmoid(z)                 e = E_z / 4 + 2^-12      (LIP_SIGMOID, SIGMOID_ABS: the requirement on the device
      g     = tanh(z)                    e = E_z + 2^-12           function, as in the GATE / TANH epilogues of the GEMM)
      act   = bf16(i, f, g, o)           stored(e, ., bf16)
      c     = f c' + i g                 e_c = |c'| e_f + |g| e_i + |i| e_g + e_i e_g + 2 u (|f c'| + |i g|)
              (two products and one add in f32, or one product and one fma: at most u per product and u |c| <= u (|f c'| +
              |i g|) for the add); c_all holds that f32 value: stored(e_c, c, f32)
      h     = o tanh(c)                  e_h = |tanh c| e_o + |o| (e_c + 2^-12) + e_o (e_c + 2^-12) + u |h|
      y     = bf16(h)                    stored(e_h, h, bf16)
    A batch row or a unit the kernel leaves out keeps the NaN the test put there and fails ``assert_within``."""
    gx64 = gx.double().reshape(B, S, 2, 4, H)
    W = whh.double().reshape(2, 4, H, H)
    y64 = y.double().reshape(B, S, 2, H)
    c64 = c_all.double().reshape(B, S, 2, H)
    r_act, b_act, r_c, b_c, r_y, b_y = [], [], [], [], [], []
    for d in (0, 1):
        hp, cp = shift_prev(y64[:, :, d], d), shift_prev(c64[:, :, d], d)
        z = gx64[:, :, d] + torch.einsum("bsk,quk->bsqu", hp, W[d])
        Ez = gemm_acc_bound(torch.einsum("bsk,quk->bsqu", hp.abs(), W[d].abs()), H, bias=gx64[:, :, d])
        a = torch.sigmoid(z)
        a[:, :, 2] = torch.tanh(z[:, :, 2])
        ea = LIP_SIGMOID * Ez + SIGMOID_ABS
        ea[:, :, 2] = Ez[:, :, 2] + TANH_ABS
        i, f, g, o = a.unbind(2)
        ei, ef, eg, eo = ea.unbind(2)
        c = f * cp + i * g
        ec = cp.abs() * ef + g.abs() * ei + i.abs() * eg + ei * eg + 2 * U_ACC * ((f * cp).abs() + (i * g).abs())
        tc = torch.tanh(c)
        etc = ec + TANH_ABS
        h = o * tc
        eh = tc.abs() * eo + o.abs() * etc + eo * etc + U_ACC * h.abs()
        r_act.append(a); b_act.append(stored(ea, a, BF16))
        r_c.append(c); b_c.append(stored(ec, c, F32))
        r_y.append(h); b_y.append(stored(eh, h, BF16))
    st = lambda xs: torch.stack(xs, 2)
    hprev = torch.stack([shift_prev(y.reshape(B, S, 2, H)[:, :, d], d) for d in (0, 1)], 2)
    return {"act": (st(r_act), st(b_act)), "c_all": (st(r_c), st(b_c)), "y": (st(r_y), st(b_y)), "hprev": hprev}


# --------------------------------------------------------------------------------------------------------- backward
def bwd_refs(dy, whh, act, c_all, dgates, B, S, H, rs=False):
    """-> {"dgates_i", "dgates_f", "dgates_g", "dgates_o": (reference [B, S, 2, H], bound), "dc_carry": (.. [2, B, H], ..)}.

    Inputs of step t, all exact: dy[t] (bf16), the stored act[t] = (i, f, g, o) (bf16), c_all[t] and c' = c_all[t-1] (f32),
    and the kernel's OWN stored bf16 dgates of the next step for the recurrent product.  The carry dc_{t+1} f_{t+1} is the one
    internal state the kernels never store (the per-step kernels pass it on through dc_carry in f32, which is exact), so it
    is a float64 chain over the steps here, built from the teacher-forced dh, with a bound that is a recursion:
      dh    = dy + sum_{k < 4H} dgates'_k W_k       per-step and ticket kernels: E_dh = (4H + 4) u (sum |dgates'_k||W_k| + |dy|)
              (gemm_acc_bound, K = 4H: four per-wave chains over H each, added in f32)
              rs kernel: the producer block n multiplies its 64 gate columns, P_n = f32 MFMA over K = 64, ROUNDS the tile to
              bf16, and the owner adds the H/16 tiles and dy in f32:
                  E_dh = sum_n stored((64 + 4) u absP_n, P_n, bf16) + (H/16 + 4) u (sum_n (|P_n| + e_n) + |dy|)
              i.e. 2^-8 sum_n |P_n| plus the f32 adds (tests/test_lstm_rs_cpu.py states the algebra)
      tc    = tanh(c)                               e_tc = 2^-12 (c is read exactly)
      s     = 1 - tc^2  (f32, never stored)         e_s = 2 |tc| e_tc + e_tc^2 + 2 u
      a     = dh o s                                e_a = |o s| E_dh + |dh o| e_s + |o| E_dh e_s + 2 u |a|
      dc    = a + carry                             e_dc = e_a + e_carry + u (|a| + |carry|)
      carry' = dc f  (to the step before)           e_carry' = |f| e_dc + u |dc f|: contracted by |f| < 1 at every step
      dgates: di = dc g i (1 - i),  df = dc c' f (1 - f),  dg = dc i (1 - g^2): |factor| e_dc + 4 u |.| (four f32 operations
              on exact bf16 / f32 factors), do = dh tc o (1 - o): |tc o (1 - o)| E_dh + |dh o (1 - o)| e_tc + |o (1 - o)| E_dh
              e_tc + 4 u |do|; each stored in bf16: stored(., ., bf16)
      dc_carry (per-step kernels only): the carry' of the direction's first step, stored(e_carry', ., f32)."""
    dy64 = dy.double().reshape(B, S, 2, H)
    a64 = act.double().reshape(B, S, 2, 4, H)
    c64 = c_all.double().reshape(B, S, 2, H)
    dg64 = dgates.double().reshape(B, S, 2, 4, H)
    W = whh.double().reshape(2, 4, H, H)
    ref = {q: [] for q in GATES}
    bnd = {q: [] for q in GATES}
    r_carry, b_carry = [], []
    for d in (0, 1):
        dgn = shift_next(dg64[:, :, d], d)
        prod = torch.einsum("bsqu,quk->bsk", dgn, W[d])
        absprod = torch.einsum("bsqu,quk->bsk", dgn.abs(), W[d].abs())
        if rs:
            nb = H // 16
            P = torch.einsum("bsqnu,qnuk->bsnk", dgn.reshape(B, S, 4, nb, 16), W[d].reshape(4, nb, 16, H))
            e_tiles = gemm_acc_bound(absprod, 64) + EPS[BF16] * (P.abs().sum(2) + gemm_acc_bound(absprod, 64)) + nb * TINY[BF16]
            Edh = e_tiles + gemm_acc_bound(P.abs().sum(2) + e_tiles, nb, bias=dy64[:, :, d])
            del P
        else:
            Edh = gemm_acc_bound(absprod, 4 * H, bias=dy64[:, :, d])
        dh = dy64[:, :, d] + prod
        i, f, g, o = a64[:, :, d].unbind(2)
        cp = shift_prev(c64[:, :, d], d)
        tc = torch.tanh(c64[:, :, d])
        etc = TANH_ABS
        s = 1 - tc * tc
        es = 2 * tc.abs() * etc + etc * etc + 2 * U_ACC
        a = dh * o * s
        ea = (o * s).abs() * Edh + (dh * o).abs() * es + o.abs() * Edh * es + 2 * U_ACC * a.abs()
        dc, edc = torch.zeros_like(a), torch.zeros_like(a)
        carry, ecarry = torch.zeros_like(a[:, 0]), torch.zeros_like(a[:, 0])
        for tt in (range(S - 1, -1, -1) if d == 0 else range(S)):      # the order the backward walks direction d
            dc[:, tt] = a[:, tt] + carry
            edc[:, tt] = ea[:, tt] + ecarry + U_ACC * (a[:, tt].abs() + carry.abs())
            carry = dc[:, tt] * f[:, tt]
            ecarry = f[:, tt].abs() * edc[:, tt] + U_ACC * carry.abs()
        r_carry.append(carry); b_carry.append(stored(ecarry, carry, F32))
        fac = {"i": g * i * (1 - i), "f": cp * f * (1 - f), "g": i * (1 - g * g)}
        for q in "ifg":
            v = dc * fac[q]
            ref[q].append(v); bnd[q].append(stored(fac[q].abs() * edc + 4 * U_ACC * v.abs(), v, BF16))
        oo = o * (1 - o)
        v = dh * tc * oo
        e = (tc * oo).abs() * Edh + (dh * oo).abs() * etc + oo.abs() * Edh * etc + 4 * U_ACC * v.abs()
        ref["o"].append(v); bnd["o"].append(stored(e, v, BF16))
    out = {"dgates_" + q: (torch.stack(ref[q], 2), torch.stack(bnd[q], 2)) for q in GATES}
    out["dc_carry"] = (torch.stack(r_carry, 0), torch.stack(b_carry, 0))
    return out


def check_fwd(test, gx, whh, y, c_all, act, hprev, B, S, H):
    """Every stored quantity of a forward call against ``fwd_refs`` (records the ratios for ``kc.report``)."""
    r = fwd_refs(gx, whh, y, c_all, B, S, H)
    kc.assert_within(act.reshape(B, S, 2, 4, H), *r["act"], "%s act" % test, verbose=False)
    kc.assert_within(c_all.reshape(B, S, 2, H), *r["c_all"], "%s c_all" % test, verbose=False)
    kc.assert_within(y.reshape(B, S, 2, H), *r["y"], "%s y" % test, verbose=False)
    if hprev is not None:
        same = hprev.reshape(B, S, 2, H).view(torch.int16) == r["hprev"].view(torch.int16)
        assert bool(same.all()), "%s hprev: %d elements are not bitwise y of the previous step (+0 at the first)" % (
            test, int((~same).sum()))


def check_bwd(test, dy, whh, act, c_all, dgates, dc_carry, B, S, H, rs=False):
    r = bwd_refs(dy, whh, act, c_all, dgates, B, S, H, rs=rs)
    dg = dgates.reshape(B, S, 2, 4, H)
    for k, q in enumerate(GATES):
        kc.assert_within(dg[:, :, :, k], *r["dgates_" + q], "%s dgates_%s" % (test, q), verbose=False)
    if dc_carry is not None:
        kc.assert_within(dc_carry.reshape(2, B, H), *r["dc_carry"], "%s dc_carry" % test, verbose=False)


# --------------------------------------------------------------------------------------------------------- dispatch
WHOLE_DEVICE_CUS = 256
LL_MAXH = 1024


def dispatch(phase, B, H, flags=0, cus=WHOLE_DEVICE_CUS):
    """The host dispatch of icka_lstm_fwd / icka_lstm_bwd (csrc/lstm.hip) restated: -> (form, kernel, template arguments,
    grid.z) for ``cus`` = CUs of the device minus the reserved ones.  form: "ll" / "rs" / "ticket" / "step"."""
    persistent, handoff, bsplit = not flags & PER_STEP, not flags & TICKETS, not flags & NO_BATCH_SPLIT
    nrt = (B + 15) // 16
    blocks = (H // 16) * 2
    if phase == "fwd":
        if persistent and handoff and nrt <= 2 and H <= LL_MAXH and H % 128 == 0 and blocks <= cus and H // 128 in (2, 4, 6, 8):
            split = bsplit and nrt == 2 and blocks * 2 <= cus
            return "ll", "lstm_fwd_ll_kernel", (1 if split else nrt, H // 128), 2 if split else 1
    else:
        if persistent and handoff and nrt <= 2 and H <= LL_MAXH and H % 256 == 0 and blocks * nrt <= cus:
            return "rs", "lstm_bwd_rs_kernel", (H // 64,), nrt
    if persistent and nrt <= 2 and H <= 1024 and blocks <= cus:
        return "ticket", "lstm_%s_persistent_kernel" % phase, (nrt, 32 if H > 768 else 24), 1
    return "step", "lstm_%s_step_kernel" % phase, {1: (1, 24), 2: (2, 24)}.get(nrt, (4, 8)), 1


# (B, S, H, flags): the smallest shapes that reach each path.  S <= 6; S = 1 has no hand-off and first == last in the backward,
# S = 2 uses one parity buffer only; B = 1, 16, 17, 32, 33, 48, 49, 64 are a full last tile / a tile with one live row.
CASES = [
    # LL forward (rs backward)
    (1, 1, 256, 0), (16, 2, 256, 0), (17, 3, 256, 0), (32, 5, 512, 0), (9, 5, 768, 0), (16, 3, 1024, 0), (32, 3, 1024, 0),
    (32, 3, 256, NO_BATCH_SPLIT), (17, 5, 512, NO_BATCH_SPLIT), (31, 3, 768, NO_BATCH_SPLIT), (17, 3, 1024, NO_BATCH_SPLIT),
    (16, 4, 512, 0),                    # LL<1, 4> and rs<8> with grid.z = 1 (the shapes above reach them with two batch tiles)
    (20, 3, 768, 0),                    # LL<1, 6> and rs<12> with grid.z = 2
    # ticket form: H % 128 != 0 / H % 256 != 0 with the default flags, any H <= 1024 with TICKETS
    (3, 5, 32, 0), (17, 3, 128, 0), (20, 5, 384, 0), (1, 2, 896, 0), (32, 3, 896, 0), (5, 3, 768, TICKETS), (17, 3, 1024, TICKETS),
    # per-step form: the flag, H > 1024, B > 32
    (1, 1, 32, PER_STEP), (16, 3, 1056, 0), (17, 3, 1056, 0), (33, 3, 288, 0), (48, 2, 64, 0), (49, 3, 288, 0), (64, 3, 512, 0),
]


def case_id(c):
    B, S, H, fl = c
    return "B%d-S%d-H%d%s" % (B, S, H, "".join("-" + n for n, b in (("per_step", PER_STEP), ("tickets", TICKETS), (
        "no_batch_split", NO_BATCH_SPLIT)) if fl & b))


_LSTM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "icka_amd", "csrc", "lstm.hip")


def launched_instantiations(path=_LSTM_HIP):
    """Every recurrence-kernel instantiation the host code of lstm.hip launches: {(kernel, template arguments)}."""
    src = open(path).read()
    src = src[src.index('extern "C" int icka_lstm_fwd'):]
    out = set()
    for name, targs in re.findall(r"hipLaunchKernelGGL\(\((lstm_\w+_kernel)<([0-9, ]+)>\)", src):
        out.add((name, tuple(int(v) for v in targs.split(","))))
    for targs in re.findall(r"ICKA_LL_FWD\((\d+), (\d+)\);", src):
        out.add(("lstm_fwd_ll_kernel", tuple(int(v) for v in targs)))
    return out


def assert_dispatch_coverage(cases=CASES):
    """The union over the case list (whole device) is every instantiation lstm.hip launches, the batch-tiled kernels with
    grid.z = 1 and with grid.z = 2.  A pure function of the case list and the source text."""
    got = set()
    for B, S, H, fl in cases:
        for phase in ("fwd", "bwd"):
            got.add(dispatch(phase, B, H, fl)[1:])
    want = launched_instantiations()
    assert len(want) == 26, sorted(want)          # 3 + 3 per-step, 4 + 4 ticket, 8 LL, 4 rs
    have = {(n, t) for n, t, z in got}
    assert have == want, "never launched: %s; not in lstm.hip: %s" % (sorted(want - have), sorted(have - want))
    for n, t in sorted(want):
        if n == "lstm_bwd_rs_kernel" or (n == "lstm_fwd_ll_kernel" and t[0] == 1):
            for z in (1, 2):
                assert (n, t, z) in got, "%s<%s> never runs with grid.z = %d" % (n, t, z)
    return got
