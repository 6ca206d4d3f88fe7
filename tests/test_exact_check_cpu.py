"""CPU: keeps tests/exact_check.py honest.  For every fp32-exact kernel a plain torch-f32 emulation performs the kernel's
operations in the kernel's structure (per-lane partial sums with stride 64 and the wave tree, the four row phases of the
column sum, torch's f32 math functions); at every shape tests/test_exact_elements_gpu.py runs on the device it must stay
inside every bound.  Then seeded faults, one at a time, at those same shapes: each must leave a bound or break a bitwise
check -- a fault that stays inside means the shapes or the bound are too weak to trust the GPU test."""
import pytest
import torch

import exact_check as xc
from exact_check import F32

SEED = 0x1234_5678_9abc
NAN = float("nan")


# ---------------------------------------------------------------------------------------- the kernels' summation forms
def wave_sum(v):
    """wave_sum of csrc/common.h on [rows, 64]: four rotations inside the rows of 16 lanes, then (r0 + r1) + (r2 + r3)"""
    v = v.reshape(-1, 4, 16)
    for s in (8, 4, 2, 1):
        v = v + torch.roll(v, -s, 2)
    r = v[:, :, 0]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def strided_sum(t, lanes=64):
    """[rows, n] -> [rows, lanes]: the partial sum of every lane, elements lane, lane + lanes, ... added in that order"""
    rows, n = t.shape
    trips = -(-n // lanes)
    pad = torch.zeros(rows, trips * lanes, dtype=F32)
    pad[:, :n] = t
    acc = torch.zeros(rows, lanes, dtype=F32)
    for i in range(trips):
        acc = acc + pad[:, i * lanes:(i + 1) * lanes]
    return acc


def lane_sum(t):
    return wave_sum(strided_sum(t))


def caught(fn):
    """the check fails (a bound is left or a bitwise comparison breaks)"""
    try:
        fn()
    except AssertionError:
        xc.report("(seeded fault)")
        return True
    xc.report("(seeded fault)")
    return False


# ------------------------------------------------------------------------------------------------------- LayerNorm
def emu_ln_core(v, gamma, beta, eps, fault=None):
    H = v.shape[1]
    mean = (lane_sum(v[:, :64]) if fault == "mean64" else lane_sum(v)) / H
    d = v - mean[:, None]
    rs = 1.0 / torch.sqrt(lane_sum(d * d) / (H - 1 if fault == "var_hm1" else H) + eps)
    xh = d * rs[:, None]
    return {"y": xh * gamma + beta, "xhat": xh, "rstd": rs}


def emu_ln_fwd(x, m, res, gamma, beta, eps, fault=None):
    v = x * m
    if res is not None:
        v = v + res
    return emu_ln_core(v, gamma, beta, eps, fault)


def emu_ln_bwd(dy, xhat, rstd, gamma, m, fault=None):
    H = dy.shape[1]
    gv = dy * gamma
    s1, s2 = lane_sum(gv) / H, lane_sum(gv * xhat) / H
    inner = gv - s1[:, None] - (0 if fault == "no_c2" else xhat * s2[:, None])
    v = rstd[:, None] * inner
    return {"dpre": v, "ddense": v * m}


def _ln_check(M, H, p, fwd_fault=None, bwd_fault=None, mean100=False):
    x, r, gamma, beta, dy, z = xc.ln_inputs(M, H, mean100)
    m = xc.cpu_dropout_mask(M * H, p, SEED).reshape(M, H)
    res = None if mean100 else r
    o = emu_ln_fwd(x, m, res, gamma, beta, xc.EPS_LN, fwd_fault)
    xc.compare(o, xc.ln_fwd_refs(x, m, res, gamma, beta, xc.EPS_LN), "ln_fwd")
    if z is not None:
        xc.same_bits(o["y"][z], beta, "all-zero row")
    ob = emu_ln_bwd(dy, o["xhat"], o["rstd"], gamma, m, bwd_fault)
    xc.compare(ob, xc.ln_bwd_refs(dy, o["xhat"], o["rstd"], gamma, m), "ln_bwd")


def test_layernorm_emulation_inside_and_faults_outside():
    for M in xc.LN_M:
        for H in xc.ROW_H:
            for p in xc.P_DROP:
                _ln_check(M, H, p)
            if H > 1:
                assert caught(lambda: _ln_check(M, H, 0.0, fwd_fault="var_hm1")), ("variance over H - 1", M, H)
                assert caught(lambda: _ln_check(M, H, 0.1, bwd_fault="no_c2")), ("xhat c2 dropped", M, H)
            if H > 64:
                assert caught(lambda: _ln_check(M, H, 0.0, fwd_fault="mean64")), ("mean over 64 columns", M, H)
    _ln_check(5, 200, 0.0, mean100=True)
    assert caught(lambda: _ln_check(5, 200, 0.0, fwd_fault="var_hm1", mean100=True))
    xc.report("cpu layernorm")


# ------------------------------------------------------------------------------------------------------ column sum
def emu_colsum(a, b, accumulate, prefill, fault=None):
    M, N = a.shape
    t = a if b is None else a * b
    pad = torch.zeros(-(-M // 4) * 4, N, dtype=F32)
    pad[:M] = t
    ph = torch.zeros(4, N, dtype=F32)
    for i in range(pad.shape[0] // 4):
        ph = ph + pad[4 * i:4 * i + 4]
    if fault == "skip_phase":
        ph[3] = 0.0
    s = (ph[0] + ph[1]) + (ph[2] + ph[3])
    return {"out": prefill + s if accumulate and fault != "ignore_accumulate" else s}


def _colsum_check(M, N, with_b, acc, fault=None):
    a, b = xc.rnd(M, N, seed=1), (xc.rnd(M, N, seed=2) if with_b else None)
    pre = torch.full((N,), 0.5)
    xc.compare(emu_colsum(a, b, acc, pre, fault), xc.colsum_refs(a, b, acc, pre), "colsum")


def test_colsum_emulation_inside_and_faults_outside():
    for M in xc.COLSUM_M:
        for N in xc.COLSUM_N:
            for with_b in (False, True):
                for acc in (0, 1):
                    _colsum_check(M, N, with_b, acc)
                assert caught(lambda: _colsum_check(M, N, with_b, 1, "ignore_accumulate")), ("accumulate ignored", M, N)
                if M >= 4:
                    assert caught(lambda: _colsum_check(M, N, with_b, 0, "skip_phase")), ("last row phase skipped", M, N)
    xc.report("cpu colsum")


# ------------------------------------------------------------------------------------------------------ embeddings
def _tables(H, vocab, types, max_pos):
    return xc.rnd(vocab, H, seed=21), xc.rnd(max_pos, H, seed=22), xc.rnd(types, H, seed=23)


def emu_scatter(table, index, g, skip=None):
    for r in range(g.shape[0]):               # one row after the other: one of the orders the atomics may take
        if skip is None or int(index[r]) != skip:
            table[int(index[r])] += g[r]
    return table


def _embed_check(H, with_tt, fwd_fault=None, sc_fault=None):
    e = xc.EMBED
    B, S = e["B"], e["S"]
    ids = xc.embed_ids(B, S, e["vocab"])
    tt = (torch.arange(B * S).reshape(B, S) % 2) if with_tt else None
    word, pos, typ = _tables(H, e["vocab"], e["types"], e["max_pos"])
    gamma, beta = xc.rnd(H, seed=4) + 1.0, xc.rnd(H, seed=5)
    wi, pi, ti = xc.embed_rows(ids, tt, S)
    if fwd_fault == "pos_div":
        pi = torch.arange(B * S) // S
    o = emu_ln_core((word[wi] + pos[pi]) + typ[ti], gamma, beta, xc.EPS_LN)
    xc.compare(o, xc.embed_fwd_refs(ids, tt, word, pos, typ, gamma, beta, S, xc.EPS_LN), "embed_fwd")
    dpre = xc.rnd(B * S, H, seed=6)
    wi, pi, ti = xc.embed_rows(ids, tt, S)
    sizes = (e["vocab"], e["max_pos"], e["types"])
    out = {"dword": emu_scatter(torch.full((sizes[0], H), 0.5), wi, dpre, None if sc_fault == "pad_row" else e["padding_idx"]),
           "dpos": emu_scatter(torch.full((sizes[1], H), 0.5), pi, dpre), "dtyp": emu_scatter(torch.full((sizes[2], H), 0.5), ti, dpre)}
    xc.compare(out, xc.embed_scatter_refs(dpre, ids, tt, S, sizes, e["padding_idx"], 0.5), "embed_scatter")
    xc.same_bits(out["dword"][e["padding_idx"]], torch.full((H,), 0.5), "padding row")


def emu_prompt(H, pos_offset, sc_fault=None):
    c = xc.PROMPT
    B, S_in, S, P = c["B"], c["S_in"], c["S"], c["P"]
    ids = xc.embed_ids(B, S_in, c["vocab"])
    src = torch.tensor(c["src"], dtype=torch.int32)
    word, pos, typ = _tables(H, c["vocab"], 2, c["max_pos"])
    prompt = xc.rnd(B, P, H, seed=24)
    gamma, beta = xc.rnd(H, seed=4) + 1.0, xc.rnd(H, seed=5)
    isp, wid, prow, prw = xc.prompt_rows(ids, src, B, S_in, S, P, pos_offset)
    x = torch.where(isp[:, None], prompt.reshape(B * P, H)[prow], word[wid])
    o = emu_ln_core((x + pos[prw]) + typ[0], gamma, beta, xc.EPS_LN)
    xc.compare(o, xc.prompt_fwd_refs(ids, src, prompt, word, pos, typ, gamma, beta, B, S_in, S, P, pos_offset, xc.EPS_LN),
               "prompt_fwd")
    dpre = xc.rnd(B * S, H, seed=6)
    sizes = (c["vocab"], c["max_pos"], 2)
    refs = xc.prompt_scatter_refs(dpre, ids, src, B, S_in, S, P, pos_offset, sizes, c["padding_idx"], 0.5)
    dprompt = torch.full((B * P, H), NAN)
    dprompt[prow[isp]] = dpre[isp]
    out = {"dword": emu_scatter(torch.full((sizes[0], H), 0.5), wid[~isp], dpre[~isp], c["padding_idx"]),
           "dpos": emu_scatter(torch.full((sizes[1], H), 0.5), prw - (pos_offset if sc_fault == "no_pos_offset" else 0), dpre),
           "dtyp": emu_scatter(torch.full((sizes[2], H), 0.5), torch.zeros(B * S, dtype=torch.long), dpre)}
    xc.compare(out, refs, "prompt_scatter")
    assert bool((refs["dprompt_source"] >= 0).all())
    xc.same_bits(dprompt, dpre[refs["dprompt_source"]], "dprompt")
    xc.same_bits(out["dword"][c["padding_idx"]], torch.full((H,), 0.5), "padding row")


def test_embedding_emulations_inside_and_faults_outside():
    for H in xc.ROW_H:
        for with_tt in (False, True):
            _embed_check(H, with_tt)
        assert caught(lambda: _embed_check(H, True, sc_fault="pad_row")), ("padding row receives gradient", H)
        if H > 1:          # (H = 1: every LayerNorm output is beta whatever the input row)
            assert caught(lambda: _embed_check(H, True, fwd_fault="pos_div")), ("position row // S", H)
        for off in xc.PROMPT["pos_offsets"]:
            emu_prompt(H, off)
        assert caught(lambda: emu_prompt(H, 4, sc_fault="no_pos_offset")), ("pos_offset ignored", H)
    xc.report("cpu embeddings")


# --------------------------------------------------------------------------------------------------------- softmax
def emu_softmax_fwd(P0, mask, m, scale, rpb, Sq, fault=None):
    rows, Skv = P0.shape
    B = mask.shape[0]
    r = torch.arange(rows)
    mk = mask[(r // Sq).clamp_max(B - 1) if fault == "mask_row" else r // rpb]
    z = P0 * scale + mk
    mx = z.amax(-1, keepdim=True)
    e = torch.exp(z - mx)
    p = e / lane_sum(e)[:, None]
    return {"P": p, "Pd": p * m}


def emu_softmax_bwd(P, dPd, m, scale, fault=None):
    dp = dPd * m
    dot = lane_sum(dp * P)[:, None]
    return {"dS": P * (dp - dot) * (1.0 if fault == "no_scale" else scale)}


def _softmax_check(Skv, scale, p, kind="tail", fwd_fault=None, bwd_fault=None):
    c = xc.SOFTMAX
    B, heads, Sq = c["B"], c["heads"], c["Sq"]
    rows = B * heads * Sq
    P0, mask = xc.rnd(rows, Skv, seed=1, scale=2.0), xc.softmax_mask(Skv, kind)
    m = xc.cpu_attn_dropout_mask(rows, Skv, p, SEED)
    m_used = xc.cpu_dropout_mask(rows * Skv, p, SEED).reshape(rows, Skv) if fwd_fault == "flat_mask" else m
    o = emu_softmax_fwd(P0, mask, m_used, scale, heads * Sq, Sq, fwd_fault)
    xc.compare(o, xc.softmax_fwd_refs(P0, mask, m, scale, heads * Sq), "softmax_fwd")
    dPd = xc.rnd(rows, Skv, seed=3)
    xc.compare(emu_softmax_bwd(o["P"], dPd, m, scale, bwd_fault), xc.softmax_bwd_refs(o["P"], dPd, m, scale), "softmax_bwd")


def test_softmax_emulation_inside_and_faults_outside():
    for Skv in xc.SOFTMAX["Skv"]:
        for scale in xc.SOFTMAX["scales"]:
            for p in xc.P_DROP:
                _softmax_check(Skv, scale, p)
            if Skv > 1:    # (one key: the probability is 1 under any mask)
                assert caught(lambda: _softmax_check(Skv, scale, 0.0, fwd_fault="mask_row")), ("mask row // Sq", Skv)
        _softmax_check(Skv, 1.0, 0.1, kind="all")
        if Skv > 2:        # (at one or two keys the two mask forms may agree on all 18 rows)
            assert caught(lambda: _softmax_check(Skv, 1.0, 0.1, fwd_fault="flat_mask")), ("flat-index dropout mask", Skv)
        if Skv > 1:        # (one key: dS is zero whatever the scale)
            assert caught(lambda: _softmax_check(Skv, 0.125, 0.1, bwd_fault="no_scale")), ("scale missing", Skv)
    xc.report("cpu softmax")


# ------------------------------------------------------------------------------------------------------ elementwise
def emu_act_fwd(mode, x, aux=None):
    if mode == 0:
        return {"y": x * 0.5 * (1.0 + torch.erf(x * F32_SQRT1_2))}
    if mode == 1:
        return {"y": torch.tanh(x)}
    s = 1.0 / (1.0 + torch.exp(-x))
    return {"y2": s, "y": s * aux}


F32_SQRT1_2 = torch.tensor(0.70710678118654752, dtype=F32)
F32_K = torch.tensor(0.3989422804014327, dtype=F32)


def emu_act_bwd(mode, dy, s, aux=None, fault=None):
    if mode == 0:
        gp = 0.5 * (1.0 + torch.erf(s * F32_SQRT1_2))
        if fault != "gelu_no_xphi":
            gp = gp + s * F32_K * torch.exp(-0.5 * s * s)
        return {"dx": dy * gp}
    if mode == 1:
        return {"dx": dy * (1.0 - s * s)}
    return {"dx": dy * aux * s * (1.0 - s), "dx2": dy * (aux if fault == "dx2_aux" else s)}


def _act_check(n, fault=None, modes=(0, 1, 2)):
    x = xc.uniform(n, seed=1, planted=xc.PLANTED)
    aux, dy = xc.rnd(n, seed=2), xc.rnd(n, seed=3)
    for mode in modes:
        o = emu_act_fwd(mode, x, aux)
        xc.compare(o, xc.act_fwd_refs(mode, x, aux), "act_fwd mode %d" % mode)
        saved = x if mode == 0 else (o["y"] if mode == 1 else o["y2"])
        xc.compare(emu_act_bwd(mode, dy, saved, aux, fault), xc.act_bwd_refs(mode, dy, saved, aux), "act_bwd mode %d" % mode)


@pytest.mark.parametrize("n", xc.FLAT_N)
def test_flat_emulations_inside_and_faults_outside(n):
    _act_check(n)
    assert caught(lambda: _act_check(n, "gelu_no_xphi", modes=(0,))), "gelu' without x phi(x)"
    assert caught(lambda: _act_check(n, "dx2_aux", modes=(2,))), "dx2 from aux"
    x = xc.uniform(n, seed=1, planted=xc.PLANTED)
    m = xc.cpu_dropout_mask(n, 0.1, SEED)
    xc.compare({"y": x * m}, xc.mul_refs(x, m), "dropout")
    for num, den in ((None, None), (3.0, 7.0), (3.0, 0.0), (None, 5.0), (0.25, None)):
        s = torch.tensor(1.0 if num is None else num) / torch.tensor(1.0 if den is None else max(den, 1.0))
        xc.compare({"y": x * s}, xc.scale_ratio_refs(x, num, den), "scale_by_ratio")
    assert caught(lambda: xc.compare({"y": x * (torch.tensor(3.0) / torch.tensor(0.0))}, xc.scale_ratio_refs(x, 3.0, 0.0), "x")), \
        "den = 0 not clamped"
    xc.report("cpu flat n=%d" % n)


def test_add_emulation_inside():
    for M, N in xc.ADD_MN:
        a, b = xc.rnd(M, N, seed=1), xc.rnd(M, N, seed=2)
        xc.compare({"out": a + b}, xc.add_refs(a, b), "add")
        assert caught(lambda: xc.compare({"out": a + b * (1 + 2.0 ** -20)}, xc.add_refs(a, b), "add")), (M, N)
    xc.report("cpu add")


# ----------------------------------------------------------------------------------------------------- sample gates
def _emu_gate(gate, mode):
    if mode == 0:
        return 1.0 / (1.0 + torch.exp(-gate.reshape(-1)))
    g2 = gate.reshape(-1, 2)
    return 1.0 / (1.0 + torch.exp(g2[:, 0] - g2[:, 1]))


def emu_sample_gate(a, c, gate, mode, dout, B, S, fault=None):
    H = a.shape[1]
    g = _emu_gate(gate, mode).repeat_interleave(S)[:, None]
    out = g * a if c is None else g * a + (1.0 - g) * c
    o = {"out": out, "da": g * dout}
    if c is not None:
        o["dc"] = (1.0 - g) * dout
    terms = (dout * (a if c is None else a - c)).reshape(B, S * H)
    acc = torch.stack([wave_sum(strided_sum(terms[b:b + 1], 256).reshape(4, 64)) for b in range(B)])
    gb = _emu_gate(gate, mode)
    t = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) * gb * (1.0 - gb)
    o["dgate"] = t if mode == 0 else torch.stack([t if fault == "flip_sign" else -t, t], -1)
    return o


def _sample_gate_check(B, S, H, mode, with_c, fault=None):
    a, c, dout = xc.rnd(B * S, H, seed=1), (xc.rnd(B * S, H, seed=2) if with_c else None), xc.rnd(B * S, H, seed=3)
    gate = xc.rnd(B * (mode + 1), seed=4, scale=2.0)
    o = emu_sample_gate(a, c, gate, mode, dout, B, S, fault)
    xc.compare(o, xc.sample_gate_fwd_refs(a, c, gate, mode, B, S), "sample_gate_fwd")
    xc.compare(o, xc.sample_gate_bwd_refs(dout, a, c, gate, mode, B, S), "sample_gate_bwd")
    if mode == 1:
        xc.same_bits(o["dgate"][:, 0], -o["dgate"][:, 1], "dgate words")


def test_sample_gate_emulation_inside_and_fault_outside():
    for B, S, H in xc.SAMPLE_GATE:
        for mode in (0, 1):
            for with_c in (False, True):
                _sample_gate_check(B, S, H, mode, with_c)
        assert caught(lambda: _sample_gate_check(B, S, H, 1, True, "flip_sign")), ("dgate[2b] sign", B, S, H)
    xc.report("cpu sample gates")


# -------------------------------------------------------------------------------------------------------- LSTM cell
def lstm_inputs(B, S, H):
    z = xc.uniform(B, S, 2, 4, H, seed=1, lo=-4.0, hi=4.0, planted=(40.0, -40.0))
    return z, xc.rnd(B, S, 2, H, seed=2), [xc.rnd(2, B, H, seed=10 + k) for k in range(S)]


def emu_lstm_fwd(z, c_all, y, hprev, act, B, S, H, k, fault=None):
    for d, (t, tp) in enumerate(xc.lstm_rows(B, S, k)):
        if fault == "rev_tm1" and d == 1:
            tp = t - 1
        sg = lambda v: 1.0 / (1.0 + torch.exp(-v))
        i, f, g, o = sg(z[:, t, d, 0]), sg(z[:, t, d, 1]), torch.tanh(z[:, t, d, 2]), sg(z[:, t, d, 3])
        cp = c_all[:, tp, d].clone() if k else torch.zeros(B, H)
        c = f * cp + i * g
        act[:, t, d] = torch.stack([i, f, g, o], 1)
        c_all[:, t, d] = c
        y[:, t, d] = o * torch.tanh(c)
        hprev[:, t, d] = y[:, tp, d] if k else 0.0


def emu_lstm_bwd(dy, dh_rec, dc, act, c_all, dg, B, S, H, k, first):
    for d, (t, tp) in enumerate(xc.lstm_rows(B, S, k)):
        i, f, g, o = act[:, t, d].unbind(1)
        c = c_all[:, t, d]
        cp = c_all[:, tp, d] if k else torch.zeros(B, H)
        tc = torch.tanh(c)
        dh = dy[:, t, d] + (0.0 if first else dh_rec[d])
        dcc = (0.0 if first else dc[d]) + dh * o * (1.0 - tc * tc)
        dg[:, t, d] = torch.stack([dcc * g * i * (1.0 - i), dcc * cp * f * (1.0 - f), dcc * i * (1.0 - g * g),
                                   dh * tc * o * (1.0 - o)], 1)
        dc[d] = dcc * f


def _lstm_check(B, S, H, fault=None):
    z, dy, dh = lstm_inputs(B, S, H)
    c_all, y, hprev = (torch.full((B, S, 2, H), NAN) for _ in range(3))
    act, dg = torch.full((B, S, 2, 4, H), NAN), torch.full((B, S, 2, 4, H), NAN)
    for k in range(S):
        emu_lstm_fwd(z, c_all, y, hprev, act, B, S, H, k, fault)
        for d, r in enumerate(xc.lstm_fwd_refs(z, c_all, y, B, S, H, k)):
            t = xc.lstm_rows(B, S, k)[d][0]
            xc.compare({"act": act[:, t, d], "c": c_all[:, t, d], "y": y[:, t, d]}, r, "lstm_fwd")
            xc.same_bits(hprev[:, t, d], r["hprev"], "hprev")
    dc = torch.full((2, B, H), NAN)
    for k in range(S - 1, -1, -1):
        first = k == S - 1
        dh_rec = torch.full((2, B, H), NAN) if first else dh[k]
        dc_in = dc.clone()
        emu_lstm_bwd(dy, dh_rec, dc, act, c_all, dg, B, S, H, k, first and fault != "ignore_first")
        for d, r in enumerate(xc.lstm_bwd_refs(dy, dh_rec, dc_in, act, c_all, B, S, H, k, first)):
            t = xc.lstm_rows(B, S, k)[d][0]
            xc.compare({"dgates": dg[:, t, d], "dc_carry": dc[d]}, r, "lstm_bwd")


def test_lstm_cell_emulation_inside_and_faults_outside():
    for B, S, H in xc.LSTM:
        _lstm_check(B, S, H)
        assert caught(lambda: _lstm_check(B, S, H, "ignore_first")), ("first ignored", B, S, H)
        if S > 1:
            assert caught(lambda: _lstm_check(B, S, H, "rev_tm1")), ("reverse direction reads t - 1", B, S, H)
    xc.report("cpu lstm cell")


# ------------------------------------------------------------------------------------------------------------ GEMM
def emu_gemm(op, A, B, bias, alpha, beta, c_old, fault=None):
    a = A if op in (xc.NT, xc.NN) else A.transpose(-1, -2)
    b = B.transpose(-1, -2) if op in (xc.NT, xc.TT) else B
    K = a.shape[-1]
    if fault == "ktail":
        K -= K % 16
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=F32)
    for k in range(K):                                       # the k-ordered chain of the matrix instruction
        acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    v = alpha * acc + (0.0 if bias is None else bias)
    if beta != 0 or fault == "beta0_read":
        v = v + beta * c_old
    return {"C": v}


def gemm_inputs(op, M, N, K, batch=()):
    A = xc.rnd(*batch, *((M, K) if op in (xc.NT, xc.NN) else (K, M)), seed=1)
    B = xc.rnd(*batch, *((N, K) if op in (xc.NT, xc.TT) else (K, N)), seed=2)
    return A, B, xc.rnd(N, seed=3), xc.rnd(*batch, M, N, seed=4)


def _gemm_check(op, M, N, K, with_bias, alpha, beta, fault=None, batch=()):
    A, B, bias, c_old = gemm_inputs(op, M, N, K, batch)
    bias = bias if with_bias else None
    if beta == 0:
        c_old = torch.full_like(c_old, NAN)
    xc.compare(emu_gemm(op, A, B, bias, alpha, beta, c_old, fault), xc.gemm_refs(op, A, B, bias, alpha, beta, c_old), "x_gemm")


@pytest.mark.parametrize("op", [xc.NT, xc.NN, xc.TN, xc.TT])
def test_gemm_emulation_inside_and_faults_outside(op):
    for i, (M, N) in enumerate(xc.GEMM_MN):
        for j, K in enumerate(xc.GEMM_K):
            alpha, beta = xc.GEMM_AB[(i + j) % 2]
            _gemm_check(op, M, N, K, (i + j) % 3 != 0, alpha, beta)
            if K % 16:
                assert caught(lambda: _gemm_check(op, M, N, K, True, alpha, beta, "ktail")), ("k tail dropped", M, N, K)
        assert caught(lambda: _gemm_check(op, M, N, 17, True, 1.0, 0.0, "beta0_read")), ("beta C read at beta = 0", M, N)
    _gemm_check(op, 5, 7, 9, True, 0.5, 2.0, batch=(2, 3))
    xc.report("cpu x_gemm op %d" % op)


# --------------------------------------------------------------------------------------------------------- token CE
def emu_token_ce(x, labels, mask, fault=None):
    M, C = x.shape
    valid = mask != 0
    inr = (labels >= 0) & (labels < C)
    grad_rows = {None: valid & inr, "masked_grad": inr, "oob_label_grad": valid}[fault]
    mx = x.amax(-1, keepdim=True)
    se = torch.zeros(M, 1)
    for c in range(C):
        se = se + torch.exp(x[:, c:c + 1] - mx)
    lse = mx + torch.log(se)
    onehot = torch.arange(C)[None, :] == labels.to(torch.int32)[:, None]       # (the cast to int is part of the fault)
    if fault is None:
        onehot = torch.arange(C)[None, :] == labels[:, None]
    dl = torch.where(grad_rows[:, None], torch.exp(x - lse) - onehot.to(F32), torch.zeros(M, C))
    cnt = valid & inr
    loss = torch.where(cnt, lse[:, 0] - x.gather(1, labels.clamp(0, C - 1)[:, None])[:, 0], torch.zeros(M))
    pad = torch.zeros(-(-M // 64) * 64)
    pad[:M] = loss
    total = torch.tensor(0.5)
    for w in wave_sum(pad.reshape(-1, 64)):
        total = total + w
    return {"dlogits": dl, "loss_sum": total.reshape(1)}, 2.0 + float(cnt.sum())


def _ce_check(M, C, fault=None):
    x, labels, mask = xc.ce_inputs(M, C)
    o, count = emu_token_ce(x, labels, mask, fault)
    refs = xc.token_ce_refs(x, labels, mask)
    xc.compare(o, refs, "token_ce")
    assert count == refs["count"]


def test_token_ce_emulation_inside_and_faults_outside():
    for M in xc.CE_M:
        for C, _ in xc.CE_C_LD:
            _ce_check(M, C)
            assert caught(lambda: _ce_check(M, C, "oob_label_grad")), ("valid row with label -100 gets a gradient", M, C)
            if M > 1 and C > 1:     # (M = 1 has no masked row; C = 1: softmax - onehot is 0 on an in-range row)
                assert caught(lambda: _ce_check(M, C, "masked_grad")), ("masked-out row gets a gradient", M, C)
    xc.report("cpu token_ce")
