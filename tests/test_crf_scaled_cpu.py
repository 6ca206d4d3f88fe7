"""CPU: the scaled linear-domain forward-backward that crf.hip runs for <= 16 tags (a_t = (a_{t-1} . E) x_t / sum(a_{t-1}),
normaliser lagging one step; bhat_{t-1} = E (x_t bhat_t / S_{t-1}); marginal_t = a_t . bhat_t), restated in numpy float32
and checked against the oracle (oracle/crf_oracle.py, float64, autograd) -- the algebra the kernel relies on, without a GPU."""
import numpy as np
import torch

from oracle import crf_oracle as O


def scaled_forward_backward(e, tags, L, start, end, trans):
    """one sample; returns (log Z, d(-llh)/d e [S, C]) in float32 arithmetic"""
    f = np.float32
    S, C = e.shape
    mT = trans.max()
    E = np.exp(trans - mT).astype(f)
    mx = e.max(1)
    x = np.exp(e - mx[:, None]).astype(f)
    mS = start.max()
    a = (np.exp(start - mS) * x[0]).astype(f)
    al, Sc = [a.copy()], {}
    lz = f(mS + mx[0])
    for t in range(1, S):
        if t < L:
            sm = a.sum(dtype=f)
            Sc[t] = sm
            a = ((a @ E) * (x[t] * (f(1) / sm))).astype(f)
            lz = f(lz + np.log(sm) + mx[t] + mT)
        al.append(a.copy())
    mE = end.max()
    zend = (a * np.exp(end - mE)).sum(dtype=f)
    logz = f(lz + mE + np.log(zend))
    bh = (np.exp(end - mE) / zend).astype(f)
    de = np.zeros((S, C), f)
    for t in range(S - 1, -1, -1):
        if t >= L and t > 0:
            continue
        marg = al[t] * bh
        onehot = np.zeros(C, f); onehot[tags[t]] = 1
        de[t] = marg - onehot          # d(-llh)/de
        if t == 0:
            break
        u = (x[t] * bh / Sc[t]).astype(f)
        bh = (E @ u).astype(f)
    return logz, de


def test_scaled_forward_backward_matches_the_oracle():
    g = torch.Generator().manual_seed(3)
    B, S, C = 5, 40, 13
    e = torch.randn(B, S, C, generator=g) * 3.0
    tags = torch.randint(0, C, (B, S), generator=g)
    lens = torch.tensor([S, 1, 17, 33, 2])
    mask = torch.arange(S)[None, :] < lens[:, None]
    start, end = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    trans = torch.randn(C, C, generator=g) * 0.7
    trans[2, 5] = -1e4                                   # a forbidden transition: E = 0 exactly
    er = e.double().clone().requires_grad_(True)
    ref = O.crf_llh(er, tags, mask, start.double(), end.double(), trans.double())
    (-ref.sum()).backward()
    gold = O.crf_llh(e.double(), tags, mask, start.double(), end.double(), trans.double())
    for b in range(B):
        logz, de = scaled_forward_backward(e[b].numpy(), tags[b].numpy(), int(lens[b]), start.numpy(), end.numpy(), trans.numpy())
        # marginals (= gradient of -llh w.r.t. the emissions)
        assert np.abs(de - er.grad[b].numpy()).max() < 2e-4
        # normaliser: llh = gold-path score - log Z
        tb, L = tags[b].numpy(), int(lens[b])
        score = float(start[tb[0]] + e[b, 0, tb[0]] + sum(trans[tb[t - 1], tb[t]] + e[b, t, tb[t]] for t in range(1, L)) + end[tb[L - 1]])
        assert abs((score - float(logz)) - float(gold[b])) < 2e-3 * max(1.0, abs(float(gold[b])) / 50)


# ------------------------------------------------------------------------------------------------------------------
# The same recursion as one call of crf_grad_small_kernel does it: any mask (holes, mask[0] == 0, None), clamped labels, the
# upstream gllh, d_start / d_end / d_trans, the normalisers it tests before it gives up -- and, for
# tests/test_crf_check_cpu.py, the faults that file seeds (``fault``; None = the kernel's rules).
FAULTS_LIN = ("advance_off", "end_last_on", "gold_prev_on", "norm_next", "de_unwritten", "trans_transposed")


def ftz(v):
    """f32 with results below the smallest normal number flushed to zero (what the device exp does to them)."""
    v = np.asarray(v, np.float32)
    return np.where(np.abs(v) < np.float32(2.0 ** -126), np.float32(0), v)


def mask_rules(mask_row, S):
    """-> (on [S] bool: step 0 and every t with mask[t] != 0;  last: sum(mask) - 1, or 0 for an empty mask)"""
    raw = np.ones(S, bool) if mask_row is None else np.asarray(mask_row) != 0
    on = raw.copy()
    on[0] = True
    cnt = int(raw.sum())
    return on, (cnt - 1 if cnt > 0 else 0)


def gold_score_f32(e, y, on, last, start, end, trans, fault=None):
    f = np.float32
    s, prev_on = f(0), 0
    for t in range(e.shape[0]):
        if not on[t]:
            continue
        yp = y[prev_on] if fault == "gold_prev_on" else y[t - 1]      # the kernel: the LITERAL previous position
        s = f(s + e[t, y[t]] + (start[y[t]] if t == 0 else trans[yp, y[t]]))
        prev_on = t
    if fault == "end_last_on":
        last = int(np.nonzero(on)[0][-1])
    return f(s + end[y[last]])


def scaled_full(e, tags, mask_row, start, end, trans, g=1.0, fault=None):
    """One sample, float32 -> dict(llh, de [S, C] (NaN where nothing was written), dstart, dend, dtrans (this sample's g * d
    llh / d .), ok (the kernel keeps the scaled result), norms (every normaliser and zend), bh_max)."""
    f = np.float32
    e, start, end, trans = (np.asarray(v, f) for v in (e, start, end, trans))
    S, C = e.shape
    on, last = mask_rules(mask_row, S)
    step = np.ones(S, bool) if fault == "advance_off" else on
    y = np.clip(np.asarray(tags), 0, C - 1)
    with np.errstate(all="ignore"):
        mT = trans.max()
        E = ftz(np.exp(trans - mT))
        mx = e.max(1)
        x = ftz(np.exp(e - mx[:, None]))
        mS, mE = start.max(), end.max()
        a = ftz(np.exp(start - mS) * x[0])
        al, Sc = [a.copy()], {}
        lz = f(mS + mx[0])
        for t in range(1, S):
            if step[t]:
                sm = a.sum(dtype=f)
                Sc[t] = sm
                a = ftz(ftz(a[:, None] * E).sum(0, dtype=f) * ftz(x[t] * (f(1) / sm)))
                lz = f(lz + np.log(sm) + mx[t] + mT)
            al.append(a.copy())
        wE = ftz(np.exp(end - mE))
        zend = (a * wE).sum(dtype=f)
        logz = f(lz + mE + np.log(zend))
        norms = np.array(list(Sc.values()) + [zend], f)
        ok = bool(np.all((norms > f(1e-30)) & (norms < f(1e30))) and np.isfinite(logz))
        bh = (wE / zend).astype(f)
        bh_max = float(np.max(np.where(np.isnan(bh), np.inf, np.abs(bh))))
        dend = -(a * bh)
        dstart = np.zeros(C, f)
        dT = np.zeros((C, C), f)
        de = np.full((S, C), np.nan, f)
        prev_on = {}
        p = 0
        for t in range(S):
            if on[t]:
                prev_on[t], p = p, t
        for t in range(S - 1, -1, -1):
            if not step[t]:
                if fault != "de_unwritten":
                    de[t] = 0
                continue
            marg = ftz(al[t] * bh)
            ok = ok and bool(np.all(np.isfinite(marg)))
            onehot = np.zeros(C, f); onehot[y[t]] = 1
            de[t] = f(g) * (onehot - marg) if on[t] else 0
            if t == 0:
                dstart = onehot - marg
                break
            c = Sc[t + 1] if (fault == "norm_next" and t + 1 in Sc) else Sc[t]
            u = ftz(ftz(x[t] * (f(1) / c)) * bh)
            dT = (dT - ftz(ftz(al[t - 1][:, None] * E) * u[None, :])).astype(f)
            if on[t]:
                dT[y[prev_on[t]] if fault == "gold_prev_on" else y[t - 1], y[t]] += 1
            bh = ftz(ftz(E * u[None, :]).sum(1, dtype=f))
            bh_max = max(bh_max, float(np.max(np.where(np.isnan(bh), np.inf, np.abs(bh)))))
        dend[y[int(np.nonzero(on)[0][-1]) if fault == "end_last_on" else last]] += 1
        num = gold_score_f32(e, y, on, last, start, end, trans, fault)
        dT = f(g) * dT
    return {"llh": f(num - logz), "de": de, "dstart": f(g) * dstart, "dend": f(g) * dend,
            "dtrans": dT.T.copy() if fault == "trans_transposed" else dT, "ok": ok, "norms": norms, "logz": logz,
            "bh_max": bh_max}


def _lse0(v):
    """log-sum-exp over axis 0 the way the kernels do it: max, exp of the differences, log of their sum (f32)."""
    m = v.max(0)
    return (m + np.log(np.exp(v - m[None]).sum(0, dtype=np.float32))).astype(np.float32)


def log_full(e, tags, mask_row, start, end, trans, g=1.0, fault=None):
    """The log-domain recursion of crf_grad_small_log / crf_grad_kernel, float32, same results layout as ``scaled_full``."""
    f = np.float32
    e, start, end, trans = (np.asarray(v, f) for v in (e, start, end, trans))
    S, C = e.shape
    on, last = mask_rules(mask_row, S)
    step = np.ones(S, bool) if fault == "advance_off" else on
    y = np.clip(np.asarray(tags), 0, C - 1)
    with np.errstate(all="ignore"):
        a = (start + e[0]).astype(f)
        al = [a.copy()]
        for t in range(1, S):
            if step[t]:
                a = (_lse0((a[:, None] + trans).astype(f)) + e[t]).astype(f)
            al.append(a.copy())
        v = (a + end).astype(f)
        logz = _lse0(v[:, None])[0]
        beta = end.copy()
        dend = -np.exp(v - logz).astype(f)
        dstart = np.zeros(C, f)
        dT = np.zeros((C, C), f)
        de = np.full((S, C), np.nan, f)
        prev_on = {}
        p = 0
        for t in range(S):
            if on[t]:
                prev_on[t], p = p, t
        for t in range(S - 1, -1, -1):
            if not step[t]:
                if fault != "de_unwritten":
                    de[t] = 0
                continue
            marg = np.exp(((al[t] + beta).astype(f) - logz).astype(f)).astype(f)
            onehot = np.zeros(C, f); onehot[y[t]] = 1
            de[t] = f(g) * (onehot - marg) if on[t] else 0
            if t == 0:
                dstart = onehot - marg
                break
            u = (e[t] + beta).astype(f)
            arg = (((al[t - 1][:, None] + trans).astype(f) + u[None, :]).astype(f) - logz).astype(f)
            dT = (dT - np.exp(arg).astype(f)).astype(f)
            if on[t]:
                dT[y[prev_on[t]] if fault == "gold_prev_on" else y[t - 1], y[t]] += 1
            beta = _lse0((trans + u[None, :]).astype(f).T.copy())
        dend[y[int(np.nonzero(on)[0][-1]) if fault == "end_last_on" else last]] += 1
        num = gold_score_f32(e, y, on, last, start, end, trans, fault)
        dT = f(g) * dT
    return {"llh": f(num - logz), "de": de, "dstart": f(g) * dstart, "dend": f(g) * dend,
            "dtrans": dT.T.copy() if fault == "trans_transposed" else dT, "ok": True, "logz": logz}
