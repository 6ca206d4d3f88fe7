"""Helpers of the variable-length LSTM tests (no test functions): a float64 restatement of what the kernels of csrc/lstm.hip
compute under ``lens`` (include/icka_hip.h: icka_lstm_fwd_varlen) -- the recurrence over ALL S positions with the i and f
pre-activations of every position t >= lens[b] set to -1e4, and the kernels' analytic backward (lstm_cell_bwd) -- and the
thing it has to equal: ``torch.nn.LSTM`` on a ``pack_padded_sequence(enforce_sorted=False)`` input, re-padded to S.

Why the mask is enough (float64 here, f32 on the device alike): sigmoid(-1e4 + anything the recurrence adds) is exactly 0
(exp overflows to inf), so at a pad c = 0 * c' + 0 * g = 0 and h = o * tanh(0) = 0 exactly: the reverse direction reaches a
sample's last real token with the zero state, the forward direction's state after it is never read by a live position.  The
backward at a pad has tanh(c) = 0 and i = f = 0, so every gate gradient is 0 * (something finite) = 0 and the carry dc * f = 0,
whatever dy holds there.

Layouts: x [B, S, I]; w_ih [2][4H, I], w_hh [2][4H, H], b_ih / b_hh [2][4H] (direction 0 forward, 1 reverse; gates i, f, g, o)."""
import torch

PAD_GATE = -1e4     # LSTM_PAD_GATE of csrc/lstm_core.h


def clamp_lens(lens, S):
    return torch.as_tensor(lens, dtype=torch.int64).clamp(0, S)


def pad_mask(lens, S):
    """bool [B, S]: True at t >= lens[b]."""
    return torch.arange(S).unsqueeze(0) >= clamp_lens(lens, S).unsqueeze(1)


def mask_gates(gx, lens, B, S, H):
    """A copy of gates_x [B*S, 8H] (column = dir*4H + gate*H + unit) with the i and f columns of both directions := -1e4 at
    the pads: what the fixed-length entry has to be fed to compute what the variable-length entry computes."""
    out = gx.clone().reshape(B, S, 2, 4, H)
    pad = pad_mask(lens, S).to(gx.device)
    out[:, :, :, :2][pad] = PAD_GATE
    return out.reshape(B * S, 8 * H)


def masked_bilstm(x, lens, w_ih, w_hh, b_ih, b_hh, dy=None):
    """float64 -> dict: out [B, S, 2H], h_n / c_n [2, B, H], act [B, S, 2, 4, H], c_all / hprev [B, S, 2, H], and with ``dy``
    [B, S, 2H] (any values at the pads): dgates [B, S, 2, 4, H], dx, dw_ih / dw_hh / db (lists over the directions; db is the
    gradient of b_ih and of b_hh alike)."""
    x = x.double()
    B, S, _ = x.shape
    H = w_hh[0].shape[1]
    ln = clamp_lens(lens, S)
    pad = pad_mask(lens, S)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    act, c_all, hprev, y = z(B, S, 2, 4, H), z(B, S, 2, H), z(B, S, 2, H), z(B, S, 2, H)
    for d in (0, 1):
        gx = (x @ w_ih[d].double().t() + b_ih[d].double() + b_hh[d].double()).reshape(B, S, 4, H).clone()
        gx[:, :, :2][pad] = PAD_GATE
        h, c = z(B, H), z(B, H)
        for t in (range(S) if d == 0 else range(S - 1, -1, -1)):
            pre = gx[:, t] + (h @ w_hh[d].double().t()).reshape(B, 4, H)
            i, f, o = (1.0 / (1.0 + torch.exp(-pre[:, q])) for q in (0, 1, 3))      # sigmoid_f of common.h
            g = torch.tanh(pre[:, 2])
            hprev[:, t, d] = h
            c = f * c + i * g
            h = o * torch.tanh(c)
            act[:, t, d] = torch.stack((i, f, g, o), 1)
            c_all[:, t, d], y[:, t, d] = c, h
    rows = torch.arange(B)
    last = (ln - 1).clamp(min=0)
    live = (ln > 0).double().unsqueeze(1)
    res = {"out": y.reshape(B, S, 2 * H), "act": act, "c_all": c_all, "hprev": hprev,
           "h_n": torch.stack((y[rows, last, 0] * live, y[:, 0, 1]), 0),
           "c_n": torch.stack((c_all[rows, last, 0] * live, c_all[:, 0, 1]), 0)}
    if dy is None:
        return res
    dy = dy.double().reshape(B, S, 2, H)
    dg = z(B, S, 2, 4, H)
    for d in (0, 1):
        carry, nxt = z(B, H), z(B, 4 * H)
        for t in (range(S - 1, -1, -1) if d == 0 else range(S)):       # against the direction
            i, f, g, o = act[:, t, d].unbind(1)
            tp = t - 1 if d == 0 else t + 1
            cp = c_all[:, tp, d] if 0 <= tp < S else z(B, H)
            dh = dy[:, t, d] + nxt @ w_hh[d].double()
            tc = torch.tanh(c_all[:, t, d])
            dc = dh * o * (1 - tc * tc) + carry
            carry = dc * f
            dg[:, t, d] = torch.stack((dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), 1)
            nxt = dg[:, t, d].reshape(B, 4 * H)
    res["dgates"] = dg
    flat = lambda d: dg[:, :, d].reshape(B * S, 4 * H)
    res["dx"] = sum(flat(d) @ w_ih[d].double() for d in (0, 1)).reshape(x.shape)
    res["dw_ih"] = [flat(d).t() @ x.reshape(B * S, -1) for d in (0, 1)]
    res["dw_hh"] = [flat(d).t() @ hprev[:, :, d].reshape(B * S, H) for d in (0, 1)]
    res["db"] = [flat(d).sum(0) for d in (0, 1)]
    return res


def packed_lstm(lstm, x, lens):
    """``lstm`` (a batch_first bidirectional nn.LSTM) on pack_padded_sequence(x, lens, enforce_sorted=False), re-padded to
    S -> (out, (h_n, c_n)).  Every length must be >= 1 (ATen refuses an empty sequence)."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    S = x.shape[1]
    packed = pack_padded_sequence(x, clamp_lens(lens, S), batch_first=True, enforce_sorted=False)
    out, hc = lstm(packed)
    out, _ = pad_packed_sequence(out, batch_first=True, total_length=S)
    return out, hc


def lstm_params(lstm):
    """nn.LSTM -> (w_ih, w_hh, b_ih, b_hh), each a list over the two directions."""
    get = lambda n: [getattr(lstm, n + "_l0").detach(), getattr(lstm, n + "_l0_reverse").detach()]
    return get("weight_ih"), get("weight_hh"), get("bias_ih"), get("bias_hh")
