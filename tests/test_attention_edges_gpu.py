"""GPU: attn_fwd / attn_bwd (whole-head and tiled) and the packed pair, element by element against float64, every tensor
inside guard bands (tests/kernel_check.py).  q is the middle slice of a NaN-filled [B*Sq, 3H] buffer, k / v / dout sit in NaN
bands; out, out16, lse, delta, dq and the dk | dv halves of one [B*Skv, 2H] buffer sit in sentinel bands.  The reference
dropout mask is the exported attn_dropout_mask (tied to numpy by test_attn_dropout_mask_matches_the_numpy_restatement)."""
import pytest
import torch

import kernel_check as kc
from kernel_check import BF16, F16, F32

pytestmark = pytest.mark.gpu

B, HEADS, H = 2, 2, 128
SCALE = 0.125
SEED = 0xabcdef12345
MASKS = ["prefix", "holes", "one sample fully masked", "single valid key"]


def _k():
    from icka_amd import kernels
    return kernels


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _mask01(kind, Skv):
    m = torch.ones(B, Skv)
    key = torch.arange(Skv)
    if kind == "prefix":
        m[1] = (key < max(1, Skv // 2)).float()
    elif kind == "holes":               # not a prefix; the last key stays valid
        m[0] = ((key % 3 != 1) | (key == Skv - 1)).float()
        m[1] = ((key >= Skv // 2) | (key == Skv - 1)).float()
    elif kind == "one sample fully masked":
        m[0] = 0.0
    else:
        m[0] = (key == Skv // 3).float()
        m[1] = (key < max(1, Skv - 2)).float()
    return m


def _heads(t, S):
    """[B*S, H] -> float64 [B, heads, S, 64]"""
    return t.double().view(B, S, HEADS, 64).permute(0, 2, 1, 3)


def _merge(t, S):
    return t.permute(0, 2, 1, 3).reshape(B * S, H)


def _run(k, path, Sq, Skv, p, mask_kind, qk_scale, dominant_last, label, lens=None):
    """One forward + backward.  ``lens`` (packed path): the number of valid queries of each sample, a prefix of its Sq; packed
    row cu[b] + i is padded row b * Sq + i, so sample b + 1 starts right after a shorter sample b and the query-side buffers
    hold sum(lens) rows and not one more.  The reference is the padded one, with dout zero at the queries left out."""
    q0, k0, v0 = _rnd(B * Sq, H, seed=1, scale=qk_scale), _rnd(B * Skv, H, seed=2, scale=qk_scale), _rnd(B * Skv, H, seed=3)
    if dominant_last:       # every row's dominant key is the LAST one: the running maximum jumps in the last key tile
        q0.view(B, Sq, HEADS, 64)[..., 0] = 8.0
        k0.view(B, Skv, HEADS, 64)[..., 0] = 0.0
        k0.view(B, Skv, HEADS, 64)[:, Skv - 1, :, 0] = 8.0
    q0, k0, v0, do0 = q0.to(BF16), k0.to(BF16), v0.to(BF16), _rnd(B * Sq, H, seed=5).to(BF16)
    packed = path == "packed"
    lens = [Sq] * B if lens is None else list(lens)
    assert packed or lens == [Sq] * B
    rows = torch.cat([b * Sq + torch.arange(n) for b, n in enumerate(lens)])        # the padded row of every packed row
    n_q = rows.numel()
    qvalid = torch.zeros(B * Sq, dtype=torch.bool)
    qvalid[rows] = True
    do0[~qvalid] = 0.0
    qv = qvalid.view(B, 1, Sq).expand(B, HEADS, Sq).cuda()
    rows_d = rows.cuda()
    fused = torch.full((n_q, 3 * H), float("nan"), dtype=BF16)
    fused[:, H:2 * H] = q0[rows]
    q = kc.guarded_input(fused, ld=3 * H + 8)[:, H:2 * H]
    kk, v, dout = (kc.guarded_input(t, ld=H + 8) for t in (k0, v0, do0[rows]))
    add = (1.0 - _mask01(mask_kind, Skv)) * -10000.0
    add_mask = kc.guarded_input(add.reshape(1, -1).to(F32))[0].view(B, Skv)
    out, c_out = kc.guarded(n_q, H, BF16, ld=H + 8)
    out16, c_out16 = kc.guarded(n_q, H, F16, ld=H + 8)
    lse2, c_lse = kc.guarded(1, B * HEADS * Sq, F32)
    dl2, c_delta = kc.guarded(1, B * HEADS * Sq, F32)
    lse, delta_out = lse2[0].view(B, HEADS, Sq), dl2[0].view(B, HEADS, Sq)
    dq, c_dq = kc.guarded(n_q, H, BF16, ld=H + 8)
    dkv, c_dkv = kc.guarded(B * Skv, 2 * H, BF16, ld=2 * H + 8)
    if packed:
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
        k.attn_fwd_packed(q, kk, v, add_mask, out, lse, cu, False, B, HEADS, Sq, Skv, p_drop=p, seed=SEED)
    else:
        k.attn_fwd(q, kk, v, add_mask, out, lse, B, HEADS, Sq, Skv, p_drop=p, seed=SEED, out16=out16, tiled=path == "tiled")
    # float64 reference of the forward
    qh, kh, vh, doh = _heads(q0.cuda(), Sq), _heads(k0.cuda(), Skv), _heads(v0.cuda(), Skv), _heads(do0.cuda(), Sq)
    s = (qh @ kh.transpose(-1, -2)) * SCALE + add.double().cuda()[:, None, None, :]
    pr = torch.softmax(s, -1)
    m = k.attn_dropout_mask(B * HEADS * Sq, Skv, p, SEED, "cuda").view(B, HEADS, Sq, Skv).double() if p > 0 else torch.ones_like(pr)
    Delta = kc.attn_delta(qh, kh, SCALE, s, pr > 0)
    lse_ref = torch.logsumexp(s, -1)
    o_ref = (pr * m) @ vh
    o_bound = kc.attn_fwd_bound(pr * m, vh, Delta)
    # (lse and delta are indexed by the padded query: only the entries of valid queries are defined)
    kc.assert_within(out, _merge(o_ref, Sq)[rows_d], _merge(o_bound, Sq)[rows_d], "attn %s out" % path, verbose=False)
    kc.assert_within(lse[qv], lse_ref[qv], kc.attn_lse_bound(lse_ref, Delta)[qv], "attn %s lse" % path, verbose=False)
    c_out(what=label + " out"); c_lse(what=label + " lse")
    if not packed:
        kc.assert_within(out16, _merge(o_ref, Sq), _merge(kc.attn_fwd_bound(pr * m, vh, Delta, F16), Sq), "attn %s out16" % path, verbose=False)
        c_out16(what=label + " out16")
    # backward
    dk_, dv_ = dkv[:, :H], dkv[:, H:]
    if packed:
        k.attn_bwd_packed(q, kk, v, add_mask, dout, lse, delta_out, dq, dk_, dv_, cu, False, B, HEADS, Sq, Skv, p_drop=p, seed=SEED)
    else:
        k.attn_bwd(q, kk, v, add_mask, out, dout, lse, delta_out, dq, dk_, dv_, B, HEADS, Sq, Skv, p_drop=p, seed=SEED,
                   tiled=path == "tiled")
    b = kc.attn_bwd_bounds(qh, kh, vh, s, pr, m, doh, lse_ref, Delta, SCALE)
    kc.assert_within(dq, _merge(b["dq"][0], Sq)[rows_d], _merge(b["dq"][1], Sq)[rows_d], "attn %s dq" % path, verbose=False)
    kc.assert_within(dk_, _merge(b["dk"][0], Skv), _merge(b["dk"][1], Skv), "attn %s dk" % path, verbose=False)
    kc.assert_within(dv_, _merge(b["dv"][0], Skv), _merge(b["dv"][1], Skv), "attn %s dv" % path, verbose=False)
    kc.assert_within(delta_out[qv], b["delta"][0][qv], b["delta"][1][qv], "attn %s delta" % path, verbose=False)
    c_dq(what=label + " dq"); c_dkv(what=label + " dk|dv"); c_delta(what=label + " delta")
    c_out(what=label + " out after bwd"); c_lse(what=label + " lse after bwd")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("path,Sq,Skv", [(path, Sq, Skv) for path in ("whole", "tiled", "packed")
                                         for Sq, Skv in [(1, 1), (5, 7), (65, 129), (129, 65), (130, 257)]]
                         + [("packed", 65, 128), ("packed", 128, 128)])       # the largest sizes the packed pair accepts
def test_attention_masks_scores_and_guards(path, Sq, Skv, p):
    """The packed pair runs with samples of unequal length (the first one shorter, so the second starts right behind it in
    every query-side buffer) and once with every query valid."""
    if path == "packed" and (Sq > 128 or Skv > 128):
        with pytest.raises(ValueError):     # the packed pair is the whole-head kernels: the refusal is the assertion
            _k().attn_fwd_packed(*[torch.empty(B * Sq, H, dtype=BF16, device="cuda")] * 3, torch.zeros(B, Skv, device="cuda"),
                                 torch.empty(B * Sq, H, dtype=BF16, device="cuda"), torch.empty(B * HEADS * Sq, device="cuda"),
                                 torch.zeros(B + 1, dtype=torch.int32, device="cuda"), False, B, HEADS, Sq, Skv)
        return
    k = _k()
    k.set_dropout_nonce(None)
    lens = (max(1, Sq - Sq // 3), Sq) if path == "packed" else None
    for mask_kind in MASKS:
        for qk_scale in (1.0, 4.0):
            _run(k, path, Sq, Skv, p, mask_kind, qk_scale, False, "%s %dx%d %s x%g" % (path, Sq, Skv, mask_kind, qk_scale), lens)
    _run(k, path, Sq, Skv, p, "prefix", 1.0, True, "%s %dx%d dominant last key" % (path, Sq, Skv))
    kc.report("attention %s %dx%d p=%g" % (path, Sq, Skv, p))
