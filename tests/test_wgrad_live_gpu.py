"""GPU: weight gradients summed over the token rows whose gradient is non-zero (ops.WGRAD_LIVE).

Three levels, every comparison BITWISE against the same computation over all rows:
  * the grouped 12-wave weight-gradient launch with per-problem row-liveness flags (icka_gemm_grouped_live);
  * the LayerNorm backward that writes the flags (icka_ln_bwd_slabs_live);
  * two BertLayers, backward with the switch on and off.
A skipped k-tile only ever adds +-0 products to accumulators that started at +0, so equality is exact, not a tolerance."""
import copy

import pytest
import torch

import icka_amd
from icka_amd import kernels as K
from icka_amd import ops, synth
from icka_amd.config import BertConfig

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
M_OUT = 768
NS = (2304, 768, 3072, 3072)        # the four weight gradients of a BERT-base layer: 54 + 18 + 72 + 72 = 216 tiles of 256 x 128
KT = 64                             # rows per k-tile

_CACHE = {}


def _operands(Kr):
    """Random operands of one grouped launch at reduction length Kr, made once and never modified."""
    if Kr not in _CACHE:
        g = torch.Generator(device="cuda").manual_seed(1000 + Kr)
        A = torch.randn(Kr, M_OUT, generator=g, device="cuda", dtype=F32).to(BF16)
        Bs = [torch.randn(Kr, n, generator=g, device="cuda", dtype=F32).to(BF16) for n in NS]
        C0 = [torch.randn(M_OUT, n, generator=g, device="cuda", dtype=F32) for n in NS]
        # LayerNorm slab layout: [slabs][icka_ln_slab_slots()][H], the reduction reads slots 0 and 1
        part = torch.randn(8, K._lib.load().icka_ln_slab_slots(), M_OUT, generator=g, device="cuda", dtype=F32)
        _CACHE[Kr] = (A, Bs, C0, part)
    return _CACHE[Kr]


def _tile_flags(Kr, live_tiles):
    f = torch.zeros(Kr, dtype=torch.uint8)
    for t in live_tiles:
        f[t * KT:(t + 1) * KT] = 1
    return f


def _row_flags(Kr, rows):
    f = torch.zeros(Kr, dtype=torch.uint8)
    f[list(rows)] = 1
    return f


def _patterns(Kr):
    """name -> list of 4 per-problem flag tensors (uint8 [Kr] on the CPU) or None (null pointer: every row live)."""
    nt = Kr // KT
    same = lambda f: [f, f, f, f]
    return {
        "all_live": same(_tile_flags(Kr, range(nt))),
        "all_dead": same(_tile_flags(Kr, [])),
        "first_dead": same(_tile_flags(Kr, range(1, nt))),
        "last_dead": same(_tile_flags(Kr, range(nt - 1))),
        "alternating": same(_tile_flags(Kr, range(0, nt, 2))),
        "single_live": same(_tile_flags(Kr, [nt // 2 + 1])),
        "per_problem": [_tile_flags(Kr, range(1, nt)), _tile_flags(Kr, range(1, nt, 2)), None, _tile_flags(Kr, [nt - 1])],
        # live rows scattered inside otherwise dead tiles: a tile with ONE live byte stays live
        "scattered": same(_row_flags(Kr, [5, 3 * KT + 63, 6 * KT])),
    }


def _launch(Kr, flags, variant, use_flags, poison=False):
    """One grouped TN launch; B rows are zero (``poison``: NaN) wherever the problem's flag is 0.  Returns every output as a
    list of tensors."""
    A, Bs, C0, part = _operands(Kr)
    beta = 1.0 if variant == "beta1" else 0.0
    descs, outs, keep, kl = [], [], [], []
    for i, n in enumerate(NS):
        f = flags[i]
        B = Bs[i] if f is None else Bs[i] * f.cuda().to(BF16)[:, None]
        if poison:
            B = B.clone()
            B[f.cuda() == 0] = float("nan")
        C = C0[i].clone() if beta else torch.full((M_OUT, n), float("nan"), device="cuda", dtype=F32)
        kw = {}
        if variant == "colsum":
            cs = torch.full((M_OUT,), float("nan"), device="cuda", dtype=F32)
            kw = dict(colsum_out=cs)
            outs.append(cs)
        if variant == "wire":
            w = torch.zeros(M_OUT, n, device="cuda", dtype=BF16)
            kw = dict(out3=w)
            outs.append(w)
        descs.append(K.gemm_desc(K.GEMM_TN, A, B, C, beta=beta, **kw))
        outs.append(C)
        keep.append(B)
        kl.append(None if f is None else f.cuda())
    reds = None
    if variant == "slab":
        r0, r1 = (torch.full((M_OUT,), float("nan"), device="cuda", dtype=F32) for _ in range(2))
        reds = [K.slab_reduction(part, 8, M_OUT, (r0, r1), False)]
        outs += [r0, r1]
    K.gemm_grouped(descs, reductions=reds, k_live=kl if use_flags else None)
    torch.cuda.synchronize()
    return outs


PATTERN_NAMES = ("all_live", "all_dead", "first_dead", "last_dead", "alternating", "single_live", "per_problem", "scattered")


@pytest.mark.parametrize("variant", ["plain", "beta1", "colsum", "slab", "wire"])
@pytest.mark.parametrize("pattern", PATTERN_NAMES)
def test_grouped_live_launch_is_bitwise_the_full_reduction(pattern, variant):
    Kr = 512
    flags = _patterns(Kr)[pattern]
    full = _launch(Kr, flags, variant, use_flags=False)
    live = _launch(Kr, flags, variant, use_flags=True)
    assert len(full) == len(live)
    for a, b in zip(full, live):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a, b), (pattern, variant, (a.float() - b.float()).abs().max().item())
    if pattern == "all_dead" and variant == "plain":
        assert all(int((c != 0).sum()) == 0 for c in live)        # no live tile: nothing staged, the epilogue writes zeros


@pytest.mark.parametrize("variant", ["plain", "wire"])
def test_dead_tiles_are_not_read_into_the_sum(variant):
    """The launch really takes the shortened path: with NaN in the dead rows of B the flagged launch equals the launch on the
    zeroed B, and the launch without flags (which reduces over every row) does not."""
    Kr = 512
    nt = Kr // KT
    flags = [_tile_flags(Kr, range(0, nt, 2)), _tile_flags(Kr, [3]), _tile_flags(Kr, range(1, nt)), _tile_flags(Kr, [])]
    want = _launch(Kr, flags, variant, use_flags=False)
    got = _launch(Kr, flags, variant, use_flags=True, poison=True)
    for a, b in zip(want, got):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a, b)
    full = _launch(Kr, flags, variant, use_flags=False, poison=True)
    assert all(torch.isnan(c.float()).all() for c in full)        # every output element sums over a poisoned row


def test_grouped_live_launch_two_mask_words():
    """K = 8192: 128 k-tiles = two 64-bit words of live tiles, dead tiles in both."""
    Kr = 8192
    nt = Kr // KT
    f0 = _tile_flags(Kr, [t for t in range(nt) if t % 3 != 1 and t not in (0, 63, 64, 127)])
    f1 = _tile_flags(Kr, [63, 64])
    f2 = _tile_flags(Kr, range(70, nt))                           # first word all dead
    f3 = _tile_flags(Kr, range(0, 40))                            # second word all dead
    flags = [f0, f1, f2, f3]
    for a, b in zip(_launch(Kr, flags, "plain", False), _launch(Kr, flags, "plain", True)):
        assert not torch.isnan(a).any()
        assert torch.equal(a, b)
    _CACHE.pop(Kr, None)


def test_ln_bwd_slabs_live_flags_and_outputs():
    B, S, H = 4, 64, 768
    M = B * S
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(M, H, generator=g, device="cuda", dtype=F32).to(BF16)
    xhat = torch.randn(M, H, generator=g, device="cuda", dtype=F32).to(BF16)
    rstd = torch.rand(M, generator=g, device="cuda", dtype=F32) + 0.5
    gamma = torch.randn(H, generator=g, device="cuda", dtype=F32)
    zero_rows = list(range(40, 64)) + list(range(64 + 50, 128)) + [130, 131, 188, 189] + list(range(192, 256))
    dy[zero_rows] = 0
    dy[45] = 0
    dy[45, H - 1] = 1.0                                           # a single non-zero element, in the last chunk
    zero_rows.remove(45)
    # row 46: the residual gradient ds itself is non-zero ONLY in the last 8-column chunk (one dy element would make ds dense
    # through the row means).  gamma = 1 and xhat = 0 at the two columns, dy = +1 / -1: both row sums are exactly 0, so
    # ds = rstd * gamma * dy there and 0 everywhere else
    gamma[H - 8] = gamma[H - 1] = 1.0
    xhat[46, H - 8] = xhat[46, H - 1] = 0
    dy[46] = 0
    dy[46, H - 8], dy[46, H - 1] = 1.0, -1.0
    zero_rows.remove(46)
    mask = torch.zeros(B, S, device="cuda", dtype=F32)
    mask[0, :36] = -3000.0                                        # a graded mask whose masked keys lie exactly 5000 below the open
    mask[0, 36:] = -8000.0                                        # ones: closed; rows with (36..39, 45, 46) and without (40..63) gradient
    mask[1, 55:] = -10000.0                                       # unmasked zero rows 50..54, masked zero rows 55..63
    mask[2, :60] = -4999.0                                        # a graded mask 2 apart (P at the "masked" keys is not 0): nothing is
    mask[2, 60:] = -5001.0                                        # closed; zero rows 130, 131 (upper level) and 188, 189 (lower level)
    mask[3, :] = -10000.0                                         # no open key at all: the sample's rows stay live as keys
    ws_n = K._lib.load().icka_ln_bwd_workspace_floats(H)
    out = {}
    for name in ("plain", "live"):
        ws = torch.zeros(ws_n, device="cuda", dtype=F32)
        dres = torch.zeros(M, H, device="cuda", dtype=BF16)
        dx = torch.zeros(M, H, device="cuda", dtype=BF16)
        if name == "plain":
            K.ln_bwd_slabs(dy, xhat, rstd, gamma, ws, dres=dres, dx=dx, p_drop=0.1, seed=77)
        else:
            rl = torch.full((M,), 7, device="cuda", dtype=torch.uint8)
            rk = torch.full((M,), 7, device="cuda", dtype=torch.uint8)
            K.ln_bwd_slabs_live(dy, xhat, rstd, gamma, ws, rl, row_live_kv=rk, add_mask=mask, dres=dres, dx=dx, p_drop=0.1, seed=77)
        out[name] = (dres, dx, ws)
    torch.cuda.synchronize()
    for a, b in zip(out["plain"], out["live"]):
        assert torch.equal(a, b)
    want = torch.ones(M, dtype=torch.uint8)
    want[zero_rows] = 0
    assert torch.equal(rl.cpu(), want)
    assert torch.equal(rl.cpu(), (out["live"][0] != 0).any(dim=1).to(torch.uint8).cpu())
    assert (out["live"][0][46] != 0).nonzero().view(-1).tolist() == [H - 8, H - 1]
    m = mask.cpu()
    open_key = (m - m.max(dim=1, keepdim=True).values) > -5000.0  # closed: some key of the sample lies 5000 or more above
    assert not open_key[0, 36:].any() and open_key[2].all() and open_key[3].all()
    want_kv = want | open_key.reshape(-1).to(torch.uint8)
    assert torch.equal(rk.cpu(), want_kv)
    assert int(want_kv.sum()) < M and int((want_kv != want).sum()) > 0
    # row_live alone (no mask) is the same bytes
    rl2 = torch.full((M,), 7, device="cuda", dtype=torch.uint8)
    K.ln_bwd_slabs_live(dy, xhat, rstd, gamma, torch.zeros(ws_n, device="cuda", dtype=F32), rl2, dres=torch.zeros_like(dy))
    assert torch.equal(rl2.cpu(), want)


# ------------------------------------------------------------------------------------------------------- layer level
LENS = (128, 70, 64, 33)            # dead 64-token tiles exist, one sample ends mid-tile


class _TwoLayers(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        from icka_amd.modeling import BertLayer
        self.l0 = BertLayer(cfg)
        self.l1 = BertLayer(cfg)


_BASE = {}


def _base_model():
    if "m" not in _BASE:
        cfg = BertConfig(512, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
                         max_position_embeddings=128)
        m = _TwoLayers(cfg)
        synth.fill_module_(m)
        g = torch.Generator().manual_seed(11)
        _BASE["m"] = m
        _BASE["x"] = torch.randn(4, 128, 768, generator=g)
    return _BASE["m"], _BASE["x"]


def _run_layers(precision, valid_only, live_on, monkeypatch):
    """One train-mode forward + backward of a fresh copy; returns (gradients, flag tensors the grouped launches got)."""
    from icka_amd.arena import arena_of
    base, x = _base_model()
    m = icka_amd.set_precision(copy.deepcopy(base).cuda().train(), precision)
    valid = (torch.arange(128)[None, :] < torch.tensor(LENS)[:, None]).float()
    ext = ((1.0 - valid) * -10000.0)[:, None, None, :].cuda()
    seen = []
    real = K.gemm_grouped

    def spy(descs, reductions=None, k_live=None):
        seen.append(None if k_live is None else [None if f is None else f.clone() for f in k_live])
        return real(descs, reductions=reductions, k_live=k_live)

    monkeypatch.setattr(K, "gemm_grouped", spy)
    monkeypatch.setattr(ops, "WGRAD_LIVE", live_on)
    for i, layer in enumerate((m.l0, m.l1)):
        arena_of(layer).set_seed(4242 + i)
    xi = x.cuda().requires_grad_(True)
    y = m.l1(m.l0(xi, ext), ext)
    if valid_only:
        loss = (y.float() * valid.cuda()[:, :, None]).square().sum()
    else:
        loss = y.float().square().sum()
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "gemm_grouped", real)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads["input"] = xi.grad.detach().clone()
    return grads, seen


def _dead_tiles(flags):
    return int((flags.view(-1, KT).max(dim=1).values == 0).sum())


@pytest.mark.parametrize("precision,valid_only", [("bf16", True), ("bf16", False), ("mixed16", True)])
def test_layer_gradients_are_bitwise_equal_with_and_without_live_rows(precision, valid_only, monkeypatch):
    on, seen_on = _run_layers(precision, valid_only, True, monkeypatch)
    off, seen_off = _run_layers(precision, valid_only, False, monkeypatch)
    assert all(s is None for s in seen_off)                       # the switch really turns the flags off
    launches = [s for s in seen_on if s is not None]
    assert len(launches) == 2 and all(len(s) == 4 and all(f is not None for f in s) for s in launches)
    dead = [_dead_tiles(f) for s in launches for f in s]
    print("\n[%s valid_only=%s] dead 64-token tiles per weight gradient (of 8): %s" % (precision, valid_only, dead))
    if valid_only:
        # lengths 128 / 70 / 64 / 33: the second 64-token tile of samples 2 and 3 has no valid token (sample 1 ends mid-tile)
        assert all(d >= 1 for d in dead), dead                    # the shortened path was taken, not merely allowed
    else:
        assert all(d == 0 for d in dead), dead                    # masked rows carry gradient: nothing may be skipped
    assert sorted(on) == sorted(off)
    for k in on:
        assert torch.equal(on[k], off[k]), (k, (on[k].float() - off[k].float()).abs().max().item())
        assert torch.isfinite(on[k].float()).all(), k
