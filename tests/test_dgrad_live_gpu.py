"""GPU: input-gradient GEMMs that do not fetch the dead token rows of their A operand (icka_gemm_live, ops.DGRAD_LIVE).

Two levels, every comparison BITWISE against the plain launch:
  * the two kernels that have a LIVE instance -- the 8-wave NN kernel on 128 x 96 tiles (ring of 3) and the 12-wave NN kernel on
    256 x 192 tiles -- at the smallest shapes the launch ladder still sends to them, over the epilogues of the encoder backward
    and flag patterns at and below the granularity of a loader piece (8 rows);
  * two BertLayers, backward with the switch on and off.
A dead 8-row piece is staged from a line of zeros instead of from A: LDS holds the same zeros, so equality is exact.  That the LIVE
instance (and not the fallback) ran is shown by the poison tests: NaN in the dead pieces of A reaches the plain launch's output and
not the live launch's."""
import copy

import pytest
import torch

import icka_amd
from icka_amd import kernels as K
from icka_amd import ops, synth
from icka_amd.config import BertConfig

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
PIECE = 8                           # rows of A per loader piece (1 KiB of a 64-deep k-tile)
# (M, N): the smallest grids the ladder sends to each kernel -- 128x96 tiles: fewer than 256 tiles of 128x128 and more of 128x96;
# 256x192 tiles: M / 256 * N / 192 >= 128 tiles, a multiple of 8, at least 3/4 of a round of 256
SHAPES = {"ws96": (256, 768), "w3": (4096, 3072)}
KS = {"ws96": (64, 128, 192, 256), "w3": (64, 128, 192)}      # 1 .. 4 k-tiles: prologue and tail of the rings of 3
EPIS = ("none", "add", "dgelu")

_CACHE = {}


def _operands(kernel, Kd):
    """Random operands of one launch, made once and never modified: A [M,K], B [K,N] (NN), aux [M,N]."""
    key = (kernel, Kd)
    if key not in _CACHE:
        M, N = SHAPES[kernel]
        g = torch.Generator(device="cuda").manual_seed(7000 + 13 * Kd + M)
        A = torch.randn(M, Kd, generator=g, device="cuda", dtype=F32).to(BF16)
        B = torch.randn(Kd, N, generator=g, device="cuda", dtype=F32).to(BF16)
        aux = torch.randn(M, N, generator=g, device="cuda", dtype=F32).to(BF16)
        _CACHE[key] = (A, B, aux)
    return _CACHE[key]


def _patterns(M):
    """name -> uint8 [M] flags (CPU).  Rows come in samples of 128 = the row tiles of the 8-wave kernel; the 12-wave kernel's tile
    is two of them."""
    r = torch.arange(M)
    s, t = r // 128, r % 128
    lens = torch.tensor([37, 128, 90, 1, 64, 121, 8, 77])[s % 8]     # 37: the dead suffix starts inside a piece
    one = torch.zeros(M, dtype=torch.bool)
    one[13] = True                                                   # one live row inside an otherwise dead piece ...
    one[128 + 77::512] = True                                        # ... and in second halves of 256-row tiles further down
    return {
        "all_live": torch.ones(M, dtype=torch.uint8),
        "all_dead": torch.zeros(M, dtype=torch.uint8),
        "dead_suffix": (t < lens).to(torch.uint8),
        "one_live_row": one.to(torch.uint8),
        "alternating_pieces": ((r // PIECE) % 2 == 0).to(torch.uint8),
        "dead_tile_beside_live": (s % 2 == 1).to(torch.uint8),       # 12-wave kernel: the two 128-row halves differ
        "halves_differ": torch.where(s % 4 == 0, (t < 40), torch.where(s % 4 == 1, t >= 0, torch.where(s % 4 == 2, t < 0, t < 99))
                                     ).to(torch.uint8),
    }


PATTERN_NAMES = ("all_live", "all_dead", "dead_suffix", "one_live_row", "alternating_pieces", "dead_tile_beside_live", "halves_differ")


def _dead_piece_rows(flags):
    """bool [M]: rows of pieces without any live row (what a LIVE instance may skip)."""
    return (flags.view(-1, PIECE).max(dim=1).values == 0).repeat_interleave(PIECE)


def _launch(op, A, B, aux, epi, flags):
    M = A.shape[0]
    N = B.shape[1] if op == K.GEMM_NN else B.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda", dtype=BF16)
    kw = {}
    if epi == "add":
        kw = dict(epilogue=K.EPI_ADD, aux=aux)
    elif epi == "dgelu":
        kw = dict(epilogue=K.EPI_DGELU, aux=aux)
    K.gemm(op, A, B, out, a_live=flags, **kw)
    return out


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("kernel,Kd", [(k, kd) for k in ("ws96", "w3") for kd in KS[k]])
def test_live_launch_is_bitwise_the_plain_launch(kernel, Kd, epi):
    A0, B, aux = _operands(kernel, Kd)
    M = A0.shape[0]
    pats = _patterns(M)
    for name in PATTERN_NAMES:
        f = pats[name].cuda()
        A = A0 * f.to(BF16)[:, None]                                # flagged rows zeroed
        plain = _launch(K.GEMM_NN, A, B, aux, epi, None)
        live = _launch(K.GEMM_NN, A, B, aux, epi, f)
        torch.cuda.synchronize()
        assert not torch.isnan(plain.float()).any(), (name,)
        assert torch.equal(_bits(plain), _bits(live)), (kernel, Kd, epi, name, (plain.float() - live.float()).abs().max().item())


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("kernel", ["ws96", "w3"])
def test_dead_pieces_are_not_read(kernel, epi):
    """NaN in the rows of A that lie in pieces without a live row: the live launch equals the plain launch on the zeroed A in every
    row (dead rows = the epilogue of +0, live rows unchanged); the plain launch on the poisoned A does not -- so the LIVE instance
    ran, not the fallback."""
    Kd = KS[kernel][-1]
    A0, B, aux = _operands(kernel, Kd)
    M = A0.shape[0]
    pats = _patterns(M)
    for name in ("dead_suffix", "one_live_row", "alternating_pieces", "dead_tile_beside_live", "halves_differ", "all_dead"):
        f = pats[name]
        dead = _dead_piece_rows(f).cuda()
        assert int(dead.sum()) > 0
        fz = f.cuda()
        A = A0 * fz.to(BF16)[:, None]
        want = _launch(K.GEMM_NN, A, B, aux, epi, None)
        Ap = A.clone()
        Ap[dead] = float("nan")
        got = _launch(K.GEMM_NN, Ap, B, aux, epi, fz)
        full = _launch(K.GEMM_NN, Ap, B, aux, epi, None)
        torch.cuda.synchronize()
        assert not torch.isnan(want.float()).any()
        assert torch.equal(_bits(want), _bits(got)), (kernel, epi, name)
        zero = torch.zeros(1, B.shape[1], device="cuda", dtype=F32)
        if epi == "none":
            assert int((_bits(got[dead]) != 0).sum()) == 0          # +0 exactly, sign included
        elif epi == "add":
            assert torch.equal(_bits(got[dead]), _bits((zero + aux[dead].float()).to(BF16)))
        assert torch.isnan(full[dead].float()).all() and not torch.isnan(full[~dead].float()).any()


def test_launches_without_a_live_instance_fall_back():
    """Flags on a launch the ladder sends elsewhere (128-wide tiles, the NT layout, the general path) change nothing."""
    g = torch.Generator(device="cuda").manual_seed(99)
    for op, M, N, Kd in ((K.GEMM_NN, 256, 512, 128), (K.GEMM_NT, 256, 768, 128), (K.GEMM_NN, 200, 100, 70)):
        A = torch.randn(M, Kd, generator=g, device="cuda", dtype=F32).to(BF16)
        B = torch.randn(*((Kd, N) if op == K.GEMM_NN else (N, Kd)), generator=g, device="cuda", dtype=F32).to(BF16)
        aux = torch.randn(M, N, generator=g, device="cuda", dtype=F32).to(BF16)
        f = (torch.arange(M, device="cuda") % 128 < 37).to(torch.uint8)
        A = A * f.to(BF16)[:, None]
        plain = _launch(op, A, B, aux, "add", None)
        live = _launch(op, A, B, aux, "add", f)
        torch.cuda.synchronize()
        assert torch.equal(_bits(plain), _bits(live)), (op, M, N, Kd)


def test_flag_argument_checks():
    A = torch.zeros(256, 64, device="cuda", dtype=BF16)
    B = torch.zeros(64, 768, device="cuda", dtype=BF16)
    out = torch.zeros(256, 768, device="cuda", dtype=BF16)
    ok = torch.ones(256, device="cuda", dtype=torch.uint8)
    with pytest.raises(ValueError):
        K.gemm(K.GEMM_NN, A, B, out, a_live=ok[:255])                                  # numel != M
    with pytest.raises(ValueError):
        K.gemm(K.GEMM_NN, A, B, out, a_live=ok.to(torch.int32))                        # not uint8
    with pytest.raises(ValueError):
        K.gemm(K.GEMM_NN, A, B, out, a_live=torch.ones(512, device="cuda", dtype=torch.uint8)[::2])   # not contiguous
    with pytest.raises(ValueError):
        K.gemm(K.GEMM_TN, torch.zeros(64, 256, device="cuda", dtype=BF16), B, torch.zeros(256, 768, device="cuda", dtype=F32),
               a_live=ok)                                                              # flags are per row of a row-major A


# ------------------------------------------------------------------------------------------------------- layer level
LENS = (128, 70, 64, 33)


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


def _run_layers(precision, valid_only, dgrad_on, monkeypatch):
    """One train-mode forward + backward of a fresh copy; returns (gradients, the flag tensors the GEMM launches got)."""
    from icka_amd.arena import arena_of
    base, x = _base_model()
    m = icka_amd.set_precision(copy.deepcopy(base).cuda().train(), precision)
    valid = (torch.arange(128)[None, :] < torch.tensor(LENS)[:, None]).float()
    ext = ((1.0 - valid) * -10000.0)[:, None, None, :].cuda()
    seen = []
    real = K.gemm

    def spy(op, A, B, out, **kw):
        if kw.get("a_live") is not None:
            seen.append(kw["a_live"].clone())
        return real(op, A, B, out, **kw)

    monkeypatch.setattr(K, "gemm", spy)
    monkeypatch.setattr(ops, "WGRAD_LIVE", True)
    monkeypatch.setattr(ops, "DGRAD_LIVE", dgrad_on)
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
    monkeypatch.setattr(K, "gemm", real)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads["input"] = xi.grad.detach().clone()
    return grads, seen


@pytest.mark.parametrize("precision,valid_only", [("bf16", True), ("bf16", False), ("mixed16", True), ("mixed16", False)])
def test_layer_gradients_are_bitwise_equal_with_and_without_dgrad_live(precision, valid_only, monkeypatch):
    on, seen_on = _run_layers(precision, valid_only, True, monkeypatch)
    off, seen_off = _run_layers(precision, valid_only, False, monkeypatch)
    assert not seen_off                                           # the switch really turns the flags off
    assert len(seen_on) == 8                                      # four input-gradient GEMMs in each of the two layers
    dead = [int(_dead_piece_rows(f.cpu()).sum()) // PIECE for f in seen_on]
    print("\n[%s valid_only=%s] dead 8-row pieces per input-gradient GEMM (of 64): %s" % (precision, valid_only, dead))
    if valid_only:
        # lengths 128 / 70 / 64 / 33: 7 + 8 + 11 whole pieces behind the last valid token
        assert all(d >= 26 for d in dead), dead
    else:
        assert all(d == 0 for d in dead), dead                    # masked rows carry gradient: nothing may be skipped
    assert sorted(on) == sorted(off)
    for k in on:
        assert torch.equal(on[k], off[k]), (k, (on[k].float() - off[k].float()).abs().max().item())
        assert torch.isfinite(on[k].float()).all(), k
