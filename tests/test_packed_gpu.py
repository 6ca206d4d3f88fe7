"""GPU: packed (padding-free) token-budget batches.  In order: the plan kernel against its CPU restatement (so the row maps are
proven in bounds before any consumer reads them), the row gather, the varlen attention kernels against the padded ones, then
the model under set_packed against the fixtures and the padded HIP path, a graph capture, the overflow path and the
refusals."""
import copy

import numpy as np
import pytest
import torch

from icka_amd import kernels as K
from icka_amd import packing, synth
from icka_amd.packing import PackOverflowError, plan_reference, set_packed
from golden_util import load_case

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-2   # test_model_gpu.py
GRAD_BARS = {"tiny_cl_r49": (1.7e-2, 1.7e-2), "tiny_cl_masks": (1.6e-2, 1.6e-2),
             "base_cl_s64_r36": (2.6e-2, 2.6e-2), "base_cl_s128_r49": (2.6e-2, 2.6e-2)}
PACKED_VS_PADDED = 2e-3


def _mask(lens, S):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()


def _plan(mask, max_tokens):
    st = packing.PackState(max_tokens)
    p = st.plan(mask.cuda())
    torch.cuda.synchronize()
    return st, p


# ---------------------------------------------------------------------------------------------------- 1. plan kernel
@pytest.mark.parametrize("lens,S,max_tokens", [
    ([1, 128, 37, 64], 128, 256),            # length 1 and length S
    ([128, 128], 128, 256),                  # T == max_tokens
    ([3, 5], 64, 1024),                      # many filler rows
    ([100, 100, 100, 20], 128, 256),         # overflow
    ([0, 7, 0], 32, 128),                    # empty samples
])
def test_plan_kernel_matches_the_cpu_restatement(lens, S, max_tokens):
    mask = _mask(lens, S)
    st, p = _plan(mask, max_tokens)
    ref = plan_reference(mask, max_tokens)
    assert p.lens.cpu().tolist() == ref["lens"].tolist()
    assert p.cu.cpu().tolist() == ref["cu_seqlens"].tolist()
    assert torch.equal(p.p2p.cpu(), ref["packed_to_padded"])
    assert torch.equal(p.pad2pack.cpu(), ref["padded_to_packed"])
    assert torch.equal(p.cls_of.cpu(), ref["cls_of"])
    assert p.status.cpu().tolist() == ref["status"].tolist()
    assert p.pad2pack.max().item() < max_tokens and p.p2p.max().item() < len(lens) * S
    over = sum(lens) > max_tokens
    if over:
        with pytest.raises(PackOverflowError, match="%d valid tokens" % sum(lens)):
            st.check_error()
    st.check_error()   # cleared (or never set)


def test_plan_kernel_flags_a_mask_that_is_not_a_prefix():
    m = _mask([4, 4], 8)
    m[1, 6] = 1
    st, p = _plan(m, 128)
    assert p.status.cpu().tolist() == [8, 2]
    assert p.pad2pack[8 + 6].item() == -2
    with pytest.raises(PackOverflowError, match="prefix"):
        st.check_error()


# ---------------------------------------------------------------------------------------------------- 2. gather
@pytest.mark.parametrize("dtype,width", [(torch.bfloat16, 256), (torch.float32, 13), (torch.float32, 64)])
def test_rows_gather_is_exact(dtype, width):
    lens, S, T = [5, 1, 16, 9], 16, 128
    _, p = _plan(_mask(lens, S), T)
    x = torch.randn(len(lens) * S, width, device="cuda").to(dtype)
    packed = K.rows_gather(x, torch.full((T, width), 7, dtype=dtype, device="cuda"), p.p2p)
    p2p = p.p2p.cpu()
    xc, pc = x.cpu(), packed.cpu()
    for t in range(T):
        exp = xc[p2p[t]] if p2p[t] >= 0 else torch.zeros(width, dtype=dtype)
        assert torch.equal(pc[t], exp), t
    back = K.rows_gather(packed, torch.full_like(x, 7), p.pad2pack).cpu()
    valid = _mask(lens, S).reshape(-1).bool()
    assert torch.equal(back[valid], xc[valid]) and back[~valid].eq(0).all()
    if dtype == torch.float32:
        m = _mask([6, 6], 8)
        _, po = _plan(m, 128)
        po.pad2pack[8 + 2] = -2
        y = K.rows_gather(torch.ones(128, width, device="cuda"), torch.zeros(16, width, device="cuda"), po.pad2pack,
                          fill=packing.F32_NAN_WORD).cpu()
        assert torch.isnan(y[10]).all() and not torch.isnan(y[:10]).any()


# ---------------------------------------------------------------------------------------------------- 3. varlen attention
def _attn_case(self_attn, p_drop, keep, S=128, R=49, lens=(1, 128, 77, 40, 64, 9), heads=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, H = len(lens), 64 * heads
    T = (sum(lens) + 127) // 128 * 128 + 128            # plus a block of filler rows
    mask = _mask(list(lens), S)
    _, p = _plan(mask, T)
    dev = "cuda"
    bf = torch.bfloat16
    Skv = S if self_attn else R
    qkv = torch.randn(B * S, 3 * H, generator=g).to(bf).to(dev)
    kv = torch.randn(B * R, 2 * H, generator=g).to(bf).to(dev)
    dO = torch.randn(B * S, H, generator=g).to(bf).to(dev)
    dO[~mask.reshape(-1).bool().to(dev)] = 0          # pad queries get no gradient in the model either
    add_q = ((1 - mask).float() * -10000.0).to(dev)
    img = torch.ones(B, R, dtype=torch.long)
    img[:, R - 5:] = 0
    add_kv = add_q if self_attn else ((1 - img).float() * -10000.0).to(dev)
    seed_a = 1234
    kbw = lambda: K.attn_keepbits(B, heads, S, Skv, dev) if keep else None   # noqa: E731
    # padded reference
    q, k, v = (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]) if self_attn else (qkv[:, :H], kv[:, :H], kv[:, H:])
    ctx = torch.empty(B * S, H, dtype=bf, device=dev)
    lse = torch.empty(B, heads, S, dtype=torch.float32, device=dev)
    kb = kbw()
    K.attn_fwd(q, k, v, add_kv, ctx, lse, B, heads, S, Skv, p_drop=p_drop, seed=seed_a, keepbits=kb)
    dq, dk, dv = (torch.zeros(B * S, H, dtype=bf, device=dev), torch.zeros(k.shape[0], H, dtype=bf, device=dev),
                  torch.zeros(k.shape[0], H, dtype=bf, device=dev))
    K.attn_bwd(q, k, v, add_kv, ctx, dO, lse, torch.empty_like(lse), dq, dk, dv, B, heads, S, Skv, p_drop=p_drop,
               seed=seed_a, keepbits=kb)
    # packed, on buffers pre-filled with garbage (the kernels must write every row they own, filler rows included)
    junk = lambda *s: torch.full(s, 3.0, dtype=bf, device=dev)   # noqa: E731
    qkv_p = K.rows_gather(qkv, junk(T, 3 * H), p.p2p)
    dO_p = K.rows_gather(dO, junk(T, H), p.p2p)
    qp, kp, vp = (qkv_p[:, :H], qkv_p[:, H:2 * H], qkv_p[:, 2 * H:]) if self_attn else (qkv_p[:, :H], kv[:, :H], kv[:, H:])
    ctx_p = junk(T, H)
    lse_p = torch.empty_like(lse)
    kb_p = kbw()
    K.attn_fwd_packed(qp, kp, vp, add_kv, ctx_p, lse_p, p.cu, self_attn, B, heads, S, Skv, p_drop=p_drop, seed=seed_a,
                      keepbits=kb_p)
    dqkv_p = junk(T, 3 * H)
    if self_attn:
        dqp, dkp, dvp = dqkv_p[:, :H], dqkv_p[:, H:2 * H], dqkv_p[:, 2 * H:]
    else:
        dqp, dkp, dvp = junk(T, H), junk(B * R, H), junk(B * R, H)
    K.attn_bwd_packed(qp, kp, vp, add_kv, dO_p, lse_p, torch.empty_like(lse), dqp, dkp, dvp, p.cu, self_attn, B, heads, S,
                      Skv, p_drop=p_drop, seed=seed_a, keepbits=kb_p)
    torch.cuda.synchronize()
    return dict(p=p, T=T, lens=lens, S=S, ctx=ctx, lse=lse, dq=dq, dk=dk, dv=dv, ctx_p=ctx_p, lse_p=lse_p, dq_p=dqp,
                dk_p=dkp, dv_p=dvp)


@pytest.mark.parametrize("self_attn", [True, False])
@pytest.mark.parametrize("p_drop,keep", [(0.0, False), (0.1, False), (0.1, True)])
def test_varlen_attention_equals_the_padded_kernels_bitwise(self_attn, p_drop, keep):
    """Masked keys add exact zeros in both forms, and the dropout hash / keep bits use the padded coordinates, so every valid
    row is bit for bit the padded kernels' result."""
    c = _attn_case(self_attn, p_drop, keep)
    p, T = c["p"], c["T"]
    n = int(p.cu[-1].item())
    p2p = p.p2p[:n].long()
    for name in ("ctx", "dq"):
        assert torch.equal(c[name + "_p"][:n], c[name][p2p]), name
        assert c[name + "_p"][n:].eq(0).all(), name + ": filler rows must be exactly zero"
    for b, ln in enumerate(c["lens"]):
        assert torch.equal(c["lse_p"][b, :, :ln], c["lse"][b, :, :ln])
    if self_attn:
        for name in ("dk", "dv"):
            assert torch.equal(c[name + "_p"][:n], c[name][p2p]), name
            assert c[name + "_p"][n:].eq(0).all(), name
    else:
        for name in ("dk", "dv"):   # key rows b*R + r: every row of every sample
            assert torch.equal(c[name + "_p"], c[name]), name


def test_varlen_attention_short_sequences():
    c = _attn_case(True, 0.1, False, S=64, lens=(64, 1, 30, 33))
    n = int(c["p"].cu[-1].item())
    p2p = c["p"].p2p[:n].long()
    assert torch.equal(c["ctx_p"][:n], c["ctx"][p2p]) and torch.equal(c["dq_p"][:n], c["dq"][p2p])
    assert torch.equal(c["dk_p"][:n], c["dk"][p2p])


def test_varlen_attention_dropout_keep_rate_on_valid_rows():
    """p = 0.1: the keep bits the packed forward leaves for its valid (query, key < length) elements keep 90 % of them, within
    5 standard deviations of a Bernoulli(0.9) count."""
    lens, S, heads, p_drop = (128, 100, 77, 128, 64, 33, 120, 128), 128, 4, 0.1
    B, H = len(lens), 64 * heads
    T = (sum(lens) + 127) // 128 * 128
    mask = _mask(list(lens), S)
    _, p = _plan(mask, T)
    g = torch.Generator().manual_seed(3)
    qkv = K.rows_gather(torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16).cuda(),
                        torch.empty(T, 3 * H, dtype=torch.bfloat16, device="cuda"), p.p2p)
    add = ((1 - mask).float() * -10000.0).cuda()
    kb = torch.zeros(K._lib.load().icka_attn_keepbits_words(B, heads, S, S), dtype=torch.int32, device="cuda")
    ctx = torch.empty(T, H, dtype=torch.bfloat16, device="cuda")
    K.attn_fwd_packed(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], add, ctx, None, p.cu, True, B, heads, S, S, p_drop=p_drop,
                      seed=77, keepbits=kb)
    torch.cuda.synchronize()
    # layout: per (b*heads + head, query, g = (key % 16) / 4) one word (S <= 128), bit (key / 16) * 4 + key % 4
    words = kb.cpu().view(B, heads, S, 4).to(torch.int64) & 0xFFFFFFFF
    key = torch.arange(S)
    bits = (words[..., (key % 16) // 4] >> ((key // 16) * 4 + key % 4)) & 1          # [B, heads, S(query), S(key)]
    valid = torch.zeros(B, 1, S, S, dtype=torch.bool)
    for b, ln in enumerate(lens):
        valid[b, 0, :ln, :ln] = True
    valid = valid.expand(B, heads, S, S)
    n = int(valid.sum())
    kept = int(bits[valid].sum())
    rate, sd = kept / n, (0.9 * 0.1 / n) ** 0.5
    print("\n[keep rate] %.5f over %d valid elements (expected 0.9 +- %.5f)" % (rate, n, sd))
    assert abs(rate - (1 - p_drop)) < 5 * sd, rate
    assert torch.isfinite(ctx.float()).all() and ctx[int(p.cu[-1]):].eq(0).all()


# ---------------------------------------------------------------------------------------------------- 4. model, eval
def _build(cfg, regions, **kw):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    c = BertConfig(cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                   num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                   max_position_embeddings=cfg["max_position_embeddings"], type_vocab_size=cfg["type_vocab_size"])
    m = MTCCMBertForMMTokenClassificationCRF(c, layer_num1=cfg["layer_num1"], num_labels=cfg["num_labels"], regions=regions,
                                             variant="cl", **kw)
    synth.fill_module_(m)
    return m.cuda()


def _run(model, g, labels=True, **kw):
    return model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                 g["visual_embeds_att"], labels=g["labels"] if labels else None, **kw)


def _grads(model):
    return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _compare_grads(ga, gb, bar, what):
    gmax = max(g.norm().item() for g in gb.values())
    worst, key = 0.0, ""
    for n, g in gb.items():
        e = ((ga[n] - g).norm() / (g.norm() + 1e-4 * gmax)).item()
        if e > worst:
            worst, key = e, n
    print("[%s] worst gradient rel-L2 packed vs padded %.3e at %s (bar %.0e)" % (what, worst, key, bar))
    assert worst <= bar, (key, worst)


@pytest.mark.parametrize("name", ["tiny_cl_r49", "tiny_cl_masks", "base_cl_s64_r36", "base_cl_s128_r49"])
@pytest.mark.parametrize("budget", ["tokens", "padded"])
def test_packed_model_matches_fixture_and_padded_path(name, budget):
    case = load_case(name)
    exp = case["expected"]
    base = _build(case["cfg"], case["cfg"]["regions"]).eval()
    g = {k: v.cuda() for k, v in case["batch"].items()}
    B, S = g["input_ids"].shape
    ntok = int(g["input_mask"].sum().item())
    max_tokens = (ntok + 127) // 128 * 128 if budget == "tokens" else (B * S + 127) // 128 * 128
    padded, packed = base, set_packed(copy.deepcopy(base), max_tokens)
    lp = _run(padded, g, labels=False)
    lk = _run(packed, g, labels=False)
    valid = g["input_mask"].bool()
    assert lk.dtype == torch.float32 and lk.shape == lp.shape
    assert lk[~valid].eq(0).all(), "pad logits must be exactly 0"
    err_ref = np.abs(lk.detach().cpu().numpy() - exp["logits"])[valid.cpu().numpy()].max()
    err_pad = (lk - lp).abs()[valid].max().item()
    print("\n[%s, %s] logits vs fixture %.3e, vs padded HIP %.3e" % (name, budget, err_ref, err_pad))
    assert err_ref < LOGIT_TOL and err_pad <= PACKED_VS_PADDED
    for m in (padded, packed):
        m.zero_grad()
    loss_p = _run(padded, g)
    loss_k = _run(packed, g)
    assert abs(loss_k.item() - float(exp["loss"][0])) < LOGIT_TOL
    assert abs(loss_k.item() - loss_p.item()) <= PACKED_VS_PADDED * max(1.0, abs(loss_p.item()))
    loss_p.backward()
    loss_k.backward()
    params = dict(packed.named_parameters())
    gmax = float(exp["grad_norms"].max())
    worst = 0.0
    for n, gn in zip([str(x) for x in exp["grad_names"]], exp["grad_norms"]):
        if n in params and gn != 0.0:
            worst = max(worst, abs(params[n].grad.float().norm().item() - gn) / (gn + 1e-4 * gmax))
    assert worst < GRAD_BARS[name][0], worst
    _compare_grads(_grads(packed), _grads(padded), PACKED_VS_PADDED, name)


# ---------------------------------------------------------------------------------------------------- 5.-6. train mode
def _train_batch(B=6, S=64, R=49, seed=5, vocab=512):
    b = synth.synthetic_batch(B, S, R, vocab_size=vocab, seed=seed, layout="BRC")
    b["visual_embeds_mean"] = b["visual_embeds_att"].mean(dim=1)
    return {k: v.cuda() for k, v in b.items()}


def _small_model(aux=False, crf=False, p=0.1):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=128, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=7, aux_losses=aux, use_crf=crf)
    synth.fill_module_(m)
    return m.cuda()


def _objective(model, g, aux):
    kw = dict(temp=0.179, temp_lamb=0.7) if aux else {}
    return _run(model, g, **kw)


@pytest.mark.parametrize("aux,crf", [(False, False), (False, True), (True, False)])
def test_train_mode_without_dropout_matches_padded(aux, crf):
    base = _small_model(aux, crf, p=0.0).train()
    packed = set_packed(copy.deepcopy(base), 512)
    g = _train_batch()
    lp, lk = _objective(base, g, aux), _objective(packed, g, aux)
    assert abs(lk.item() - lp.item()) <= PACKED_VS_PADDED * max(1.0, abs(lp.item())), (lk.item(), lp.item())
    lp.backward()
    lk.backward()
    _compare_grads(_grads(packed), _grads(base), PACKED_VS_PADDED, "train aux=%s crf=%s" % (aux, crf))


def test_train_mode_with_dropout_is_deterministic_and_drops():
    base = _small_model(p=0.1).train()
    a, b = set_packed(copy.deepcopy(base), 512), set_packed(copy.deepcopy(base), 512)
    g = _train_batch()
    la, lb = _run(a, g), _run(b, g)
    la.backward()
    lb.backward()
    assert la.item() == lb.item()
    ga, gb = _grads(a), _grads(b)
    for n in ga:   # the embedding tables accumulate by f32 atomics: equal up to summation order (the graph tests' 1e-3 rule)
        assert (ga[n] - gb[n]).abs().max().item() <= 1e-3 * max(1.0, gb[n].abs().max().item()), n
    le = _run(set_packed(copy.deepcopy(base), 512).eval(), g)
    assert la.item() != le.item() and np.isfinite(la.item())


# ---------------------------------------------------------------------------------------------------- 7. graph capture
def test_one_graph_capture_serves_batches_of_different_lengths():
    from icka_amd import GraphedModule
    base = _small_model(p=0.0).train()
    eager = set_packed(copy.deepcopy(base), 384)
    graphed_model = set_packed(copy.deepcopy(base), 384)
    batches = [_train_batch(B=6, S=64, seed=s) for s in (11, 12, 13)]
    batches[2]["input_mask"][0] = 0          # an empty sample (how a short batch is brought to the captured B)
    batches[2]["labels"][0] = 0
    args = lambda g: (g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"],   # noqa: E731
                      g["visual_embeds_mean"], g["visual_embeds_att"])
    gm = GraphedModule(graphed_model, args(batches[0]), {"labels": batches[0]["labels"]})
    for g in batches:
        eager.zero_grad()
        gm.zero_grad()
        le = _run(eager, g)
        le.backward()
        lg = gm(*args(g), labels=g["labels"])
        lg.backward()
        torch.cuda.synchronize()
        assert le.item() == lg.item(), (le.item(), lg.item())
        ge, gg = _grads(eager), _grads(graphed_model)
        for n in ge:
            assert (ge[n] - gg[n]).abs().max().item() <= 1e-3 * max(1.0, ge[n].abs().max().item()), n
    print("\n[graph] %s" % gm.stats)
    assert gm.stats["captures"] == 1, gm.stats
    gm.close()


# ---------------------------------------------------------------------------------------------------- 8. overflow
def test_overflow_gives_nan_then_error_then_recovers():
    base = _small_model(p=0.0).eval()
    packed = set_packed(copy.deepcopy(base), 128)
    g = _train_batch(B=6, S=64)                      # > 128 valid tokens
    assert g["input_mask"].sum().item() > 128
    loss = _run(packed, g)
    torch.cuda.synchronize()
    assert torch.isnan(loss).item()
    with pytest.raises(PackOverflowError, match="%d valid tokens" % int(g["input_mask"].sum().item())):
        _run(packed, g)
    small = {k: v[:2].clone() for k, v in g.items()}
    small["input_mask"][:, 50:] = 0
    small["labels"][:, 50:] = 0
    assert small["input_mask"].sum().item() <= 128
    lk = _run(packed, small)
    lp = _run(base, small)
    assert abs(lk.item() - lp.item()) <= PACKED_VS_PADDED * max(1.0, abs(lp.item()))


def test_a_copied_packed_model_reports_its_own_overflow():
    """copy.deepcopy of a packed model that has run: the copy gets a pinned error word of its own (the original's is not shared
    and not copied into pageable memory), and its overflow is reported by the copy alone."""
    base = _small_model(p=0.0).eval()
    m = set_packed(copy.deepcopy(base), 128)
    small = {k: v[:2].clone() for k, v in _train_batch(B=6, S=64).items()}
    small["input_mask"][:, 50:] = 0
    small["labels"][:, 50:] = 0
    l0 = _run(m, small)
    m2 = copy.deepcopy(m)
    assert packing.state_of(m2) is not packing.state_of(m) and packing.state_of(m2)._err is None
    big = _train_batch(B=6, S=64)
    assert torch.isnan(_run(m2, big)).item()
    assert packing.state_of(m2)._err.is_pinned()
    with pytest.raises(PackOverflowError):
        _run(m2, small)
    assert _run(m, small).item() == l0.item()               # the original saw no error
    assert _run(m2, small).item() == l0.item()


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_unsupported_modes_refuse_and_unpacking_restores_the_padded_path():
    from icka_amd import set_precision
    from icka_amd.graph import FlaggedStep, SegmentedStep
    m = _small_model(p=0.0).eval()
    g = _train_batch(B=2, S=128)
    l0 = _run(m, g, labels=False)
    set_packed(m, 512)
    for prec in ("fp32", "mixed16"):
        set_precision(m, prec)
        with pytest.raises(NotImplementedError, match=prec):
            _run(m, g, labels=False)
    set_precision(m, "bf16")
    long = _train_batch(B=1, S=256)
    with pytest.raises(NotImplementedError, match="S=256"):
        _run(m, long, labels=False)
    with pytest.raises(NotImplementedError, match="FlaggedStep"):
        FlaggedStep(m, lambda: None, reducer=None)
    with pytest.raises(NotImplementedError, match="SegmentedStep"):
        SegmentedStep(m, lambda: None, reducer=None)
    from icka_amd.graph import GraphedModule, build_step
    with pytest.raises(NotImplementedError, match=r"build_step\(reducer=\)"):
        build_step(m, lambda: None, reducer=object())
    with pytest.raises(NotImplementedError, match=r"GraphedModule\(reducer=\)"):
        GraphedModule(m, (), {}, reducer=object())
    set_packed(m, None)
    l1 = _run(m, g, labels=False)
    assert torch.equal(l0, l1)
