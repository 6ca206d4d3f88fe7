"""GPU: the auxiliary training objective of the gated taggers (aux_losses=True; csrc/objective.hip).

1. the contrastive kernels against the float64 oracle (tests/objective_oracle.py) on the same rounded inputs;
2. the swap and ReLU-backward kernels against their torch restatements, bitwise;
3. the model against the reference's own loss and gradients (tests/golden/objective_*.npz) in bf16, mixed16 and fp32;
4. the defaults unchanged; 5. missing arguments refused; 6. the objective under graph.GraphedModule."""
import copy
import os

import numpy as np
import pytest
import torch

import icka_amd
import objective_oracle as OO
from icka_amd import kernels as K
from icka_amd import synth
from golden_util import GOLDEN_DIR, _sample, load_case

pytestmark = pytest.mark.gpu

GRAD_BARS = (1.1e-2, 1.6e-2)        # tests/test_model_gpu.py GRAD_BARS["tiny_gatecl_s128"]
# The bias gradients of the projection heads and of the pooler are sums over the batch of gradients that nearly cancel (with the
# seeded weights the projected rows are close to their biases, so the cosines differ little between pairs): in the 16-bit modes
# they carry the trunk's bf16 rounding at up to 1.6e-2 (norm) / 1.5e-1 (tensor) relative, measured on MI355X.  The fp32 mode
# pins them at 1e-3 (measured <= 2.6e-5); every other gradient is held to GRAD_BARS.
CANCELLING = tuple(h + ".bias" for h in ("text_dense_cl", "text_ouput_cl", "image_dense_cl", "image_output_cl")) + \
    ("bert.pooler.dense.bias",)
CANCELLING_BARS = (3e-2, 2.5e-1)
LOSS_BAR_KERNEL = 1e-4    # f32 cosines over D <= 1024 products: measured <= 5.6e-5 relative (gradients: <= 2.3e-5, bar 1e-4)
HEADS = ("text_dense_cl", "text_ouput_cl", "image_dense_cl", "image_output_cl")
GATECL = ["objective_gatecl_b8_n%s" % s for s in ("none", "0", "4", "3", "8")] + ["objective_gatecl_b8_tl0",
                                                                                 "objective_gatecl_b8_tl1"]


# ------------------------------------------------------------------------------------------------ 1. kernels vs the oracle
def _kernel_run(t, v, temp, tl):
    B, _ = t.shape
    stats = torch.empty(2, dtype=torch.float32, device="cuda")
    ws = K.contrastive_workspace(B, t.device)
    K.contrastive_fwd(t, v, temp, tl, stats, ws)
    dcl = torch.full((1,), 1.0, dtype=torch.float32, device="cuda")
    dt = torch.empty(t.shape, dtype=torch.float32, device="cuda")
    dv = torch.empty_like(dt)
    K.contrastive_bwd(t, v, temp, tl, ws, dcl, dt, dv)
    return stats[0].clone(), dt, dv


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 2, 7, 32, 64, 256])
def test_contrastive_kernels_match_float64_oracle(B, dtype):
    worst_l, worst_g = 0.0, 0.0
    for D in (64, 768, 1024):
        g = torch.Generator().manual_seed(B * 7919 + D)
        t = torch.randn(B, D, generator=g).to(dtype)
        v = (0.5 * torch.randn(B, D, generator=g) + 0.3 * t.float()).to(dtype)    # correlated pairs: a non-trivial softmax
        tc, vc = t.cuda(), v.cuda()
        t64, v64 = t.double(), v.double()
        for temp in (0.05, 0.179, 1.0):
            for tl in (0.0, 0.7, 1.0):
                loss, dt, dv = _kernel_run(tc, vc, temp, tl)
                ref = OO.cl_loss(t64, v64, temp, tl).item()
                rdt, rdv = OO.cl_grad(t64, v64, temp, tl)
                if B == 1:
                    assert loss.item() == 0.0 and dt.abs().max().item() == 0.0 and dv.abs().max().item() == 0.0
                    continue
                el = abs(loss.item() - ref) / abs(ref)
                eg = max(((dt.double().cpu() - rdt).norm() / rdt.norm()).item(),
                         ((dv.double().cpu() - rdv).norm() / rdv.norm()).item())
                worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
                assert el <= LOSS_BAR_KERNEL, (D, temp, tl, el)
                assert eg <= 1e-4, (D, temp, tl, eg)
        loss2, dt2, dv2 = _kernel_run(tc, vc, 0.179, 0.7)        # two runs: bitwise
        loss1, dt1, dv1 = _kernel_run(tc, vc, 0.179, 0.7)
        assert torch.equal(loss1, loss2) and torch.equal(dt1, dt2) and torch.equal(dv1, dv2)
    print("\n[B=%d %s] worst loss rel err %.2e, worst grad rel L2 %.2e" % (B, dtype, worst_l, worst_g))


def test_contrastive_shapes_outside_the_limits_are_refused():
    lib = K._lib.load()
    buf = torch.zeros(300 * 4104, dtype=torch.float32, device="cuda")
    stats = torch.empty(2, dtype=torch.float32, device="cuda")
    ws = torch.empty(300 * 300 + 6 * 300, dtype=torch.float32, device="cuda")
    s = K._stream()
    for B, D in ((257, 64), (0, 64), (4, 4104), (4, 12), (4, 0)):
        rc = lib.icka_contrastive_fwd(buf.data_ptr(), max(D, 8), buf.data_ptr(), max(D, 8), 0, B, D, 0.179, 0.7, None, 0,
                                      stats.data_ptr(), ws.data_ptr(), s)
        assert rc == -1, (B, D, rc)     # ICKA_E_SHAPE, nothing launched
        if B >= 1:
            t = buf[:B * D].view(B, D) if D > 0 else buf[:B].view(B, 1)
            with pytest.raises(ValueError):
                K.contrastive_fwd(t, t, 0.179, 0.7, stats, ws)


# ------------------------------------------------------------------------------------------------ 2. swap and ReLU backward
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("B,n", [(8, 4), (8, 3), (8, 8), (32, 16), (5, 1)])
def test_sample_swap_is_the_permutation(B, n, dtype):
    x = torch.randn(B * 16, 24, device="cuda").to(dtype)
    y = K.sample_swap(x, torch.empty_like(x), B, n)
    ref = OO.swap(x.view(B, 16, 24).cpu(), n).view(B * 16, 24)
    assert torch.equal(y.cpu(), ref)
    assert torch.equal(K.sample_swap(y, torch.empty_like(y), B, n), x)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_relu_backward_is_the_masked_gradient(dtype):
    y = torch.relu(torch.randn(1000, 37, device="cuda")).to(dtype)
    y.view(-1)[::7] = 0
    dy = torch.randn(1000, 37, device="cuda").to(dtype)
    dx = K.relu_bwd(dy, y, torch.empty_like(dy))
    assert torch.equal(dx, torch.where(y > 0, dy, torch.zeros_like(dy)))
    x = torch.randn(999, device="cuda").to(dtype)
    assert torch.equal(K.relu_bwd(x, x, torch.empty_like(x)), torch.relu(x))


# ------------------------------------------------------------------------------------------------ 3. model vs the reference
def _ref_state_dict(z):
    """The reference's full state_dict of the fixture, regenerated from synth.seeded_tensor and checked against its samples."""
    sd = {}
    for k, shp, smp in zip(z["sd_names"], z["sd_shapes"], z["sd_samples"]):
        k, shape = str(k), tuple(int(d) for d in str(shp).split(",") if d)
        sd[k] = synth.seeded_tensor(k, shape)
        np.testing.assert_array_equal(np.resize(_sample(sd[k], 16), 16), smp)
    return sd


def _model(case, z, aux=True, use_crf=True):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = case["cfg"]
    c = BertConfig(cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                   num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                   max_position_embeddings=cfg["max_position_embeddings"], type_vocab_size=cfg["type_vocab_size"])
    m = MTCCMBertForMMTokenClassificationCRF(c, layer_num1=cfg["layer_num1"], num_labels=cfg["num_labels"], variant=case["variant"],
                                             max_seq_length=case["batch"]["input_ids"].shape[1], use_crf=use_crf, aux_losses=aux)
    missing, unexpected = m.load_state_dict(_ref_state_dict(z), strict=False)
    return m.cuda().eval(), missing, unexpected


def _args(case, z):
    g = {k: v.cuda() for k, v in case["batch"].items()}
    temp, tl, lamb, nr, _n = z["meta_objective"]
    return g, dict(temp=float(temp), temp_lamb=float(tl), lamb=float(lamb), negative_rate=None if nr < 0 else int(nr))


def _loss(model, g, kw, variant):
    if variant == "gate_cl":
        return model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                     g["visual_embeds_att"], kw["temp"], kw["temp_lamb"], kw["lamb"], g["labels"], kw["negative_rate"])
    return model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                 g["visual_embeds_att"], temp=kw["temp"], temp_lamb=kw["temp_lamb"], labels=g["labels"])


@pytest.mark.parametrize("precision", ["bf16", "mixed16", "fp32"])
@pytest.mark.parametrize("name", GATECL + ["objective_cl_b4_s32"])
def test_objective_matches_reference_fixture(name, precision):
    case = load_case(name)
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    model, _, _ = _model(case, z)
    icka_amd.set_precision(model, precision)
    g, kw = _args(case, z)
    model.zero_grad()
    loss = _loss(model, g, kw, case["variant"])
    loss.backward()
    ref = float(z["loss"][0])
    el = abs(loss.item() - ref) / abs(ref)
    params = dict(model.named_parameters())
    gmax = float(z["grad_norms"].max())
    worst_n, worst_t, key_n, key_t = 0.0, 0.0, "", ""
    canc_n, canc_t = 0.0, 0.0
    seen = set()
    for n, gn in zip([str(x) for x in z["grad_names"]], z["grad_norms"]):
        if gn == 0.0:
            continue
        assert n in params, n
        gr = params[n].grad
        assert gr is not None, n
        seen.add(n)
        rel = abs(gr.float().norm().item() - gn) / (gn + 1e-4 * gmax)
        e = 0.0
        if "grad/" + n in z.files:
            r = torch.from_numpy(z["grad/" + n])
            e = ((gr.float().cpu() - r).norm() / (r.norm() + 1e-4 * gmax)).item()
        if n in CANCELLING and precision != "fp32":
            canc_n, canc_t = max(canc_n, rel), max(canc_t, e)
            continue
        if rel > worst_n:
            worst_n, key_n = rel, n
        if e > worst_t:
            worst_t, key_t = e, n
    for n in ("bert.pooler.dense.weight", "bert.pooler.dense.bias") + tuple(h + s for h in HEADS for s in (".weight", ".bias")) + \
            (("crs_classifier.weight", "crs_classifier.bias") if case["variant"] == "gate_cl" else ()):
        assert n in seen, n
    print("\n[%s %s] loss %.6f vs %.6f (rel %.2e); worst grad-norm err %.2e at %s; worst grad-tensor rel L2 %.2e at %s; "
          "cancelling biases %.2e / %.2e" % (name, precision, loss.item(), ref, el, worst_n, key_n, worst_t, key_t, canc_n, canc_t))
    assert canc_n <= CANCELLING_BARS[0] and canc_t <= CANCELLING_BARS[1], (canc_n, canc_t)
    bars = (1e-3, 1e-3, 1e-3) if precision == "fp32" else (2e-2,) + GRAD_BARS
    assert el <= bars[0], el
    assert worst_n <= bars[1], (key_n, worst_n)
    assert worst_t <= bars[2], (key_t, worst_t)


# ------------------------------------------------------------------------------------------------ 4. defaults unchanged
def test_defaults_unchanged_and_reference_checkpoint_loads():
    name = "objective_gatecl_b8_n4"
    case = load_case(name)
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    plain, _, _ = _model(case, z, aux=False, use_crf=False)
    aux, missing, unexpected = _model(case, z, aux=True, use_crf=True)
    assert missing == []
    assert unexpected and all(k.startswith("self_attention") for k in unexpected), unexpected
    heads = {h + s for h in HEADS for s in (".weight", ".bias")}
    crf = {"crf.start_transitions", "crf.end_transitions", "crf.transitions"}
    assert set(aux.state_dict()) == set(plain.state_dict()) | heads | crf
    assert not any("_cl." in k for k in plain.state_dict())
    g, _kw = _args(case, z)
    with torch.no_grad():
        a = plain(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                  g["visual_embeds_att"])
        aux.crf = None
        b = aux(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                g["visual_embeds_att"])
    assert torch.equal(a, b)
    la = plain.logits(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_att"])
    lb = aux.logits(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_att"])
    assert torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------ 5. missing arguments
@pytest.mark.parametrize("missing", ["temp", "temp_lamb", "lamb"])
def test_missing_objective_arguments_raise(missing):
    name = "objective_gatecl_b8_n4"
    case = load_case(name)
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    model, _, _ = _model(case, z)
    g, kw = _args(case, z)
    kw[missing] = None
    with pytest.raises(ValueError, match=missing):
        _loss(model, g, kw, "gate_cl")


# ------------------------------------------------------------------------------------------------ 6. capture
def test_objective_under_graphed_module_matches_eager():
    from icka_amd.config import BertConfig
    from icka_amd.graph import GraphedModule
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=128, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, variant="gate_cl", max_seq_length=64,
                                                regions=49, use_crf=True, aux_losses=True)
    synth.fill_module_(base)
    base = base.cuda().train()
    eager = copy.deepcopy(base)
    graphed = copy.deepcopy(base)

    def batch(seed, temp):
        b = {k: v.cuda() for k, v in synth.synthetic_batch(8, 64, 49, vocab_size=512, seed=seed).items()}
        return (b["input_ids"], b["segment_ids"], b["input_mask"], b["added_attention_mask"], b["visual_embeds_mean"],
                b["visual_embeds_att"], temp, 0.7, 0.62, b["labels"], 4)

    gm = GraphedModule(graphed, batch(100, 0.179), {})
    for step, (seed, temp) in enumerate(((101, 0.179), (102, 0.179), (103, 0.179), (104, 0.5))):
        args = batch(seed, temp)
        eager.zero_grad()
        graphed.zero_grad()
        le = eager(*args)
        le.backward()
        lg = gm(*args)
        lg.backward()
        torch.cuda.synchronize()
        pe, pg = dict(eager.named_parameters()), dict(graphed.named_parameters())
        gmax = max(p.grad.norm().item() for p in pe.values() if p.grad is not None)
        worst, key, nonbit = 0.0, "", []
        for n, p in pe.items():
            if p.grad is None:
                continue
            assert pg[n].grad is not None, n
            if not torch.equal(p.grad, pg[n].grad):
                nonbit.append(n)
                # floor: 1e-4 of the largest gradient norm, as tests/test_model_gpu.py (the cross-attention key bias has an exactly
                # zero true gradient: what it holds is rounding noise)
                e = ((p.grad - pg[n].grad).norm() / (p.grad.norm() + 1e-4 * gmax)).item()
                if e > worst:
                    worst, key = e, n
        print("\n[capture step %d temp %.3f] loss eager %.7f graphed %.7f; %s; grads not bitwise: %s (worst rel L2 %.2e at %s)"
              % (step, temp, le.item(), lg.item(), gm.stats, nonbit, worst, key))
        assert torch.equal(le.detach(), lg.detach()), (le.item(), lg.item())
        # gradients: the same kernels in the same order, except for the f32 atomics some of the existing kernels accumulate with
        # (embedding tables, the CRF, split reductions): within 1e-3, the bar tests/test_whole_loop_gpu.py holds bf16 replays to
        assert worst <= 1e-3, (key, worst)
    assert gm.stats["eager_calls"] == 0 and gm.stats["captures"] == 2, gm.stats
    gm.close()
