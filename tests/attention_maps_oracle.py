"""Float64 restatement of the attention maps of the MNER trunk: softmax(Q.K^T / sqrt(d) + mask) per attention module, built from
oracle.mner_oracle's own pieces (dense, _split_heads, the layer functions).  Shared by the CPU and GPU attention-map tests."""
from __future__ import annotations

import math
import os
from typing import Dict

import numpy as np
import torch

from oracle import mner_oracle as O

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_maps_tiny.npz")


def probs(P, prefix, q_src, kv_src, add_mask, cfg) -> torch.Tensor:
    """attention_probs of BertSelfAttention / BertCoAttention before dropout, [B,heads,Sq,Skv]."""
    h = cfg.num_attention_heads
    q = O._split_heads(O.dense(q_src, P, prefix + ".query"), h)
    k = O._split_heads(O.dense(kv_src, P, prefix + ".key"), h)
    return torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(cfg.hidden_size // h) + add_mask, dim=-1)


def trunk_maps(P, cfg, batch, layer_num1: int, regions: int) -> Dict[str, torch.Tensor]:
    """{module name: maps} of mner_oracle.mner_trunk in eval mode; P in float64."""
    f64 = torch.float64
    add = O.additive_mask(batch["input_mask"], f64)
    x = O.embeddings(P, "bert.embeddings", batch["input_ids"], batch["segment_ids"], cfg, False)
    maps = {}
    for i in range(cfg.num_hidden_layers):
        pre = "bert.encoder.layer.%d" % i
        maps[pre + ".attention.self"] = probs(P, pre + ".attention.self", x, x, add, cfg)
        x = O.bert_layer(P, pre, x, add, cfg, False)
    vis = O.dense(O.region_tokens(batch["visual_embeds_att"].to(f64), regions), P, "vismap2text")
    img_add = O.additive_mask(batch["added_attention_mask"][:, :regions], f64)
    for j in range(layer_num1):
        pre = "txt2img_attention.layer.%d" % j
        maps[pre + ".attention.self"] = probs(P, pre + ".attention.self", x, vis, img_add, cfg)
        x = O.cross_layer(P, pre, x, vis, img_add, cfg, False)
    return maps


def scale_qk_(model, factor: float) -> None:
    """What the fixture script did to the reference: query / key WEIGHTS of every attention module times ``factor``."""
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "query") and hasattr(m, "key"):
                m.query.weight.mul_(factor)
                m.key.weight.mul_(factor)


_CASE = None


def load_fixture():
    """(golden_util case, {"all/<name>" | "mean/<name>": array}, names, qk scale) -- loaded once, shared, never modified."""
    global _CASE
    if _CASE is None:
        from golden_util import load_case
        case = load_case("attention_maps_tiny")
        exp = case["expected"]
        for v in exp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASE = (case, exp, [str(n) for n in exp["names"]], float(exp["qk_scale"][0]))
    return _CASE


# ---------------------------------------------------------------------------------------------- shared by the GPU tests and
# tools/attention_maps_bench.py (which reports the error maxima of exactly these inputs)
def _K():
    from icka_amd import kernels
    return kernels


KERNEL_SHAPES = [(3, 2, 32, 32), (2, 3, 80, 80), (2, 2, 32, 49), (2, 2, 32, 36), (3, 2, 1, 32), (1, 2, 144, 144), (1, 1, 256, 256),
          (1, 1, 40, 512)]
GUARD = 64
SENTINEL = 12345.0


def kernel_case(B, heads, Sq, Skv, seed=0):
    """bf16 q / k as column slices of wider token-major buffers (unit-order scores at scale 1/8), an additive mask with a
    partial, an all-masked and a one-key sample as far as B allows."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Sq + Skv)
    H = heads * 64
    qb = torch.empty(B * Sq, H + 64).normal_(0, 1, generator=g).to(torch.bfloat16)
    kb = torch.empty(B * Skv, 2 * H).normal_(0, 1, generator=g).to(torch.bfloat16)
    m01 = torch.ones(B, Skv)
    kinds = {1: ["partial"], 2: ["onekey", "allmasked"], 3: ["partial", "allmasked", "onekey"]}[B]
    for b, kind in enumerate(kinds):
        if kind == "partial":
            m01[b, Skv - Skv // 3:] = 0
        elif kind == "allmasked":
            m01[b] = 0
        else:
            m01[b] = 0
            m01[b, Skv // 2] = 1
    add = (1.0 - m01) * -10000.0
    return qb, kb, add, H


def kernel_ref(qb, kb, add, B, heads, Sq, Skv, H):
    q = qb[:, 64:64 + H].double().view(B, Sq, heads, 64).permute(0, 2, 1, 3)
    k = kb[:, H:2 * H].double().view(B, Skv, heads, 64).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) / 8.0 + add.double()[:, None, None, :]
    return torch.softmax(s, dim=-1)


def kernel_launch(qb, kb, add, B, heads, Sq, Skv, H, mean, offset=0):
    """-> (maps, guard region before, guard region after); the output sits ``GUARD + offset`` floats into a sentinel buffer."""
    n = B * Sq * Skv * (1 if mean else heads)
    buf = torch.full((2 * GUARD + offset + n,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD + offset:GUARD + offset + n]
    P = _K().attn_probs(qb.cuda()[:, 64:64 + H], kb.cuda()[:, H:2 * H], add.cuda(), B, heads, Sq, Skv, head_mean=mean, out=out)
    assert P.data_ptr() == out.data_ptr()
    shape = (B, Sq, Skv) if mean else (B, heads, Sq, Skv)
    return P.view(shape), buf[:GUARD + offset], buf[GUARD + offset + n:]


def build_model(precision="bf16"):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    import icka_amd
    from icka_amd import synth
    case, exp, names, factor = load_fixture()
    cfg = case["cfg"]
    c = BertConfig(cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                   num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                   max_position_embeddings=cfg["max_position_embeddings"], type_vocab_size=cfg["type_vocab_size"])
    m = MTCCMBertForMMTokenClassificationCRF(c, layer_num1=cfg["layer_num1"], num_labels=cfg["num_labels"], regions=cfg["regions"],
                                             variant="cl", max_seq_length=case["batch"]["input_ids"].shape[1])
    synth.fill_module_(m)
    scale_qk_(m, factor)
    icka_amd.set_precision(m, precision)
    batch = {k: v.cuda() for k, v in case["batch"].items()}
    return m.cuda(), batch, exp, names


def call_model(model, g, labels=False):
    return model(g["input_ids"], g["segment_ids"], g["input_mask"], g["added_attention_mask"], g["visual_embeds_mean"],
                 g["visual_embeds_att"], labels=g["labels"] if labels else None)
