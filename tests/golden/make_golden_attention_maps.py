#!/usr/bin/env python3
"""Generate tests/golden/attention_maps_tiny.npz by running the REFERENCE itself (dev container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attention_maps.py

The reference's ``cl`` model (2 encoder layers, H 128, 2 heads, layer_num1 = 1; B 3, S 32, 49 regions) runs in ``eval()`` and a
forward hook on the ``dropout`` child of every attention module captures its input: ``attention_probs`` as the reference computes
them (Cross_Modal_Interaction_Module.py:492-497, :606-611), before dropout.

Masks: sample 0 full length, sample 1 half length, sample 2 with a single valid text token; sample 1 also loses its last five
regions.

The seeded N(0, 0.02) weights give maps within 0.005 of uniform (mean row maximum 0.046 self / 0.031 cross), against which a
constant output would pass any sensible bar.  So the ``query`` and ``key`` WEIGHTS (not the biases) of every attention module
are multiplied by QK_SCALE after seeding, and the script asserts on the reference's own maps that the mean row maximum is
>= 0.3 for every hooked module.  The fixture stores the factor, the per-head maps and their head means; only data is written.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from icka_amd import synth  # noqa: E402

QK_SCALE = 8.0
PEAK_MIN = 0.3
CFG = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
           max_position_embeddings=64)
B, S, R, LAYER_NUM1, NUM_LABELS, SEED = 3, 32, 49, 1, 13, 21


def scale_qk_(model, factor: float) -> None:
    """Multiply the query / key weights of every attention module (a module with ``query`` and ``key`` children) by ``factor``."""
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "query") and hasattr(m, "key"):
                m.query.weight.mul_(factor)
                m.key.weight.mul_(factor)


def masks_(batch, regions: int) -> None:
    im = batch["input_mask"]
    im[0] = 1
    im[1] = 0
    im[1, :im.shape[1] // 2] = 1
    im[2] = 0
    im[2, 0] = 1
    am = batch["added_attention_mask"]
    am[:, :regions] = 1
    am[1, regions - 5:regions] = 0
    am[:, regions:] = im
    g = torch.Generator().manual_seed(7)
    batch["input_ids"] = torch.randint(1, CFG["vocab_size"], im.shape, generator=g) * im


def main():
    torch.set_num_threads(8)
    _CM, CL, _GCL = MG._import_reference()
    ref_cfg, _ocfg = MG._cfg_pair(CL, **dict(CFG))
    torch.manual_seed(0)
    model = CL.MTCCMBertForMMTokenClassificationCRF(ref_cfg, layer_num1=LAYER_NUM1, num_labels=NUM_LABELS)
    synth.fill_module_(model)
    scale_qk_(model, QK_SCALE)
    model.eval()
    batch = synth.synthetic_batch(B, S, R, num_labels=NUM_LABELS, vocab_size=CFG["vocab_size"], seed=SEED, layout="BCHW")
    masks_(batch, R)

    got = {}
    hooks = []
    for name, m in model.named_modules():
        if hasattr(m, "query") and hasattr(m, "key") and hasattr(m, "dropout"):
            hooks.append(m.dropout.register_forward_hook(
                lambda _mod, inp, _out, name=name: got.setdefault(name, []).append(inp[0].detach().clone())))
    with torch.no_grad():
        model(batch["input_ids"], batch["segment_ids"], batch["input_mask"], batch["added_attention_mask"],
              batch["visual_embeds_mean"], batch["visual_embeds_att"], None)
    for h in hooks:
        h.remove()
    names = list(got)
    out = {
        "meta_cfg": np.array([ref_cfg.vocab_size, ref_cfg.hidden_size, ref_cfg.num_hidden_layers, ref_cfg.num_attention_heads,
                              ref_cfg.intermediate_size, ref_cfg.max_position_embeddings, ref_cfg.type_vocab_size, LAYER_NUM1,
                              NUM_LABELS, R], dtype=np.int64),
        "meta_variant": np.array("cl"),
        "qk_scale": np.array([QK_SCALE], dtype=np.float64),
        "names": np.array(names),
        "input_ids": batch["input_ids"].numpy(), "segment_ids": batch["segment_ids"].numpy(),
        "input_mask": batch["input_mask"].numpy(), "added_attention_mask": batch["added_attention_mask"].numpy(),
        "labels": batch["labels"].numpy(),
        "vis_seed": np.array([SEED], dtype=np.int64), "vis_layout": np.array("BCHW"),
        "vis_sample": MG._sample(batch["visual_embeds_att"]),
    }
    for n in names:
        assert len(got[n]) == 1, (n, len(got[n]))
        p = got[n][0]
        assert p.dim() == 4 and p.dtype == torch.float32
        peak = p.max(dim=-1).values.mean().item()
        assert peak >= PEAK_MIN, "%s: mean row maximum %.3f < %.1f: raise QK_SCALE" % (n, peak, PEAK_MIN)
        out["all/" + n] = p.numpy()
        out["mean/" + n] = p.mean(dim=1).numpy()
        print("%-48s %s mean row max %.3f" % (n, tuple(p.shape), peak))
    path = os.path.join(HERE, "attention_maps_tiny.npz")
    np.savez_compressed(path, **out)
    print("attention_maps_tiny %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
