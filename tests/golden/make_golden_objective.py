#!/usr/bin/env python3
"""Generate tests/golden/objective_*.npz: the reference's full training loss of the gated taggers with labels
(my_bert/gate_cl_modeling.py:1319-1395, my_bert/cl_modeling.py:1338-1382), run by the reference's OWN forward (dev container
only; the reference is imported in-process as make_golden.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objective.py

Stand-ins around the reference: the torchcrf package is replaced by a CRF whose forward is oracle.crf_oracle (crf_llh /
crf_reduce) over parameters with torchcrf's names and seeded values, so the CRF term is real and differentiable; Tensor.cuda
is the identity (the reference moves its relevance labels with .cuda(), :1345); the gate_cl forward prints the shape of the
cross encoder's output list (:1338-1340), so that list gets a ``shape``.  Every parameter is synth.seeded_tensor(name), the
model runs in eval mode.  Per case the fixture holds the inputs (as make_golden.py), the objective's arguments, the names,
shapes and samples of the reference's full state_dict (the values are regenerated from synth.seeded_tensor), the loss, its
parts (main, cl_loss, crs_loss from the reference's own total_loss / crs_loss on the same tensors) and the parameter
gradients (norms, samples, whole tensors up to 4096 elements).  tests/objective_oracle.py must equal the reference to 1e-6.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as MG  # noqa: E402
import objective_oracle as OO  # noqa: E402
from icka_amd import synth  # noqa: E402
from oracle import crf_oracle  # noqa: E402

TEMP, TEMP_LAMB, LAMB = 0.179, 0.7, 0.62      # My_cross_attention.py:479-497 defaults
TINY = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
            max_position_embeddings=128)


class CRF(nn.Module):
    """torchcrf.CRF's parameters and call convention, computed by oracle.crf_oracle."""

    def __init__(self, num_tags, batch_first=False):
        super().__init__()
        assert batch_first
        self.num_tags = num_tags
        self.start_transitions = nn.Parameter(torch.empty(num_tags))
        self.end_transitions = nn.Parameter(torch.empty(num_tags))
        self.transitions = nn.Parameter(torch.empty(num_tags, num_tags))
        self.last = None

    def forward(self, emissions, tags, mask=None, reduction="mean"):
        llh = crf_oracle.crf_llh(emissions, tags, mask, self.start_transitions, self.end_transitions, self.transitions)
        self.last = crf_oracle.crf_reduce(llh, mask, reduction)
        return self.last

    def decode(self, emissions, mask=None):
        return crf_oracle.crf_decode(emissions, mask, self.start_transitions, self.end_transitions, self.transitions)


class _Layers(list):
    @property
    def shape(self):
        return (len(self),)


def _capture(model, names):
    out = {}

    def hook(name):
        def f(_m, inp, o):
            out[name] = (inp, o)
        return f
    hs = [getattr(model, n).register_forward_hook(hook(n)) for n in names]
    return out, hs


def make_case(CL, GCL, name, variant, batch, seq_len, seed, negative_rate=None, temp=TEMP, temp_lamb=TEMP_LAMB, lamb=LAMB):
    mod = GCL if variant == "gate_cl" else CL
    ref_cfg, _ = MG._cfg_pair(mod, **dict(TINY))
    torch.manual_seed(0)
    model = mod.MTCCMBertForMMTokenClassificationCRF(ref_cfg, layer_num1=1, num_labels=13)
    synth.fill_module_(model)
    model.eval()
    model.txt2img_attention.register_forward_hook(lambda _m, _i, o: _Layers(o))
    heads = ["text_ouput_cl", "image_output_cl", "txt2img_attention"] + (["crs_classifier"] if variant == "gate_cl" else [])
    cap, hooks = _capture(model, heads)
    b = synth.synthetic_batch(batch, seq_len, 49, num_labels=13, vocab_size=ref_cfg.vocab_size, seed=seed, layout="BCHW")
    model.zero_grad()
    with contextlib.redirect_stdout(io.StringIO()):
        if variant == "gate_cl":
            loss = model(b["input_ids"], b["segment_ids"], b["input_mask"], b["added_attention_mask"], b["visual_embeds_mean"],
                         b["visual_embeds_att"], temp, temp_lamb, lamb, b["labels"], negative_rate)
        else:
            loss = model(b["input_ids"], b["segment_ids"], b["input_mask"], b["added_attention_mask"], b["visual_embeds_mean"],
                         b["visual_embeds_att"], None, temp, temp_lamb, b["labels"])
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    # ---- the parts, from the reference's own loss functions on the tensors of the run
    with torch.no_grad():
        t, v = cap["text_ouput_cl"][1], cap["image_output_cl"][1]
        main = -model.crf.last
        cl = model.total_loss(t, v, temp, temp_lamb)
        n = OO.negatives(batch, negative_rate) if variant == "gate_cl" else 0
        errs = {"cl": abs(OO.cl_loss(t, v, temp, temp_lamb).item() - cl.item())}
        if variant == "gate_cl":
            crs = cap["crs_classifier"][1]
            crs_l = model.crs_loss(crs, OO.crs_labels(batch, n))
            errs["crs"] = abs(OO.crs_loss(crs, n).item() - crs_l.item())
            total = lamb * main + (1 - lamb) * (crs_l + cl)
            cross = cap["txt2img_attention"][1][-1]
            seen = cap["crs_classifier"][0][0].view(batch, seq_len, -1)[:, :, TINY["hidden_size"]:]
            errs["swap"] = (OO.swap(cross, n) - seen).abs().max().item()
        else:
            crs_l = torch.zeros(())
            total = 0.88 * main + 0.12 * cl
        errs["total"] = abs(total.item() - loss.item())
    assert max(errs.values()) <= 1e-6, (name, errs)
    sd = model.state_dict()
    names = sorted(grads)
    out = {
        "meta_cfg": np.array([ref_cfg.vocab_size, ref_cfg.hidden_size, ref_cfg.num_hidden_layers, ref_cfg.num_attention_heads,
                              ref_cfg.intermediate_size, ref_cfg.max_position_embeddings, ref_cfg.type_vocab_size, 1, 13, 49],
                             dtype=np.int64),
        "meta_variant": np.array(variant),
        "meta_objective": np.array([temp, temp_lamb, lamb, -1 if negative_rate is None else negative_rate, n], dtype=np.float64),
        "input_ids": b["input_ids"].numpy(), "segment_ids": b["segment_ids"].numpy(), "input_mask": b["input_mask"].numpy(),
        "added_attention_mask": b["added_attention_mask"].numpy(), "labels": b["labels"].numpy(),
        "vis_seed": np.array([seed], dtype=np.int64), "vis_layout": np.array("BCHW"),
        "vis_sample": MG._sample(b["visual_embeds_att"]),
        "loss": np.array([loss.item()], dtype=np.float64),
        "parts": np.array([main.item(), cl.item(), crs_l.item()], dtype=np.float64),
        "t": t.detach().numpy(), "v": v.detach().numpy(),
        "sd_names": np.array(list(sd)),
        "sd_shapes": np.array([",".join(str(d) for d in sd[k].shape) for k in sd]),
        "sd_samples": np.stack([np.resize(MG._sample(sd[k].float(), 16), 16) for k in sd]),
        "grad_names": np.array(names),
        "grad_norms": np.array([grads[k].norm().item() for k in names], dtype=np.float64),
        "grad_samples": np.stack([np.resize(MG._sample(grads[k], 16), 16) for k in names]),
    }
    if variant == "gate_cl":
        out["crs"] = cap["crs_classifier"][1].detach().numpy()
    for k in names:
        if grads[k].numel() <= 4096:
            out["grad/" + k] = grads[k].numpy()
    path = os.path.join(HERE, name + ".npz")
    with open(path, "wb") as f:           # np.savez_compressed stamps the time into the zip: write it reproducibly
        _savez(f, out)
    print("%-32s %7.1f KB  loss %.6f  parts %s  oracle-vs-reference %s" % (
        name, os.path.getsize(path) / 1024.0, loss.item(), np.round(out["parts"], 6).tolist(),
        {k: "%.1e" % e for k, e in errs.items()}))


def _savez(f, arrays):
    """np.savez_compressed with fixed zip timestamps, so that re-running the script reproduces the files' sha256."""
    import zipfile
    with zipfile.ZipFile(f, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(8)
    _CM, CL, GCL = MG._import_reference()
    CL.CRF = GCL.CRF = CRF
    torch.Tensor.cuda = lambda self, *a, **k: self
    for nr in (None, 0, 4, 3, 8):
        make_case(CL, GCL, "objective_gatecl_b8_n%s" % ("none" if nr is None else nr), "gate_cl", 8, 128, 21, nr)
    make_case(CL, GCL, "objective_gatecl_b8_tl0", "gate_cl", 8, 128, 22, 4, temp_lamb=0.0)
    make_case(CL, GCL, "objective_gatecl_b8_tl1", "gate_cl", 8, 128, 23, 4, temp_lamb=1.0)
    make_case(CL, GCL, "objective_cl_b4_s32", "cl", 4, 32, 24)


if __name__ == "__main__":
    main()
