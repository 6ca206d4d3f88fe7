"""CPU: the attention-map fixture (made by the reference itself, tests/golden/make_golden_attention_maps.py) is a sound
yardstick -- rows are distributions, masked keys carry nothing, the maps are peaked enough that a constant output would fail --
and the float64 restatement built from the CPU oracle reproduces it; the C-ABI declares the probability entry."""
import os
import re

import numpy as np
import torch

from attention_maps_oracle import load_fixture, trunk_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_MIN = 0.3     # mean row maximum the fixture script asserts on the reference's maps


def test_fixture_rows_are_distributions():
    _case, exp, names, _f = load_fixture()
    assert names == ["bert.encoder.layer.0.attention.self", "bert.encoder.layer.1.attention.self",
                     "txt2img_attention.layer.0.attention.self"]
    for n in names:
        p = exp["all/" + n]
        assert p.dtype == np.float32 and p.shape == (3, 2, 32, 49 if n.startswith("txt2img") else 32)
        assert np.abs(p.astype(np.float64).sum(-1) - 1.0).max() < 1e-5, n
        assert p.min() >= 0.0


def test_fixture_masks_and_masked_keys():
    case, exp, names, _f = load_fixture()
    im = case["batch"]["input_mask"].numpy()
    assert im.sum(1).tolist() == [32, 16, 1]                       # full, half and single-token samples
    am = case["batch"]["added_attention_mask"].numpy()
    for n in names:
        p = exp["all/" + n]
        if n.startswith("txt2img"):
            assert am[1, 44:49].sum() == 0 and p[1, :, :, 44:].max() < 1e-30, n      # sample 1 lost its last five regions
        else:
            assert p[1, :, :, 16:].max() < 1e-30, n                # masked keys of the half-length sample
            assert p[2, :, :, 1:].max() < 1e-30 and np.abs(p[2, :, :, 0] - 1.0).max() < 1e-6, n


def test_fixture_head_means():
    _case, exp, names, _f = load_fixture()
    for n in names:
        assert np.abs(exp["mean/" + n] - exp["all/" + n].mean(axis=1)).max() < 1e-7, n
        assert exp["mean/" + n].shape == exp["all/" + n].shape[:1] + exp["all/" + n].shape[2:]


def test_fixture_is_peaked():
    """Against near-uniform maps (0.046 self / 0.031 cross with the unscaled seeded weights) a constant output would pass."""
    _case, exp, names, factor = load_fixture()
    assert factor > 1.0
    for n in names:
        peak = float(exp["all/" + n].max(-1).mean())
        assert peak >= PEAK_MIN, (n, peak)


def test_float64_oracle_reproduces_the_fixture():
    from icka_amd import synth
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    from oracle import mner_oracle as O
    from attention_maps_oracle import scale_qk_
    case, exp, names, factor = load_fixture()
    cfg = case["cfg"]
    c = BertConfig(cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                   num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                   max_position_embeddings=cfg["max_position_embeddings"], type_vocab_size=cfg["type_vocab_size"])
    m = MTCCMBertForMMTokenClassificationCRF(c, layer_num1=cfg["layer_num1"], num_labels=cfg["num_labels"], regions=cfg["regions"],
                                             variant="cl", max_seq_length=32)
    synth.fill_module_(m)
    scale_qk_(m, factor)
    P = {k: v.detach().to(torch.float64) for k, v in m.state_dict().items() if torch.is_floating_point(v)}
    ocfg = O.OracleConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"],
                          num_attention_heads=cfg["num_attention_heads"], intermediate_size=cfg["intermediate_size"],
                          max_position_embeddings=cfg["max_position_embeddings"], type_vocab_size=cfg["type_vocab_size"])
    with torch.no_grad():
        maps = trunk_maps(P, ocfg, case["batch"], cfg["layer_num1"], cfg["regions"])
    assert list(maps) == names
    for n in names:
        err = np.abs(maps[n].numpy() - exp["all/" + n]).max()
        assert err < 1e-5, (n, err)


def test_header_declares_the_probability_entry():
    text = open(os.path.join(ROOT, "include", "icka_hip.h")).read()
    assert re.search(r"\bint\s+icka_attn_probs\s*\(", text)
    assert re.search(r"#define\s+ICKA_ATTN_PROBS_HEAD_MEAN\s+1\b", text)
    from icka_amd import _lib
    assert "icka_attn_probs" in _lib.PROTOTYPES and _lib.ABI_VERSION == 6
