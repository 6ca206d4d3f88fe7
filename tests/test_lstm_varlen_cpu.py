"""CPU: the variable-length LSTM contract (include/icka_hip.h: icka_lstm_fwd_varlen) restated in float64
(tests/lstm_varlen_oracle.py: the recurrence over all S positions with the i / f pre-activations of the pads at -1e4, and the
kernels' analytic backward) equals torch.nn.LSTM on a pack_padded_sequence input -- values and every gradient to 1e-12, exact
zeros at the pads -- so the mask is all the kernels need; plus what the feature must not disturb: the dispatch restatement
of tests/lstm_check.py still finds its 26 instantiations in csrc/lstm.hip, and the ABI lists the new entries."""
import pytest
import torch

import lstm_check as lc
import lstm_varlen_oracle as vo

TOL = 1e-12


def _lstm(I, H, seed):
    torch.manual_seed(seed)
    return torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()


# lengths 1 and S, unsorted; one sample per length; all full; all 1
CASES = [(5, 7, 8, 8, [3, 7, 1, 5, 7]), (4, 6, 16, 8, [6, 1, 4, 2]), (3, 5, 8, 16, [5, 5, 5]), (2, 4, 8, 8, [1, 1]),
         (6, 9, 8, 8, [2, 9, 4, 1, 8, 3])]


@pytest.mark.parametrize("B,S,I,H,lens", CASES)
def test_masked_recurrence_is_nn_lstm_on_a_packed_input(B, S, I, H, lens):
    lstm = _lstm(I, H, B * 10 + S)
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, S, I, generator=g, dtype=torch.float64)
    dy = torch.randn(B, S, 2 * H, generator=g, dtype=torch.float64)          # non-zero at the pads too
    xr = x.clone().requires_grad_(True)
    ro, (rh, rc) = vo.packed_lstm(lstm, xr, lens)
    (ro * dy).sum().backward()
    r = vo.masked_bilstm(x, lens, *vo.lstm_params(lstm), dy=dy)
    worst = {"out": (r["out"] - ro.detach()).abs().max().item(), "h_n": (r["h_n"] - rh.detach()).abs().max().item(),
             "c_n": (r["c_n"] - rc.detach()).abs().max().item(), "dx": (r["dx"] - xr.grad).abs().max().item()}
    for d, sfx in enumerate(("", "_reverse")):
        worst["dw_ih" + sfx] = (r["dw_ih"][d] - getattr(lstm, "weight_ih_l0" + sfx).grad).abs().max().item()
        worst["dw_hh" + sfx] = (r["dw_hh"][d] - getattr(lstm, "weight_hh_l0" + sfx).grad).abs().max().item()
        worst["db_ih" + sfx] = (r["db"][d] - getattr(lstm, "bias_ih_l0" + sfx).grad).abs().max().item()
        worst["db_hh" + sfx] = (r["db"][d] - getattr(lstm, "bias_hh_l0" + sfx).grad).abs().max().item()
    print("\n[masked recurrence vs packed nn.LSTM B%d S%d I%d H%d] worst abs differences: %s" % (
        B, S, I, H, ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))
    for k, v in worst.items():
        assert v < TOL, (k, v)
    pad = vo.pad_mask(lens, S)
    for k in ("out", "dx", "dgates", "c_all"):
        assert bool((r[k][pad] == 0).all()), "%s is not exactly zero at the pads" % k
    assert bool((r["act"][pad][:, :, :2] == 0).all()) and bool(torch.isfinite(r["act"]).all())


def test_samples_of_length_zero_change_nothing_and_read_zero():
    """ATen refuses an empty sequence, so a batch with len = 0 samples is checked against the batch without them."""
    B, S, I, H = 5, 6, 8, 8
    lens = [0, 4, 0, 6, 1]
    keep = [1, 3, 4]
    lstm = _lstm(I, H, 3)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, S, I, generator=g, dtype=torch.float64)
    dy = torch.randn(B, S, 2 * H, generator=g, dtype=torch.float64)
    P = vo.lstm_params(lstm)
    full = vo.masked_bilstm(x, lens, *P, dy=dy)
    part = vo.masked_bilstm(x[keep], [lens[b] for b in keep], *P, dy=dy[keep])
    # (a BLAS product over another number of rows may round differently: 1e-12, not bitwise)
    for k in ("out", "dx", "dgates", "c_all", "act"):
        assert (full[k][keep] - part[k]).abs().max().item() < TOL, k
    for k in ("h_n", "c_n"):
        assert (full[k][:, keep] - part[k]).abs().max().item() < TOL, k
        assert bool((full[k][:, [0, 2]] == 0).all())
    for k in ("out", "dx", "dgates"):
        assert bool((full[k][[0, 2]] == 0).all())
    for k in ("dw_ih", "dw_hh", "db"):
        for d in (0, 1):
            assert (full[k][d] - part[k][d]).abs().max().item() < TOL       # (a sum over more, exactly zero, rows)
    # ... and the kept samples are nn.LSTM's
    ro, (rh, rc) = vo.packed_lstm(lstm, x[keep], [lens[b] for b in keep])
    assert (part["out"] - ro).abs().max().item() < TOL and (part["h_n"] - rh).abs().max().item() < TOL


def test_lengths_outside_the_sequence_clamp():
    B, S, I, H = 3, 4, 8, 8
    lstm = _lstm(I, H, 1)
    x = torch.randn(B, S, I, dtype=torch.float64)
    P = vo.lstm_params(lstm)
    a = vo.masked_bilstm(x, [S + 5, 2, -3], *P)
    b = vo.masked_bilstm(x, [S, 2, 0], *P)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["h_n"], b["h_n"])
    full, _ = lstm(x)
    assert (a["out"][0] - full[0].detach()).abs().max().item() < TOL


def test_mask_gates_helper_marks_the_pads_of_both_directions():
    B, S, H = 3, 4, 8
    gx = torch.randn(B * S, 8 * H)
    m = vo.mask_gates(gx, [4, 1, 0], B, S, H).reshape(B, S, 2, 4, H)
    pad = vo.pad_mask([4, 1, 0], S)
    assert bool((m[:, :, :, :2][pad] == vo.PAD_GATE).all())
    same = m == gx.reshape(B, S, 2, 4, H)
    assert bool(same[:, :, :, 2:].all()) and bool(same[~pad].all())


def test_lengths_of_mask_is_the_rule_of_the_packing_plan():
    from icka_amd import packing
    from icka_amd.lstm import lengths_of_mask
    mask = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 1, 1, 0], [1, 0, 0, 0, 0]])
    assert lengths_of_mask(mask).tolist() == packing.plan_reference(mask, 64)["lens"].tolist() == [3, 5, 0, 1, 1]


def test_lengths_argument_is_checked():
    from icka_amd.lstm import _check_lengths
    dev = torch.device("cpu")
    assert _check_lengths(torch.tensor([1, 2, 3]), 3, dev).dtype == torch.int32
    with pytest.raises(TypeError):
        _check_lengths(torch.tensor([1.0, 2.0, 3.0]), 3, dev)
    with pytest.raises(TypeError):
        _check_lengths([1, 2, 3], 3, dev)
    with pytest.raises(ValueError):
        _check_lengths(torch.tensor([1, 2]), 3, dev)
    with pytest.raises(ValueError):
        _check_lengths(torch.tensor([[1, 2, 3]]), 3, dev)
    with pytest.raises(ValueError):
        _check_lengths(torch.tensor([1, 2, 3]), 3, torch.device("meta"))


def test_set_length_aware_switches_every_bilstm_and_refuses_a_model_without_one():
    import icka_amd
    from icka_amd.lstm import BiLSTM

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = BiLSTM(32, 32), torch.nn.Sequential(BiLSTM(32, 32))
    m = Two()
    assert not m.a.length_aware and not m.b[0].length_aware           # off by default
    assert icka_amd.set_length_aware(m) is m and m.a.length_aware and m.b[0].length_aware
    icka_amd.set_length_aware(m, False)
    assert not m.a.length_aware and not m.b[0].length_aware
    with pytest.raises(ValueError):
        icka_amd.set_length_aware(torch.nn.Linear(2, 2))


def test_dispatch_restatement_still_covers_the_source():
    """Variable length is a runtime property of the same 26 instantiations, all launched below the first icka_lstm_fwd* entry."""
    lc.assert_dispatch_coverage()


def test_abi_lists_the_variable_length_entries():
    from icka_amd import _lib
    for name, nargs in (("icka_lstm_fwd_varlen", 13), ("icka_lstm_bwd_varlen", 13), ("icka_lstm_mask_gates", 7)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert len(_lib.PROTOTYPES["icka_lstm_fwd"][1]) == 12 and len(_lib.PROTOTYPES["icka_lstm_bwd"][1]) == 12
    assert not [n for n in _lib.PROTOTYPES if "varlen" in n and "_set_" in n]
