"""GPU: the variable-length LSTM (include/icka_hip.h: icka_lstm_fwd_varlen / icka_lstm_bwd_varlen / icka_lstm_mask_gates).

Kernel level: every form of the recurrence once (tagged words with one and two batch tiles, ICKA_LSTM_NO_BATCH_SPLIT, the
rs backward <4> / <8> / <12>, both ticket kernels, the per-step kernels at B = 33), S = 6, outputs pre-filled with NaN.  The
call on (gates_x, lens) must equal -- torch.equal, at every position -- the FIXED-length entry (same instantiation, all S steps)
on a copy of gates_x whose pad i / f columns were set to -1e4 with torch: the select at the load is that mask and nothing
else (and a later form that skips steps must still store every position).  The step-wise float64 bounds of tests/lstm_check.py
hold on it.

Module level: BiLSTM(x, lengths=) against CPU nn.LSTM on a pack_padded_sequence input (bf16 and fp32 mode, the tolerances of
the same comparisons without lengths in tests/test_lstm_gpu.py / tests/test_exact_gpu.py: masking adds only exact zeros),
argument errors, one captured step replayed on two length sets, and the `_gate_1` tagger under set_length_aware."""
import functools

import pytest
import torch

import kernel_check as kc
import lstm_check as lc
import lstm_varlen_oracle as vo
from kernel_check import BF16, F32

pytestmark = pytest.mark.gpu

S_K = 6
TAGGER_GRAD_BAR = 1.6e-2   # the bar of tests/test_lstm_gpu.py::test_gate_1_tagger_end_to_end_against_oracle_composition
# (B, H, flags): shapes of lstm_check.CASES, one per form
KERNEL_CASES = [
    (16, 512, 0),                      # LL<1, 4> / rs<8>, grid.z = 1
    (20, 768, 0),                      # LL<1, 6> / rs<12>, grid.z = 2: the two tiles have different longest rows
    (32, 256, lc.NO_BATCH_SPLIT),      # LL<2, 2>: one block holds both tiles; rs<4> with grid.z = 2
    (20, 384, 0),                      # ticket forward and backward <2, 24>
    (5, 768, lc.TICKETS),              # ticket forward and backward <1, 24> by the flag
    (33, 288, 0),                      # per-step <4, 8>: all S steps with the mask
]
PATTERNS = ["mixed", "zero_tile", "short"]


def _case_id(c):
    return lc.case_id((c[0], S_K, c[1], c[2]))


def _lens(B, S, pattern):
    """mixed: 0, 1 and S in the first 16-row tile (maximum S), the later tiles stop at S - 2 (with 0 and 1 among them);
    zero_tile: the first tile all zero, the later ones mixed up to S - 1 (B <= 16: the whole batch is empty, L = 0);
    short: nothing longer than S - 3: the last positions are pads of every row."""
    cyc = {"mixed": [S, 0, 1, 3, S - 1, 2], "zero_tile": [0], "short": [1, S - 3, 0, 2]}[pattern]
    late = {"mixed": [S - 2, 0, 1, 2], "zero_tile": [S - 1, 1, 0, 3], "short": [S - 3, 0, 1]}[pattern]
    return [cyc[b % len(cyc)] if b < 16 else late[b % len(late)] for b in range(B)]


def _inputs(B, S, H):
    g = torch.Generator().manual_seed(B * 1000 + S * 10 + H + 7)
    whh = (torch.randn(8 * H, H, generator=g) * H ** -0.5).to(BF16)          # [2][4H][H]
    gx = torch.randn(B * S, 8 * H, generator=g) * 0.7
    dy = (torch.randn(B * S, 2 * H, generator=g) * 0.3).to(BF16)            # non-zero at the pads
    return whh, gx, dy


def _gin(values):
    return kc.Guarded(values.shape[0], values.shape[1], values.dtype, fill=kc.NAN_FILL[values.dtype], init=values.cuda())


def _skip_unless_reachable(phase, B, H, fl):
    from icka_amd import kernels as K
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count - K._LSTM_RESERVED[0]
    want, got = lc.dispatch(phase, B, H, fl), lc.dispatch(phase, B, H, fl, cus=cus)
    if got != want:
        pytest.skip("%d CUs: %s<%s> is unreachable" % (cus, want[1], want[2]))
    return want


def _err_word(what):
    from icka_amd import _lib
    torch.cuda.synchronize()
    rc = _lib.load().icka_lstm_barrier_error()
    assert rc == 0, "icka_lstm_barrier_error() = %d after %s" % (rc, what)


def _fwd(B, S, H, fl, gx, whh, lens):
    """One forward into NaN-filled guarded outputs (Guarded fills an output's logical part with NaN)."""
    from icka_amd import kernels as K
    M = B * S
    o = {"y": kc.Guarded(M, 2 * H, BF16), "c_all": kc.Guarded(M, 2 * H, F32), "act": kc.Guarded(M, 8 * H, BF16),
         "hprev": kc.Guarded(M, 2 * H, BF16)}
    K.lstm_fwd(gx.view, whh.view, o["y"].view, o["c_all"].view, o["act"].view, o["hprev"].view, B, S, H, flags=fl, lens=lens)
    torch.cuda.synchronize()
    for n, g in list(o.items()) + [("gates_x", gx), ("w_hh", whh)]:
        g.check(what="forward " + n)
    return o


def _bwd(B, S, H, fl, dy, whh_t, fw, lens):
    from icka_amd import kernels as K
    dg, carry = kc.Guarded(B * S, 8 * H, BF16), kc.Guarded(2 * B, H, F32)
    K.lstm_bwd(dy.view, whh_t.view, fw["act"].view, fw["c_all"].view, dg.view, carry.view, B, S, H, flags=fl, lens=lens)
    torch.cuda.synchronize()
    for n, g in (("dgates", dg), ("dc_carry", carry), ("dy", dy), ("act", fw["act"]), ("c_all", fw["c_all"])):
        g.check(what="backward " + n)
    return dg, carry


@functools.lru_cache(maxsize=None)
def _run(case, pattern):
    """The variable-length call and the fixed-length call on the masked copy, forward and backward; computed once per
    (case, pattern), shared by the tests below and left unchanged."""
    B, H, fl = case
    S = S_K
    whh, gx, dy = _inputs(B, S, H)
    lens = _lens(B, S, pattern)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    whh_g = _gin(whh)
    whh_t = _gin(whh.reshape(2, 4 * H, H).transpose(1, 2).reshape(2 * H, 4 * H).contiguous())
    gxm = vo.mask_gates(gx, lens, B, S, H)
    var = _fwd(B, S, H, fl, _gin(gx), whh_g, lens_d)
    fix = _fwd(B, S, H, fl, _gin(gxm), whh_g, None)
    dy_g = _gin(dy)
    var_dg, var_carry = _bwd(B, S, H, fl, dy_g, whh_t, var, lens_d)
    fix_dg, _ = _bwd(B, S, H, fl, dy_g, whh_t, fix, None)
    _err_word("the launches of %s %s" % (_case_id(case), pattern))
    return {"lens": lens, "whh": whh_g, "gxm": gxm.cuda(), "dy": dy.cuda(), "var": var, "fix": fix, "var_dg": var_dg,
            "fix_dg": fix_dg, "var_carry": var_carry}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_case_id)
def test_varlen_forward_equals_the_untrimmed_call_on_masked_gates(case, pattern):
    B, H, fl = case
    S = S_K
    form = _skip_unless_reachable("fwd", B, H, fl)[0]
    r = _run(case, pattern)
    var, fix = r["var"], r["fix"]
    for n in ("y", "c_all", "hprev"):
        assert torch.equal(var[n].view, fix[n].view), "%s %s: %d elements differ from the untrimmed call (NaN left: %d)" % (
            form, n, int((var[n].view != fix[n].view).sum()), int(torch.isnan(var[n].view.float()).sum()))
    pad = vo.pad_mask(r["lens"], S).cuda()
    act_v, act_f = var["act"].view.reshape(B, S, 2, 4, H), fix["act"].view.reshape(B, S, 2, 4, H)
    assert torch.equal(act_v[~pad], act_f[~pad]), "%s act differs at live positions" % form
    assert bool(torch.isfinite(act_v.float()).all()), "%s act is not finite everywhere" % form
    assert bool((act_v[pad][:, :, :2] == 0).all()), "%s act: i / f are not exactly zero at the pads" % form
    # the contract the weight-gradient GEMMs rely on: exact zeros at every pad (hprev: y of the step before, so zero too except
    # the forward direction's t = len, which holds the last live h)
    for n in ("y", "c_all"):
        assert bool((var[n].view.reshape(B, S, 2 * H)[pad] == 0).all()), "%s %s is not exactly zero at the pads" % (form, n)
    hp = var["hprev"].view.reshape(B, S, 2, H)
    assert bool((hp[:, :, 1][pad] == 0).all()) and bool(torch.isfinite(hp.float()).all())
    lc.check_fwd("varlen fwd " + form, r["gxm"], r["whh"].view, var["y"].view, var["c_all"].view, var["act"].view,
                 var["hprev"].view, B, S, H)
    kc.report("lstm_fwd_varlen %s %s" % (_case_id(case), pattern))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_case_id)
def test_varlen_backward_equals_the_untrimmed_call(case, pattern):
    B, H, fl = case
    S = S_K
    form = _skip_unless_reachable("bwd", B, H, fl)[0]
    r = _run(case, pattern)
    dv, df = r["var_dg"].view, r["fix_dg"].view
    assert torch.equal(dv, df), "%s dgates: %d elements differ from the untrimmed call (NaN left: %d)" % (
        form, int((dv != df).sum()), int(torch.isnan(dv.float()).sum()))
    pad = vo.pad_mask(r["lens"], S).cuda()
    assert bool((dv.reshape(B, S, 8 * H)[pad] == 0).all()), "%s dgates is not exactly zero at the pads" % form
    var = r["var"]
    lc.check_bwd("varlen bwd " + form, r["dy"], r["whh"].view, var["act"].view, var["c_all"].view, dv,
                 r["var_carry"].view if form == "step" else None, B, S, H, rs=form == "rs")
    kc.report("lstm_bwd_varlen %s %s" % (_case_id(case), pattern))


def test_mask_gates_kernel_is_the_torch_mask():
    from icka_amd import kernels as K
    B, S, H = 5, 7, 64
    lens = [7, 0, 3, 12, -2]
    gx = torch.randn(B * S, 8 * H)
    g = _gin(gx)
    K.lstm_mask_gates(g.view, torch.tensor(lens, dtype=torch.int32, device="cuda"), B, S, H)
    torch.cuda.synchronize()
    g.check(what="masked gates_x")
    assert torch.equal(g.view.cpu(), vo.mask_gates(gx, lens, B, S, H))


# ------------------------------------------------------------------------------------------------------- module level
def _module_lens(B, S):
    """Unsorted, every length >= 1 (ATen's packing refuses 0), lengths 1 and S among them."""
    base = [S, 1, max(1, S - 2), 2, S - 1, 3]
    return [base[b % len(base)] for b in range(B)]


def _packed_reference(ref, x, lens, w):
    xr = x.clone().requires_grad_(True)
    ro, (rh, rc) = vo.packed_lstm(ref, xr, lens)
    (ro * w).sum().backward()
    return xr, ro.detach(), rh.detach(), rc.detach()


@pytest.mark.parametrize("form", ["handoff", "tickets", "per_step"])
@pytest.mark.parametrize("B,S,H", [(3, 7, 256), (20, 6, 512), (33, 5, 64)])
def test_bilstm_with_lengths_against_packed_aten(B, S, H, form):
    from icka_amd import _lib
    from icka_amd.lstm import BiLSTM
    torch.manual_seed(B * 100 + S)
    ref = torch.nn.LSTM(H, H, batch_first=True, bidirectional=True)
    mine = BiLSTM(H, H)
    mine.recurrence_flags = {"handoff": 0, "tickets": _lib.LSTM_TICKETS, "per_step": _lib.LSTM_PER_STEP}[form]
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    lens = _module_lens(B, S)
    lens_d = torch.tensor(lens, device="cuda")                          # int64: the layer casts on the device
    x = torch.randn(B, S, H) * 0.5
    w = torch.randn(B, S, 2 * H, generator=torch.Generator().manual_seed(1))      # non-zero at the pads
    xg = x.cuda().requires_grad_(True)
    out, (h_n, c_n) = mine(xg, lengths=lens_d)
    (out.float() * w.cuda()).sum().backward()
    xr, ro, rh, rc = _packed_reference(ref, x.to(BF16).float(), lens, w)     # the kernels see the bf16-rounded input
    assert out.shape == ro.shape and out.dtype == BF16
    err = (out.float().cpu() - ro).abs().max().item()
    eh, ec = (h_n.cpu() - rh).abs().max().item(), (c_n.cpu() - rc).abs().max().item()
    rel = lambda a, b: ((a.float().cpu() - b).norm() / (b.norm() + 1e-12)).item()
    grads = {"dx": rel(xg.grad, xr.grad)}
    for n, p in mine.named_parameters():
        grads[n] = rel(p.grad, dict(ref.named_parameters())[n].grad)
    print("\n[BiLSTM lengths B%d S%d H%d %s] out %.3e h_n %.3e c_n %.3e, worst gradient rel %.3e" % (
        B, S, H, form, err, eh, ec, max(grads.values())))
    assert err < 2e-2 and eh < 2e-2 and ec < 3e-2, (err, eh, ec)
    for n, v in grads.items():
        assert v < 3e-2, (n, v)
    pad = vo.pad_mask(lens, S).cuda()
    assert bool((out[pad] == 0).all()) and bool((xg.grad[pad] == 0).all())
    # lengths past the sequence clamp: S + 5 is S, and S everywhere is the layer without lengths
    with torch.no_grad():
        a, (ah, ac) = mine(xg, lengths=torch.full((B,), S + 5, device="cuda"))
        b, (bh, bc) = mine(xg, lengths=torch.full((B,), S, device="cuda", dtype=torch.int32))
        c, (ch, cc) = mine(xg)
    assert torch.equal(a, b) and torch.equal(ah, bh) and torch.equal(ac, bc)
    assert torch.equal(b, c) and torch.equal(bh, ch) and torch.equal(bc, cc)
    _err_word("BiLSTM with lengths")


@pytest.mark.parametrize("B,S,H", [(3, 7, 256), (20, 6, 512), (33, 5, 64)])
def test_fp32_bilstm_with_lengths_against_packed_aten(B, S, H):
    """fp32 mode: the mask as a pass over the f32 gate buffer (icka_lstm_mask_gates); the tolerances of
    tests/test_exact_gpu.py::test_fp32_bilstm_against_aten."""
    import icka_amd
    from icka_amd.lstm import BiLSTM
    torch.manual_seed(B * 100 + S)
    ref = torch.nn.LSTM(H, H, batch_first=True, bidirectional=True)
    mine = BiLSTM(H, H)
    mine.load_state_dict(ref.state_dict())
    mine = icka_amd.set_precision(mine.cuda(), "fp32")
    lens = _module_lens(B, S)
    x = torch.randn(B, S, H) * 0.5
    w = torch.randn(B, S, 2 * H, generator=torch.Generator().manual_seed(1))
    xg = x.cuda().requires_grad_(True)
    out, (h_n, c_n) = mine(xg, lengths=torch.tensor(lens, device="cuda", dtype=torch.int32))
    (out * w.cuda()).sum().backward()
    xr, ro, rh, rc = _packed_reference(ref, x, lens, w)
    assert out.dtype == F32
    err = (out.cpu() - ro).abs().max().item()
    rel = lambda a, b: ((a.double().cpu() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    worst = rel(xg.grad, xr.grad)
    for n, p in mine.named_parameters():
        worst = max(worst, rel(p.grad, dict(ref.named_parameters())[n].grad))
    print("\n[fp32 BiLSTM lengths B%d S%d H%d] max abs out err %.3e, worst gradient rel-L2 %.3e" % (B, S, H, err, worst))
    assert err < 1e-5, err
    assert (h_n.cpu() - rh).abs().max().item() < 1e-5 and (c_n.cpu() - rc).abs().max().item() < 1e-5
    assert worst < 1e-4, worst
    pad = vo.pad_mask(lens, S).cuda()
    assert bool((out[pad] == 0).all()) and bool((xg.grad[pad] == 0).all())


def test_samples_of_length_zero_read_zero_and_leave_the_others_alone():
    from icka_amd.lstm import BiLSTM
    B, S, H = 6, 5, 256
    torch.manual_seed(3)
    m = BiLSTM(H, H).cuda()
    x = (torch.randn(B, S, H) * 0.5).cuda()
    lens = torch.tensor([0, 4, 0, 5, 1, 0], device="cuda")
    keep = [1, 3, 4]
    with torch.no_grad():
        out, (h_n, c_n) = m(x, lengths=lens)
        part, (ph, pc) = m(x[keep].contiguous(), lengths=lens[keep])
    assert bool((out[[0, 2, 5]] == 0).all()) and bool((h_n[:, [0, 2, 5]] == 0).all()) and bool((c_n[:, [0, 2, 5]] == 0).all())
    # ... and the batch without them computes the same for the others (the bf16 tolerances of the comparison with ATen: the
    # input projection of another number of rows may take another GEMM tiling)
    assert (out[keep].float() - part.float()).abs().max().item() < 2e-2
    assert (h_n[:, keep] - ph).abs().max().item() < 2e-2 and (c_n[:, keep] - pc).abs().max().item() < 3e-2
    _err_word("a batch with empty samples")


def test_bilstm_lengths_argument_errors():
    from icka_amd.lstm import BiLSTM
    m = BiLSTM(64, 64).cuda()
    x = torch.zeros(2, 3, 64, device="cuda")
    with pytest.raises(TypeError):
        m(x, lengths=torch.tensor([1.0, 2.0], device="cuda"))
    with pytest.raises(TypeError):
        m(x, lengths=[1, 2])
    with pytest.raises(ValueError):
        m(x, lengths=torch.tensor([1, 2, 3], device="cuda"))
    with pytest.raises(ValueError):
        m(x, lengths=torch.tensor([[1, 2]], device="cuda"))
    with pytest.raises(ValueError):
        m(x, lengths=torch.tensor([1, 2]))                  # on the host
    with pytest.raises(NotImplementedError):
        m(x, hx=(x, x), lengths=torch.tensor([1, 2], device="cuda"))


def test_one_captured_step_serves_length_sets_with_different_maxima():
    """The lengths are device data: ONE capture of forward + backward, replayed on two length sets whose maxima differ, equals
    the eager call on the same data each time."""
    from icka_amd.graph import GraphedStep
    from icka_amd.lstm import BiLSTM
    B, S, H = 20, 8, 256
    torch.manual_seed(11)
    m = BiLSTM(H, H).cuda()
    x = (torch.randn(B, S, H) * 0.5).cuda()
    w = (torch.randn(B, S, 2 * H) * 0.3).cuda()
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    held = {}

    def step():
        out, (h_n, c_n) = m(x, lengths=lens)
        held["out"], held["h_n"] = out, h_n
        loss = (out.float() * w).sum()
        loss.backward()
        return loss
    sets = [[(5 * b) % (S + 1) for b in range(B)],                      # both tiles reach S
            [(b % 3) if b < 16 else 1 + (b % 4) for b in range(B)]]      # maxima 2 and 4
    gs = GraphedStep(m, step, warmup=1)
    static = dict(held)          # the tensors of the capture: every replay writes these (an eager step() rebinds ``held``)
    try:
        for k, ls in enumerate(sets):
            lens.copy_(torch.tensor(ls, dtype=torch.int32))
            x.copy_((torch.randn(B, S, H, generator=torch.Generator().manual_seed(k)) * 0.5))
            m.zero_grad()
            loss = gs().clone()
            torch.cuda.synchronize()
            got = {"out": static["out"].clone(), "h_n": static["h_n"].clone(), "loss": loss}
            got.update({n: p.grad.clone() for n, p in m.named_parameters()})
            m.zero_grad()
            loss = step().clone()
            torch.cuda.synchronize()
            want = {"out": held["out"], "h_n": held["h_n"], "loss": loss}
            want.update({n: p.grad for n, p in m.named_parameters()})
            for n in want:
                assert torch.equal(got[n], want[n]), "replay %d: %s differs from the eager call" % (k, n)
            pad = vo.pad_mask(ls, S).cuda()
            assert bool((got["out"][pad] == 0).all()) and bool(torch.isfinite(got["weight_hh_l0"]).all())
        assert gs.stats["captures"] == 1 and gs.stats["replays"] == 2, gs.stats
    finally:
        gs.close()
    _err_word("the replays")


def test_gate_1_tagger_under_set_length_aware_against_the_packed_oracle_composition():
    """tests/test_lstm_gpu.py::test_gate_1_tagger_end_to_end_against_oracle_composition with the switch on: the CPU
    composition feeds its nn.LSTM packed (lengths = first zero of the mask); that test's configuration and bars."""
    import torch.nn.functional as F
    import icka_amd
    from icka_amd import synth
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
    from oracle import crf_oracle as OC
    from oracle import mner_oracle as O
    B, S, H, C = 4, 32, 128, 13
    cfg = BertConfig(512, hidden_size=H, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    model = MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=C)
    synth.fill_module_(model)
    with torch.no_grad():
        for n, p in model.lstm.named_parameters():
            p.mul_(4.0)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    model = icka_amd.set_length_aware(model.cuda().eval())
    b = synth.synthetic_batch(B, S, 49, vocab_size=512, seed=3, layout="BCHW")
    lens = icka_amd.lstm.lengths_of_mask(b["input_mask"]).tolist()
    assert min(lens) >= 1 and min(lens) < S, lens            # the batch has padding, or the test shows nothing
    g = {k: v.cuda() for k, v in b.items()}
    args = dict(input_ids=g["input_ids"], segment_ids=g["segment_ids"], input_mask=g["input_mask"],
                ori_input_ids=g["input_ids"], ori_input_mask=g["input_mask"], ori_segment_ids=g["segment_ids"],
                added_attention_mask=g["added_attention_mask"], visual_embeds_att=g["visual_embeds_att"],
                output_mask=g["input_mask"], labels=g["labels"])
    em = model(**args)
    loss = model(mode="train", **args)
    loss.backward()
    pred, dev_loss = model(mode="dev", **args)
    assert abs(dev_loss.item() - loss.item()) < 1e-4
    ocfg = O.OracleConfig(vocab_size=512, hidden_size=H, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, max_position_embeddings=64)
    _, cross, _ = O.mner_trunk(P, ocfg, b["input_ids"], b["segment_ids"], b["input_mask"], b["added_attention_mask"],
                            b["visual_embeds_att"], 1, 49, False)
    lstm = torch.nn.LSTM(H, H, batch_first=True, bidirectional=True)
    lstm_sd = {k[len("lstm."):]: v for k, v in P.items() if k.startswith("lstm.")}
    x, _ = torch.func.functional_call(lstm, lstm_sd, (torch.nn.utils.rnn.pack_padded_sequence(
        cross, torch.tensor(lens), batch_first=True, enforce_sorted=False),))
    x, _ = torch.nn.utils.rnn.pad_packed_sequence(x, batch_first=True, total_length=S)
    ref_em = F.linear(x, P["classifier.weight"], P["classifier.bias"])
    mask = b["input_mask"].bool()
    crfP = [P["crf.start_transitions"], P["crf.end_transitions"], P["crf.transitions"]]
    rloss = -OC.crf_reduce(OC.crf_llh(ref_em, b["labels"], mask, *crfP), mask, "token_mean")
    rloss.backward()
    err = (em.float().cpu() - ref_em.detach()).abs().max().item()
    gmax = max(v.grad.norm().item() for v in P.values() if v.grad is not None)
    worst = 0.0
    for k, p in model.named_parameters():
        if P[k].grad is None:
            continue
        worst = max(worst, ((p.grad.float().cpu() - P[k].grad).norm() / (P[k].grad.norm() + 1e-4 * gmax)).item())
    print("\n[_gate_1 tagger, length-aware] emissions max abs err %.3e, loss %.4f (oracle %.4f), worst grad rel err %.3e"
          % (err, loss.item(), rloss.item(), worst))
    assert err < 2e-2, err
    assert abs(loss.item() - rloss.item()) < 2e-2 * max(1.0, abs(rloss.item()))
    assert pred == OC.crf_decode(em.float().cpu(), mask, *[p.detach() for p in crfP])
    assert worst < TAGGER_GRAD_BAR, worst
    # the switch changes the result (this batch has padding) and switching it off gives the reference behaviour back
    em_off = icka_amd.set_length_aware(model, False)(**args)
    assert not torch.equal(em_off, em)
