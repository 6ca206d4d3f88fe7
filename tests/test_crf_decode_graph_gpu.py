"""GPU: capturable CRF decoding.  icka_crf_score_decode against icka_crf_decode / icka_crf_llh (same tags, bitwise-equal llh)
and brute force; and the reference's dev / test passes (My_cross_attention.py:846-875, :1022, :1047-1050) replayed through
``GraphedModule(..., decode=True)``: the lists and bitwise dev losses of the eager model, no eager call."""
import copy

import pytest
import torch

import icka_amd
from icka_amd import crf as crf_mod
from icka_amd import kernels as K
from icka_amd import synth

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _masks(B, S, g, kind):
    if kind == "none":
        return None
    if kind == "full":
        return torch.ones(B, S, dtype=torch.int64)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1                                         # one sample with a single tag
    m = (torch.arange(S)[None, :] < lens[:, None]).long()
    if kind == "holes":                                     # first-sub-word masks (the published model's output_mask)
        m = m * (torch.rand(B, S, generator=g) > 0.3).long()
        m[:, 0] = 1
        if B > 2:
            m[2, 0] = 0                                     # (rejected by the package; both kernels stay consistent)
        if B > 1:
            m[1] = 0
            m[1, 0] = 1
    return m


def _score_decode(crf, e, tags, mask):
    B, S = e.shape[:2]
    out = crf_mod.DeviceTags.empty(B, S, e.device)
    llh = torch.empty(B, dtype=F32, device=e.device) if tags is not None else None
    K.crf_score_decode(e, tags, mask, crf.start_transitions.detach(), crf.end_transitions.detach(),
                       crf.transitions.detach(), llh, out.lens, out.tags_flat)
    return out, llh


@pytest.mark.parametrize("B,S,Cn", [(32, 128, 13), (8, 128, 15), (2, 400, 13), (5, 40, 33), (4, 600, 9), (3, 7, 64),
                                    (1, 1, 4), (64, 32, 13)])
@pytest.mark.parametrize("kind", ["ragged", "holes", "full", "none"])
def test_score_decode_matches_decode_and_llh(B, S, Cn, kind):
    """Both LDS regimes (C <= 16 and S <= 512: registers + shuffles, staged or not; else the LDS kernels), prefix and
    non-prefix masks, a sample with one tag, masks that fill B*S = capacity exactly."""
    g = torch.Generator().manual_seed(B * 7919 + S * 31 + Cn)
    torch.manual_seed(B + S + Cn)
    crf = crf_mod.CRF(Cn, batch_first=True).cuda()
    e = (torch.randn(B, S, Cn, generator=g) * 2.0).cuda()
    tags = torch.randint(0, Cn, (B, S), generator=g).cuda()
    m = _masks(B, S, g, kind)
    m = m.cuda() if m is not None else None
    ref_tags = crf.decode(e, mask=m)                                         # icka_crf_decode
    ref_llh = torch.empty(B, dtype=F32, device="cuda")
    K.crf_llh(e, tags, m, crf.start_transitions.detach(), crf.end_transitions.detach(), crf.transitions.detach(), ref_llh)
    out, llh = _score_decode(crf, e, tags, m)
    assert out.tolist() == ref_tags
    assert torch.equal(llh.view(torch.int32), ref_llh.view(torch.int32)), (llh - ref_llh).abs().max().item()
    assert out.lens.tolist() == [len(r) for r in ref_tags]
    if kind in ("full", "none"):
        assert sum(out.lens.tolist()) == B * S == out.capacity
    out2, none = _score_decode(crf, e, None, m)                             # decode only
    assert none is None and out2.tolist() == ref_tags
    with crf_mod.device_decode():                                            # the module's switch
        dt = crf.decode(e, mask=m)
        dt2, llh_tm = crf.decode_llh(e, tags, mask=m, reduction="token_mean")
    assert isinstance(dt, crf_mod.DeviceTags) and dt.tolist() == ref_tags and dt2.tolist() == ref_tags
    with torch.no_grad():
        eager = crf(e, tags, mask=m, reduction="token_mean")
    assert torch.equal(llh_tm, eager)


def test_score_decode_log_domain_fallback_is_bitwise():
    """Forbidden (-1e4) transitions and wide emissions: the scaled likelihood gives up on such samples and the log-domain body
    (inline in the new kernel, step flags from LDS) computes them; still the bits of icka_crf_llh."""
    B, S, Cn = 6, 48, 13
    g = torch.Generator().manual_seed(5)
    crf = crf_mod.CRF(Cn, batch_first=True).cuda()
    with torch.no_grad():
        crf.transitions[:, 1:] = -1e4
        crf.transitions[0, 1:] = 0.0
    e = (torch.randn(B, S, Cn, generator=g) * 40.0).cuda()
    tags = torch.randint(0, Cn, (B, S), generator=g).cuda()
    m = _masks(B, S, g, "holes").cuda()
    ref_llh = torch.empty(B, dtype=F32, device="cuda")
    K.crf_llh(e, tags, m, crf.start_transitions.detach(), crf.end_transitions.detach(), crf.transitions.detach(), ref_llh)
    out, llh = _score_decode(crf, e, tags, m)
    assert out.tolist() == crf.decode(e, mask=m)
    assert torch.equal(llh.view(torch.int32), ref_llh.view(torch.int32))


def test_score_decode_against_brute_force():
    from oracle import crf_oracle as O
    for S, Cn in ((1, 3), (3, 4), (5, 3), (4, 5)):
        B = 4
        g = torch.Generator().manual_seed(S * 10 + Cn)
        torch.manual_seed(S * 10 + Cn)
        crf = crf_mod.CRF(Cn, batch_first=True).cuda()
        e = torch.randn(B, S, Cn, generator=g)
        tags = torch.randint(0, Cn, (B, S), generator=g)
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0] = S
        mask = (torch.arange(S)[None, :] < lens[:, None]).long()
        out, llh = _score_decode(crf, e.cuda(), tags.cuda(), mask.cuda())
        paths = out.tolist()
        st, en, tr = (p.detach().cpu() for p in (crf.start_transitions, crf.end_transitions, crf.transitions))
        ollh = O.crf_llh(e, tags, mask.bool(), st, en, tr)
        for b in range(B):
            logz, best, _ = O.brute_force(e[b], int(lens[b]), st, en, tr)
            assert paths[b] == best
            gold = st[tags[b, 0]] + e[b, 0, tags[b, 0]]
            for i in range(1, int(lens[b])):
                gold = gold + tr[tags[b, i - 1], tags[b, i]] + e[b, i, tags[b, i]]
            gold = gold + en[tags[b, int(lens[b]) - 1]]
            assert abs(llh[b].item() - (gold - logz).item()) < 1e-4
            assert abs(llh[b].item() - ollh[b].item()) < 1e-4


def test_score_decode_argument_errors():
    crf = crf_mod.CRF(5, batch_first=True).cuda()
    e = torch.randn(2, 4, 5, device="cuda")
    with pytest.raises(ValueError):                                          # capacity too small
        crf.decode(e, out=crf_mod.DeviceTags(torch.zeros(2, dtype=torch.int32, device="cuda"),
                                             torch.zeros(7, dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):                                          # tags without llh
        out = crf_mod.DeviceTags.empty(2, 4, "cuda")
        K.crf_score_decode(e, torch.zeros(2, 4, dtype=torch.int64, device="cuda"), None, crf.start_transitions.detach(),
                           crf.end_transitions.detach(), crf.transitions.detach(), None, out.lens, out.tags_flat)
    with pytest.raises(ValueError):                                          # B above what the kernel sums itself
        big = torch.randn(K.CRF_FLAT_MAX_B + 1, 1, 5, device="cuda")
        crf.decode(big, out=crf_mod.DeviceTags.empty(K.CRF_FLAT_MAX_B + 1, 1, "cuda"))
    out = crf_mod.DeviceTags.empty(2, 4, "cuda")
    assert crf.decode(e, out=out) is out and out.tolist() == crf.decode(e)


# ------------------------------------------------------------------------------------------------- the reference's loop
def _holes(b, seed):
    """output_mask of first sub-words: the input mask with holes, position 0 on."""
    g = torch.Generator().manual_seed(seed)
    m = b["output_mask"].clone() * (torch.rand(b["output_mask"].shape, generator=g) > 0.25).long()
    m[:, 0] = 1
    return m


def _per_step_lstm(model):
    """The per-step BiLSTM launches: the persistent form needs its grid co-resident, which a GPU shared with other
    processes does not guarantee (it then raises LstmHandoffError); these tests are about decoding."""
    from icka_amd import _lib
    model.lstm.recurrence_flags = _lib.LSTM_PER_STEP
    return model


def _gate1_case():
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=13)
    synth.fill_module_(m)
    with torch.no_grad():
        for _, p in m.lstm.named_parameters():
            p.mul_(4.0)
    _per_step_lstm(m)

    def batch(n, seed):
        b = synth.synthetic_prompt_batch(n, 32, vocab_size=512, roberta_vocab=600, prompt_tokens=17, total_len=60,
                                         seed=seed)
        b["output_mask"] = _holes(b, seed)
        return {k: v.cuda() for k, v in b.items()}
    return m, batch


def _published_case():
    import os
    import sys
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    from test_cross_modal_cpu import build_case
    fx = np.load(os.path.join(here, "golden", "cross_modal_h1024_l1.npz"))
    model, _, _, _ = build_case(fx)
    _per_step_lstm(model)
    c = {k[4:]: int(fx[k]) for k in fx.files if k.startswith("cfg_")}

    def batch(n, seed):
        b = synth.synthetic_prompt_batch(n, c["S"], vocab_size=c["vocab"], roberta_vocab=c["rvocab"],
                                         prompt_tokens=c["prompt_tokens"], total_len=c["total_len"],
                                         num_labels=c["num_labels"], seed=seed)
        b["output_mask"] = _holes(b, seed)
        return {k: v.cuda() for k, v in b.items()}
    return model, batch


PROMPT_NAMES = ("input_ids", "segment_ids", "input_mask", "ori_input_ids", "ori_input_mask", "ori_segment_ids",
                "added_attention_mask", "clip_features", "visual_embeds_mean", "visual_embeds_att", "offsets", "output_mask")


def _prompt_calls(batch):
    """(train, dev, test) call of the gated / published taggers on one batch: (args, kwargs)."""
    args = tuple(batch[k] for k in PROMPT_NAMES)
    return ((args, {"labels": batch["labels"], "mode": "train"}), (args, {"labels": batch["labels"], "mode": "dev"}),
            (args, {"mode": "test"}))


def _cl_case():
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = MTCCMBertForMMTokenClassificationCRF(cfg, layer_num1=1, num_labels=13, regions=36, variant="cl", use_crf=True)
    synth.fill_module_(m)

    def batch(n, seed):
        b = synth.synthetic_batch(n, 32, 36, vocab_size=512, seed=seed)
        return {k: v.cuda() for k, v in b.items()}
    return m, batch


CL_NAMES = ("input_ids", "segment_ids", "input_mask", "added_attention_mask", "visual_embeds_mean", "visual_embeds_att")


def _cl_calls(batch):
    """cl_modeling.py: loss with labels (:1380), decode without (:1386); the dev pass is decode only."""
    args = tuple(batch[k] for k in CL_NAMES)
    return (args, {"labels": batch["labels"]}), (args, {}), (args, {})


CASES = {"gate_1": (_gate1_case, _prompt_calls), "published": (_published_case, _prompt_calls), "cl": (_cl_case, _cl_calls)}


def _eval_passes(call, model, batch, calls, eval_bs=3):
    """Two dev passes at eval_batch_size (the second one ends on a short batch), then the test pass at batch 4 (short last)."""
    dev1 = [batch(eval_bs, 300), batch(eval_bs, 301)]
    dev2 = [batch(eval_bs, 302), batch(eval_bs, 303), batch(eval_bs - 1, 304)]
    test = [batch(4, 400), batch(4, 401), batch(2, 402)]
    out = []
    model.eval()
    with torch.no_grad():
        for b in dev1 + dev2:
            args, kw = calls(b)[1]
            r = call(*args, **kw)
            out.append((r[0], r[1].float().cpu().clone()) if isinstance(r, tuple) else r)
        for b in test:
            args, kw = calls(b)[2]
            out.append(call(*args, **kw))
    return out


def _same(eager, graphed):
    assert len(eager) == len(graphed)
    losses = [(a[1], b[1]) for a, b in zip(eager, graphed) if isinstance(a, tuple)]
    print("    dev losses bitwise equal: %d of %d" % (sum(torch.equal(x, y) for x, y in losses), len(losses)))
    for a, b in zip(eager, graphed):
        if isinstance(a, tuple):
            assert isinstance(b, tuple) and type(b[0]) is list and b[0] == a[0]
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (a[1], b[1])   # bitwise
        else:
            assert type(b) is list and all(type(r) is list for r in b) and b == a


@pytest.mark.parametrize("case", ["gate_1", "published", "cl"])
def test_dev_and_test_passes_replay_with_decode(case):
    make, calls = CASES[case]
    base, batch = make()
    base = base.cuda()
    eager_model = copy.deepcopy(base)
    ref = _eval_passes(eager_model, eager_model, batch, calls)
    model = copy.deepcopy(base).train()
    (targs, tkw) = calls(batch(4, 200))[0]
    gm = icka_amd.graph.GraphedModule(model, targs, tkw, decode=True, max_captures=8)
    got = _eval_passes(gm, gm, batch, calls)
    print("\n[%s, decode=True] %s" % (case, gm.stats))
    _same(ref, got)
    assert gm.stats["eager_calls"] == 0, gm.stats
    # the train call, dev at 3, dev short (2), test at 4, test short (2); cl: its dev and test calls are the same call
    assert gm.captures == (4 if case == "cl" else 5), gm.stats
    # a second round replays every capture
    got2 = _eval_passes(gm, gm, batch, calls)
    _same(ref, got2)
    assert gm.stats["eager_calls"] == 0 and gm.captures == (4 if case == "cl" else 5), gm.stats
    gm.close()


def test_decode_capture_interleaved_with_training_matches_eager_loop():
    """Two epochs of the reference's loop on _gate_1 in fp32 (train steps with AdamW, short last train batch, dev pass per
    epoch, then the test pass): the train losses as tests/test_whole_loop_gpu.py bounds them, the same predictions."""
    from icka_amd.optim import reference_param_groups
    base, batch = _gate1_case()
    base = icka_amd.set_precision(base.cuda(), "fp32")
    train = [batch(4, 200), batch(4, 201), batch(2, 202)]
    dev = [batch(3, 300), batch(3, 301), batch(2, 302)]
    test = [batch(4, 400), batch(1, 401)]

    def loop(model):
        opt = torch.optim.AdamW(reference_param_groups(model, 0.01), lr=1e-3)
        losses, dev_out = [], []
        for _ in range(2):
            model.train()
            for b in train:
                model.zero_grad()
                args, kw = _prompt_calls(b)[0]
                loss = model(*args, **kw)
                loss.backward()
                losses.append(loss.item())
                opt.step()
            model.eval()
            with torch.no_grad():
                for b in dev:
                    args, kw = _prompt_calls(b)[1]
                    tags, loss = model(*args, **kw)
                    dev_out.append((tags, loss.item()))
        with torch.no_grad():
            for b in test:
                args, kw = _prompt_calls(b)[2]
                dev_out.append((model(*args, **kw), None))
        return losses, dev_out

    le, de = loop(copy.deepcopy(base))
    targs, tkw = _prompt_calls(train[0])[0]
    gm = icka_amd.graph.GraphedModule(copy.deepcopy(base), targs, tkw, decode=True, max_captures=8)
    lg, dg = loop(gm)
    print("\n[_gate_1 loop, decode=True] %s" % gm.stats)
    assert gm.stats["eager_calls"] == 0, gm.stats
    assert gm.captures == 6, gm.stats      # train 4, train 2, dev 3, dev 2, test 4, test 1
    bar = 3e-5
    for a, b in zip(le, lg):
        assert abs(a - b) <= bar * max(1.0, abs(a)), (le, lg)
    same = total = 0
    for (ta, la), (tb, lb) in zip(de, dg):
        assert type(tb) is list
        if la is not None:
            assert abs(la - lb) <= 1e-3 * max(1.0, abs(la)), (la, lb)
        for ra, rb in zip(ta, tb):
            assert len(ra) == len(rb)
            same += sum(int(x == y) for x, y in zip(ra, rb))
            total += len(ra)
    # parameters differ by the f32 atomics' order (test_whole_loop_gpu.py): a near-tie may flip a tag
    assert same >= 0.99 * total, (same, total)
    gm.close()


def test_decode_past_max_captures_runs_eagerly():
    base, batch = _gate1_case()
    base = base.cuda()
    eager_model = copy.deepcopy(base)
    ref = _eval_passes(eager_model, eager_model, batch, _prompt_calls)
    targs, tkw = _prompt_calls(batch(4, 200))[0]
    gm = icka_amd.graph.GraphedModule(copy.deepcopy(base).train(), targs, tkw, decode=True, max_captures=2)
    got = _eval_passes(gm, gm, batch, _prompt_calls)
    _same(ref, got)
    assert gm.captures == 2 and gm.stats["eager_calls"] == len(ref) - gm.stats["replays"] > 0, gm.stats
    gm.close()


def test_decode_false_keeps_dev_and_test_calls_eager():
    base, batch = _gate1_case()
    base = base.cuda()
    eager_model = copy.deepcopy(base)
    ref = _eval_passes(eager_model, eager_model, batch, _prompt_calls)
    targs, tkw = _prompt_calls(batch(4, 200))[0]
    gm = icka_amd.graph.GraphedModule(copy.deepcopy(base).train(), targs, tkw, max_captures=8)
    got = _eval_passes(gm, gm, batch, _prompt_calls)
    for a, b in zip(ref, got):
        if isinstance(a, tuple):
            assert b[0] == a[0] and torch.equal(a[1], b[1])
        else:
            assert b == a
    assert gm.captures == 1 and gm.stats["eager_calls"] == len(ref) and gm.stats["replays"] == 0, gm.stats
    gm.close()
