"""GPU: icka_chunk_eval / ChunkEvaluator against the fixture recorded from the reference's ner_evaluate.py and against the
Python restatement (metrics.filter_batch + evaluate_lists), and the sync-free dev loop GraphedModule(decode="device") +
ChunkEvaluator against the eager model's lists.  Every comparison of counts is exact."""
import copy
import os

import numpy as np
import pytest
import torch

import icka_amd
from icka_amd import crf as crf_mod
from icka_amd import metrics as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LMAP = M.label_list_map(M.REFERENCE_LABEL_LIST)
L = len(LMAP)


def _fx():
    f = np.load(os.path.join(HERE, "golden", "chunk_eval.npz"))
    return {k: f[k] for k in f.files}


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).cuda()


def _n0(mask_row):
    z = np.flatnonzero(np.asarray(mask_row) == 0)
    return int(z[0]) if z.size else len(mask_row)


def _device_tags(pred, mask, rng, extra=True):
    """pred [B, S] as back-to-back paths: path b = pred[b, :len_b] with n0_b <= len_b <= S (what the kernel may rely on)."""
    pred, mask = np.asarray(pred), np.asarray(mask)
    B, S = pred.shape
    lens = [max(1, int(rng.integers(_n0(mask[b]), S + 1)) if extra else _n0(mask[b])) for b in range(B)]
    flat = np.concatenate([pred[b, :lens[b]] for b in range(B)])
    buf = np.full(B * S, -7, dtype=np.int64)          # entries past the paths are never read
    buf[:len(flat)] = flat
    return crf_mod.DeviceTags(torch.tensor(lens, dtype=torch.int32).cuda(), torch.as_tensor(buf, dtype=torch.int32).cuda())


def _host_scores(batches):
    pl, gl = [], []
    for pred, labels, mask in batches:
        p, g = M.filter_batch(np.asarray(pred).tolist(), np.asarray(labels), np.asarray(mask), LMAP)
        pl += p
        gl += g
    return M.evaluate_lists(pl, gl, LMAP)


def _same(a, b):
    assert a.counts == b.counts, (a.counts, b.counts)
    assert a.per_class_counts == b.per_class_counts
    for x, y in zip(tuple(a), tuple(b)):
        assert (np.isnan(x) and np.isnan(y)) or np.float64(x).view(np.int64) == np.float64(y).view(np.int64)


@pytest.mark.parametrize("form", ["padded", "flat", "lists"])
def test_kernel_equals_the_reference_fixture(form):
    fx = _fx()
    rng = np.random.default_rng(1)
    ev = M.ChunkEvaluator.for_label_list([str(s) for s in fx["label_list"]])
    for n in range(fx["labels"].shape[0]):
        pred = {"padded": lambda: _dev(fx["preds"][n]), "flat": lambda: _device_tags(fx["preds"][n], fx["masks"][n], rng),
                "lists": lambda: fx["preds"][n].tolist()}[form]()
        ev.update(pred, _dev(fx["labels"][n]), _dev(fx["masks"][n]))
    sc = ev.compute()
    assert [sc.counts["correct_preds"], sc.counts["total_preds"], sc.counts["total_correct"]] == fx["counts"].tolist()
    assert sc.counts["kept_tokens"] == int(fx["list_len"].sum())
    for got, want in zip(tuple(sc), fx["evaluate"]):
        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64)
    types = [str(s) for s in fx["types"]]
    for i, t in enumerate(types):
        if t != "O":
            assert [np.float64(v).view(np.int64) for v in sc.per_class[t]] == [v.view(np.int64) for v in fx["each_class"][i]]
    _same(sc, _host_scores([(fx["preds"][n], fx["labels"][n], fx["masks"][n]) for n in range(fx["labels"].shape[0])]))


def test_accumulation_equals_one_update_on_the_concatenation():
    fx = _fx()
    a, b = M.ChunkEvaluator(LMAP), M.ChunkEvaluator(LMAP)
    for n in range(3):
        a.update(_dev(fx["preds"][n]), _dev(fx["labels"][n]), _dev(fx["masks"][n]))
    b.update(_dev(fx["preds"].reshape(96, -1)), _dev(fx["labels"].reshape(96, -1)), _dev(fx["masks"].reshape(96, -1)))
    assert torch.equal(a.counters, b.counters)
    a.reset()
    assert int(a.counters.abs().sum()) == 0


def _random_case(B, S, rng, kind):
    """Gold over the 15 ids with entity runs, predictions = gold with 30 % redrawn over all ids (tag 0 and the special labels
    among them), ragged prefix masks with one non-prefix row."""
    ids = np.arange(L)
    labels = rng.choice(ids, size=(B, S), p=np.array([1, 8, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1]) / 40.0)
    mask = (np.arange(S)[None, :] < rng.integers(0, S + 1, (B, 1))).astype(np.int64)
    mask[0] = 1
    if B > 2 and S > 2:
        mask[2, S // 2] = 0
    if kind == "all_O":
        labels[:] = 1
    elif kind == "all_skipped":
        labels[:] = rng.choice([10, 11, 12, 13, 14], size=(B, S))
    elif kind == "zero_mask":
        mask[:] = 0
    elif kind == "entity_to_end" and S >= 3:
        labels[:, -3:] = [4, 5, 5]                     # B-PER I-PER I-PER up to the last kept token of the full rows
    redraw = rng.random((B, S)) < 0.3
    pred = np.where(redraw, rng.integers(0, L, (B, S)), labels)
    if kind == "all_O":
        pred = np.where(rng.random((B, S)) < 0.05, rng.integers(0, L, (B, S)), labels)
    return pred, labels, mask


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 256, 512])
@pytest.mark.parametrize("B", [1, 4, 32, 200])
def test_random_cases_equal_evaluate_lists(B, S):
    rng = np.random.default_rng(B * 1000 + S)
    for kind in ("random", "all_O", "all_skipped", "zero_mask", "entity_to_end"):
        pred, labels, mask = _random_case(B, S, rng, kind)
        want = _host_scores([(pred, labels, mask)])
        for form in ("padded", "flat", "flat_tight"):
            ev = M.ChunkEvaluator(LMAP)
            p = _dev(pred) if form == "padded" else _device_tags(pred, mask, rng, extra=form == "flat")
            ev.update(p, _dev(labels), _dev(mask))
            _same(ev.compute(), want)
            if kind in ("all_skipped", "zero_mask"):
                assert np.isnan(ev.compute().acc) and ev.compute().counts["kept_tokens"] == 0


def test_strided_prediction_rows():
    rng = np.random.default_rng(9)
    pred, labels, mask = _random_case(8, 100, rng, "random")
    wide = torch.full((8, 160), 3, dtype=torch.int64, device="cuda")
    wide[:, :100] = _dev(pred)
    ev = M.ChunkEvaluator(LMAP)
    ev._ensure()
    icka_amd.kernels.chunk_eval(_dev(labels), _dev(mask), ev._table, ev.counters, len(ev.types), pred=wide[:, :100])
    _same(ev.compute(), _host_scores([(pred, labels, mask)]))


def test_bad_ids_are_counted_and_leave_the_counters_alone():
    rng = np.random.default_rng(5)
    pred, labels, mask = _random_case(6, 70, rng, "random")
    mask[:] = 1
    labels[:, 10] = 1                                   # a kept position in every row
    good = M.ChunkEvaluator(LMAP)
    keep = [0, 2, 4]
    good.update(_dev(pred[keep]), _dev(labels[keep]), _dev(mask[keep]))
    bad_pred, bad_labels = pred.copy(), labels.copy()
    bad_pred[1, 10] = L                                 # predicted id out of range at a kept position
    bad_pred[3, 10] = -1
    bad_labels[5, 69] = 99                              # gold id out of range
    ev = M.ChunkEvaluator(LMAP)
    ev.update(_dev(bad_pred), _dev(bad_labels), _dev(mask))
    assert ev.counters.tolist()[5] == 3
    assert ev.counters.tolist()[:5] == good.counters.tolist()[:5] and ev.counters.tolist()[6:] == good.counters.tolist()[6:]
    with pytest.raises(ValueError):
        ev.compute()
    # a path shorter than its sample's kept range
    short = M.ChunkEvaluator(LMAP)
    lens = torch.tensor([70, 69, 70, 70, 70, 70], dtype=torch.int32).cuda()
    flat = torch.as_tensor(np.concatenate([pred[b, :n] for b, n in enumerate(lens.tolist())]), dtype=torch.int32).cuda()
    short.update(crf_mod.DeviceTags(lens, flat), _dev(labels), _dev(mask))
    ref = M.ChunkEvaluator(LMAP)
    sel = [0, 2, 3, 4, 5]
    ref.update(_dev(pred[sel]), _dev(labels[sel]), _dev(mask[sel]))
    assert short.counters.tolist()[5] == 1 and short.counters.tolist()[:5] == ref.counters.tolist()[:5]
    with pytest.raises(ValueError):
        short.compute()
    # python lists that end early are refused the same way
    lst = M.ChunkEvaluator(LMAP)
    rows = pred.tolist()
    rows[1] = rows[1][:20]
    lst.update(rows, _dev(labels), _dev(mask))
    assert lst.counters.tolist()[5] == 1


def test_update_captured_in_a_graph_equals_eager_updates():
    rng = np.random.default_rng(11)
    cases = [_random_case(16, 128, rng, "random") for _ in range(4)]
    ev = M.ChunkEvaluator(LMAP)
    sp, sl, sm = (_dev(x) for x in cases[0])
    loss = torch.zeros((), device="cuda")
    ev.update(sp, sl, sm); ev.add_loss(loss)            # warm-up (allocations) outside the capture
    ev.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.update(sp, sl, sm)
        ev.add_loss(loss)
    ev.reset()
    losses = [0.1, 0.7, 1.3]
    for (p, l, m), lv in zip(cases[1:], losses):
        sp.copy_(_dev(p)); sl.copy_(_dev(l)); sm.copy_(_dev(m)); loss.fill_(lv)
        g.replay()
    eager = M.ChunkEvaluator(LMAP)
    for (p, l, m), lv in zip(cases[1:], losses):
        eager.update(_dev(p), _dev(l), _dev(m))
        eager.add_loss(torch.tensor(lv, device="cuda"))
    assert torch.equal(ev.counters, eager.counters)
    got, want = ev.compute(), eager.compute()
    _same(got, _host_scores(cases[1:]))
    host_mean = sum(torch.tensor(v, dtype=torch.float32).item() for v in losses) / 3
    assert got.mean_loss == want.mean_loss == host_mean


def test_deferred_check_runs_in_compute():
    ev = M.ChunkEvaluator(LMAP)
    rng = np.random.default_rng(3)
    pred, labels, mask = _random_case(2, 16, rng, "random")
    tags = _device_tags(pred, mask, rng)
    calls = []

    def boom():
        calls.append(1)
        raise icka_amd.kernels.LstmHandoffError("hand-off failed in a replay")
    tags.deferred_check = boom
    ev.update(tags, _dev(labels), _dev(mask))
    with pytest.raises(icka_amd.kernels.LstmHandoffError):
        ev.compute()
    ev.reset()
    ev.update(_dev(pred), _dev(labels), _dev(mask))
    ev.compute()
    assert calls == [1]


# ------------------------------------------------------------------------------------------------- the reference's dev loop
def _gate1_case():
    from icka_amd import _lib, synth
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
    cfg = BertConfig(512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=L)
    synth.fill_module_(m)
    with torch.no_grad():
        for _, p in m.lstm.named_parameters():
            p.mul_(4.0)
    # the per-step BiLSTM launches: the persistent form needs its grid co-resident, which a shared GPU does not guarantee
    m.lstm.recurrence_flags = _lib.LSTM_PER_STEP

    def batch(n, seed):
        b = synth.synthetic_prompt_batch(n, 32, vocab_size=512, roberta_vocab=600, prompt_tokens=17, total_len=60,
                                         num_labels=L, seed=seed)
        g = torch.Generator().manual_seed(seed)
        lens = b["output_mask"].sum(1)
        b["output_mask"] = (torch.arange(32)[None, :] < torch.clamp(lens - torch.randint(0, 3, lens.shape, generator=g), min=1)[:, None]).long()
        return {k: v.cuda() for k, v in b.items()}
    return m, batch


NAMES = ("input_ids", "segment_ids", "input_mask", "ori_input_ids", "ori_input_mask", "ori_segment_ids",
         "added_attention_mask", "clip_features", "visual_embeds_mean", "visual_embeds_att", "offsets", "output_mask")


def test_dev_loop_on_device_equals_the_eager_lists():
    base, batch = _gate1_case()
    base = base.cuda()
    dev = [batch(3, 300), batch(3, 301), batch(3, 302), batch(2, 303)]
    test = [batch(4, 400), batch(4, 401)]
    eager = copy.deepcopy(base).eval()
    pl, gl = [], []
    with torch.no_grad():
        for b in dev:
            tags, _ = eager(*[b[k] for k in NAMES], labels=b["labels"], mode="dev")
            p, g = M.filter_batch(tags, b["labels"].cpu(), b["output_mask"].cpu(), LMAP)
            pl += p
            gl += g
    want = M.evaluate_lists(pl, gl, LMAP)
    assert want.counts["kept_tokens"] > 0 and want.counts["total_correct"] > 0

    tb = batch(4, 200)
    targs, tkw = tuple(tb[k] for k in NAMES), {"labels": tb["labels"], "mode": "train"}
    lists = icka_amd.graph.GraphedModule(copy.deepcopy(base).train(), targs, tkw, decode=True, max_captures=8)
    lists.eval()
    host_losses = []
    with torch.no_grad():
        for b in dev:
            tags, loss = lists(*[b[k] for k in NAMES], labels=b["labels"], mode="dev")
            assert type(tags) is list and all(type(r) is list for r in tags)       # decode=True still returns lists
            host_losses.append(loss.item())
    assert lists.decode is True
    lists.close()

    gm = icka_amd.graph.GraphedModule(copy.deepcopy(base).train(), targs, tkw, decode="device", max_captures=8)
    assert gm.decode == "device"
    gm.eval()
    ev = M.ChunkEvaluator(LMAP)
    with torch.no_grad():
        for rnd in range(2):                            # the second round replays every capture
            ev.reset()
            before = dict(gm.stats)
            for b in dev:
                tags, loss = gm(*[b[k] for k in NAMES], labels=b["labels"], mode="dev")
                assert isinstance(tags, crf_mod.DeviceTags) and tags.deferred_check is not None
                ev.update(tags, b["labels"], b["output_mask"])
                ev.add_loss(loss)
            got = ev.compute()
            _same(got, want)
            assert got.mean_loss == sum(host_losses) / len(host_losses)
        assert gm.stats["replays"] - before["replays"] == len(dev) and gm.stats["captures"] == before["captures"]
        for b in test:
            tags = gm(*[b[k] for k in NAMES], mode="test")
            assert isinstance(tags, crf_mod.DeviceTags)
            assert tags.tolist() == eager(*[b[k] for k in NAMES], mode="test")
    assert gm.stats["eager_calls"] == 0, gm.stats
    gm.close()


def test_decode_device_past_max_captures_returns_device_tags_eagerly():
    base, batch = _gate1_case()
    base = base.cuda()
    tb = batch(4, 200)
    targs, tkw = tuple(tb[k] for k in NAMES), {"labels": tb["labels"], "mode": "train"}
    gm = icka_amd.graph.GraphedModule(copy.deepcopy(base).train(), targs, tkw, decode="device", max_captures=1)
    gm.eval()
    b = batch(3, 300)
    with torch.no_grad():
        tags, loss = gm(*[b[k] for k in NAMES], labels=b["labels"], mode="dev")
        ref_tags, ref_loss = copy.deepcopy(base).eval()(*[b[k] for k in NAMES], labels=b["labels"], mode="dev")
    assert isinstance(tags, crf_mod.DeviceTags) and tags.deferred_check is not None and gm.stats["eager_calls"] == 1
    assert tags.tolist() == ref_tags and torch.equal(loss, ref_loss)
    gm.close()
