"""CPU: the token-budget batch sampler, the torch restatement of the pack plan (the GPU test pins the plan kernel against it)
and the refusals of set_packed."""
import pytest
import torch

from icka_amd import packing
from icka_amd.packing import TokenBudgetBatchSampler, plan_reference, set_packed


def _lengths(n=500, lo=8, hi=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (n,), generator=g).tolist()


@pytest.mark.parametrize("shuffle", [False, True])
def test_sampler_covers_every_index_once_within_budget(shuffle):
    lengths = _lengths()
    s = TokenBudgetBatchSampler(lengths, max_tokens=1024, max_batch=12, shuffle=shuffle, seed=3)
    batches = list(s)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(len(lengths)))
    for b in batches:
        assert 1 <= len(b) <= 12
        assert sum(lengths[i] for i in b) <= 1024
    assert len(s) == len(batches)


def test_sampler_fills_the_budget_in_order():
    s = TokenBudgetBatchSampler([100, 100, 100, 50, 10], max_tokens=256, max_batch=8)
    assert list(s) == [[0, 1], [2, 3, 4]]


def test_sampler_is_deterministic_per_seed_and_epoch():
    lengths = _lengths(200)
    a = list(TokenBudgetBatchSampler(lengths, 2048, 64, shuffle=True, seed=7))
    b = list(TokenBudgetBatchSampler(lengths, 2048, 64, shuffle=True, seed=7))
    c = list(TokenBudgetBatchSampler(lengths, 2048, 64, shuffle=True, seed=8))
    assert a == b and a != c
    s = TokenBudgetBatchSampler(lengths, 2048, 64, shuffle=True, seed=7)
    s.set_epoch(1)
    assert list(s) != a


def test_sampler_drop_last():
    lengths = [60, 60, 60, 60, 60]            # 2 per batch of 128: the last batch holds one sample and has room for more
    keep = list(TokenBudgetBatchSampler(lengths, 128, 8, drop_last=False))
    drop = list(TokenBudgetBatchSampler(lengths, 128, 8, drop_last=True))
    assert keep == [[0, 1], [2, 3], [4]]
    assert drop == [[0, 1], [2, 3]]
    full = list(TokenBudgetBatchSampler([60, 60, 60, 60], 128, 8, drop_last=True))
    assert full == [[0, 1], [2, 3]]
    by_count = list(TokenBudgetBatchSampler([10] * 6, 1024, 3, drop_last=True))
    assert by_count == [[0, 1, 2], [3, 4, 5]]


def test_sampler_refuses_a_sample_longer_than_the_budget():
    with pytest.raises(ValueError, match="more than max_tokens"):
        TokenBudgetBatchSampler([10, 300], 256)


def _mask(lens, S):
    return (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()


def test_plan_reference_maps():
    lens, S = [1, 5, 8, 3], 8
    p = plan_reference(_mask(lens, S), 128)
    assert p["lens"].tolist() == lens
    assert p["cu_seqlens"].tolist() == [0, 1, 6, 14, 17]
    p2p, pad2pack = p["packed_to_padded"], p["padded_to_packed"]
    assert p2p[17:].eq(-1).all()                       # filler rows
    for b, n in enumerate(lens):
        c0 = p["cu_seqlens"][b].item()
        for s in range(S):
            if s < n:
                assert pad2pack[b * S + s].item() == c0 + s
                assert p2p[c0 + s].item() == b * S + s
            else:
                assert pad2pack[b * S + s].item() == -1
    assert [i for i, v in enumerate(p["cls_of"].tolist()) if v >= 0] == [0, 1, 6, 14]
    assert p["status"].tolist() == [17, 0]


def test_plan_reference_exact_fit_and_overflow():
    S = 128
    fit = plan_reference(_mask([128, 128], S), 256)
    assert fit["cu_seqlens"].tolist() == [0, 128, 256] and fit["status"].tolist() == [256, 0]
    assert fit["packed_to_padded"].ge(0).all()
    over = plan_reference(_mask([100, 100, 100, 20], S), 256)
    # the third sample would end at 300: it and every later sample are dropped; their valid tokens are marked -2
    assert over["cu_seqlens"].tolist() == [0, 100, 200, 200, 200]
    assert over["status"].tolist() == [320, 1]
    assert over["padded_to_packed"].max().item() < 256
    assert over["packed_to_padded"].max().item() < 4 * S
    assert (over["padded_to_packed"].view(4, S)[2:, :20] == -2).all()


def test_plan_reference_flags_a_mask_that_is_not_a_prefix():
    m = _mask([4, 4], 8)
    m[1, 6] = 1
    p = plan_reference(m, 128)
    assert p["status"].tolist() == [4 + 4, 2]
    assert p["padded_to_packed"][8 + 6].item() == -2


@pytest.mark.parametrize("bad", [0, -128, 100, 4097])
def test_set_packed_refuses_bad_max_tokens(bad):
    with pytest.raises(ValueError, match="positive multiple of 128"):
        set_packed(torch.nn.Linear(2, 2), bad)
    with pytest.raises(TypeError, match="max_tokens must be an int"):
        set_packed(torch.nn.Linear(2, 2), 4096.0)


def _tiny(variant="cl", **kw):
    from icka_amd.config import BertConfig
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF
    cfg = BertConfig(64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    return MTCCMBertForMMTokenClassificationCRF(cfg, num_labels=5, variant=variant, max_seq_length=32, **kw)


def test_set_packed_refuses_unsupported_models_and_modes():
    from icka_amd import set_precision
    from icka_amd.config import BertConfig
    with pytest.raises(NotImplementedError, match="gate_cl"):
        set_packed(_tiny("gate_cl"), 4096)
    with pytest.raises(NotImplementedError, match="fp8"):
        set_packed(_tiny(cross_attention_fp8=True), 4096)
    for prec in ("fp32", "mixed16"):
        with pytest.raises(NotImplementedError, match=prec):
            set_packed(set_precision(_tiny(), prec), 4096)
    with pytest.raises(NotImplementedError, match="MTCCMBertForMMTokenClassificationCRF"):
        set_packed(torch.nn.Linear(2, 2), 4096)
    from icka_amd.modeling import MTCCMBertForMMTokenClassificationCRF_gate_1
    cfg = BertConfig(64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    with pytest.raises(NotImplementedError, match="_gate_1"):
        set_packed(MTCCMBertForMMTokenClassificationCRF_gate_1(cfg, num_labels=5), 4096)
    m = _tiny()
    assert set_packed(m, 4096) is m and packing.state_of(m).max_tokens == 4096
    with pytest.raises(NotImplementedError, match="S=256"):
        packing.validate(m, 256)
    set_packed(m, None)
    assert packing.state_of(m) is None


def test_set_packed_refuses_the_cross_modal_model():
    from icka_amd import cross_modal
    cls = [getattr(cross_modal, n) for n in dir(cross_modal) if isinstance(getattr(cross_modal, n), type)
           and issubclass(getattr(cross_modal, n), torch.nn.Module) and getattr(cross_modal, n).__module__ == cross_modal.__name__]
    assert cls
    for c in cls:
        obj = c.__new__(c)
        torch.nn.Module.__init__(obj)
        with pytest.raises(NotImplementedError, match="only"):
            set_packed(obj, 4096)


def test_a_copied_pack_state_does_not_carry_the_error_word():
    """The error word is pinned host memory the plan kernel stores to.  A deep copy or a pickle round trip of the model would
    copy it into ordinary pageable memory (and detach the numpy view that reads it): the copy must drop it and make its own."""
    import copy
    import io
    st = packing.PackState(4096)
    st._err = torch.tensor([5000, 1], dtype=torch.int32)      # stands in for a word set by an overflowing batch
    st._err_np = st._err.numpy()
    c = copy.deepcopy(st)
    assert c is not st and c.max_tokens == 4096 and c._err is None and c._err_np is None
    assert st._err is not None                                 # the original keeps its word
    buf = io.BytesIO()
    torch.save(st, buf)
    buf.seek(0)
    p = torch.load(buf, weights_only=False)
    assert p.max_tokens == 4096 and p._err is None and p._err_np is None
    m = _tiny()
    set_packed(m, 512)
    packing.state_of(m)._err = torch.zeros(2, dtype=torch.int32)
    m2 = copy.deepcopy(m)
    assert packing.state_of(m2) is not packing.state_of(m) and packing.state_of(m2)._err is None


def test_every_data_parallel_entry_point_refuses_a_packed_model():
    from icka_amd.graph import FlaggedStep, GraphedModule, SegmentedStep, build_step
    m = set_packed(_tiny(), 512)
    reducer = object()                      # never reached: the refusal comes first
    with pytest.raises(NotImplementedError, match="FlaggedStep"):
        FlaggedStep(m, lambda: None, reducer)
    with pytest.raises(NotImplementedError, match="SegmentedStep"):
        SegmentedStep(m, lambda: None, reducer)
    with pytest.raises(NotImplementedError, match=r"build_step\(reducer=\)"):
        build_step(m, lambda: None, reducer=reducer)
    with pytest.raises(NotImplementedError, match=r"GraphedModule\(reducer=\)"):
        GraphedModule(m, (), {}, reducer=reducer)
