"""CPU: the joint-buffer layouts of ``ConstrainedPaths``, ``CrfPosterior`` and ``NBestPaths`` (icka_amd/crf.py) against offsets
worked out by hand from the class docstrings.  The three classes only allocate, so they are built on the CPU: B = 3, S = 5
(capacity 15), nbest = 2.  ``entities.py`` and the graphed evaluation slice these buffers by the same offsets."""
import pytest
import torch

from icka_amd.crf import ConstrainedPaths, CrfPosterior, DeviceTags, NBestPaths

F32, I32 = torch.float32, torch.int32
B, S, CAP, NBEST = 3, 5, 15, 2


def _fill(obj):
    """joint[i] = i; returns the host copy that ``unpack`` takes."""
    obj.joint.copy_(torch.arange(obj.joint.numel(), dtype=I32))
    return obj.joint.cpu()


def _bits(lo, hi):
    """The f32 values whose words are lo .. hi-1."""
    return torch.arange(lo, hi, dtype=I32).view(F32).tolist()


def _is_view(obj, t, lo, shape, dtype):
    assert t.dtype == dtype and tuple(t.shape) == shape, (t.dtype, tuple(t.shape))
    assert t.is_contiguous() and t.storage_offset() == lo
    assert t.data_ptr() == obj.joint.data_ptr() + 4 * lo            # a view of the joint buffer, not a copy


def test_constrained_paths_layout():
    p = ConstrainedPaths(B, S, "cpu")
    assert p.slices == {"infeasible": (0, 1), "lens": (1, 4), "tags_flat": (4, 19), "scores": (19, 22)}
    assert p.joint.dtype == I32 and tuple(p.joint.shape) == (22,)
    assert (p.batch_size, p.capacity) == (3, 15)
    _is_view(p, p.infeasible, 0, (1,), I32)
    assert isinstance(p.tags, DeviceTags)
    _is_view(p, p.tags.lens, 1, (3,), I32)
    _is_view(p, p.tags.tags_flat, 4, (15,), I32)
    _is_view(p, p.scores, 19, (3,), F32)
    h = _fill(p)
    assert p.tags.lens.tolist() == [1, 2, 3] and p.tags.tags_flat.tolist() == list(range(4, 19))
    want = {"infeasible": 0, "lens": [1, 2, 3], "scores": _bits(19, 22), "paths": [[4], [5, 6], [7, 8, 9]]}
    assert p.unpack(h) == want and p.host() == want
    assert p.tolist() == [[4], [5, 6], [7, 8, 9]]
    assert repr(p) == "ConstrainedPaths(batch=3, capacity=15, device=cpu)"


def test_constrained_paths_reports_an_infeasible_sample_as_none():
    p = ConstrainedPaths(B, S, "cpu")
    p.joint.zero_()
    p.infeasible.fill_(1)
    p.tags.lens.copy_(torch.tensor([2, 1, 2], dtype=I32))
    p.tags.tags_flat[:5].copy_(torch.tensor([4, 5, -1, 7, 8], dtype=I32))
    p.scores.copy_(torch.tensor([1.5, float("-inf"), -2.0]))
    assert p.host() == {"infeasible": 1, "lens": [2, 1, 2], "scores": [1.5, float("-inf"), -2.0],
                        "paths": [[4, 5], None, [7, 8]]}


def test_crf_posterior_layout_with_entities():
    p = CrfPosterior(B, S, "cpu", True)
    assert p.slices == {"bad": (0, 1), "lens": (1, 4), "tags_flat": (4, 19), "n_ent": (19, 22), "ent": (22, 67),
                        "log_z": (67, 70), "seq_logp": (70, 73), "token_conf": (73, 88), "ent_conf": (88, 103)}
    assert list(p.slices) == ["bad", "lens", "tags_flat", "n_ent", "ent", "log_z", "seq_logp", "token_conf", "ent_conf"]
    assert p.joint.dtype == I32 and tuple(p.joint.shape) == (103,)
    assert (p.batch_size, p.capacity) == (3, 15) and p.marginals is None
    _is_view(p, p.bad, 0, (1,), I32)
    assert isinstance(p.tags, DeviceTags)
    _is_view(p, p.tags.lens, 1, (3,), I32)
    _is_view(p, p.tags.tags_flat, 4, (15,), I32)
    _is_view(p, p.n_ent, 19, (3,), I32)
    _is_view(p, p.ent, 22, (15, 3), I32)
    _is_view(p, p.log_z, 67, (3,), F32)
    _is_view(p, p.seq_logp, 70, (3,), F32)
    _is_view(p, p.token_conf, 73, (15,), F32)
    _is_view(p, p.ent_conf, 88, (15,), F32)
    h = _fill(p)
    assert p.ent[4].tolist() == [34, 35, 36]                        # row k of ent: words 22 + 3 k ..
    want = {"bad": 0, "lens": [1, 2, 3], "tags_flat": list(range(4, 19)), "n_ent": [19, 20, 21], "ent": list(range(22, 67)),
            "log_z": _bits(67, 70), "seq_logp": _bits(70, 73), "token_conf": _bits(73, 88), "ent_conf": _bits(88, 103)}
    assert p.unpack(h) == want and p.host() == want
    assert repr(p) == "CrfPosterior(batch=3, capacity=15, entities=True, device=cpu)"


def test_crf_posterior_layout_without_entities():
    p = CrfPosterior(B, S, "cpu", False)
    assert p.slices == {"bad": (0, 1), "lens": (1, 4), "tags_flat": (4, 19), "n_ent": (19, 19), "ent": (19, 19),
                        "log_z": (19, 22), "seq_logp": (22, 25), "token_conf": (25, 40), "ent_conf": (40, 40)}
    assert p.joint.dtype == I32 and tuple(p.joint.shape) == (40,)
    assert p.n_ent is None and p.ent is None and p.ent_conf is None and p.marginals is None
    _is_view(p, p.bad, 0, (1,), I32)
    _is_view(p, p.tags.lens, 1, (3,), I32)
    _is_view(p, p.tags.tags_flat, 4, (15,), I32)
    _is_view(p, p.log_z, 19, (3,), F32)
    _is_view(p, p.seq_logp, 22, (3,), F32)
    _is_view(p, p.token_conf, 25, (15,), F32)
    h = _fill(p)
    want = {"bad": 0, "lens": [1, 2, 3], "tags_flat": list(range(4, 19)), "n_ent": [], "ent": [],
            "log_z": _bits(19, 22), "seq_logp": _bits(22, 25), "token_conf": _bits(25, 40), "ent_conf": []}
    assert p.unpack(h) == want and p.host() == want
    assert repr(p) == "CrfPosterior(batch=3, capacity=15, entities=False, device=cpu)"


def test_crf_posterior_host_runs_the_deferred_check():
    p = CrfPosterior(B, S, "cpu", False)
    _fill(p)
    calls = []
    p.tags.deferred_check = lambda: calls.append(1)
    p.host()
    assert calls == [1]
    p.unpack(p.joint.cpu())                                         # unpack alone does not
    assert calls == [1]

    def refuse():
        raise RuntimeError("deferred")
    p.tags.deferred_check = refuse
    with pytest.raises(RuntimeError, match="deferred"):
        p.host()


def test_nbest_paths_layout():
    p = NBestPaths(B, S, NBEST, "cpu")
    assert p.slices == {"lens": (0, 3), "n_paths": (3, 6), "scores": (6, 12), "tags": (12, 42)}
    assert p.joint.dtype == I32 and tuple(p.joint.shape) == (42,)
    assert (p.batch_size, p.capacity, p.nbest) == (3, 15, 2)
    _is_view(p, p.lens, 0, (3,), I32)
    _is_view(p, p.n_paths, 3, (3,), I32)
    _is_view(p, p.scores, 6, (3, 2), F32)
    _is_view(p, p.tags, 12, (2, 15), I32)
    r1 = p.rank(1)
    assert isinstance(r1, DeviceTags)
    _is_view(p, r1.lens, 0, (3,), I32)
    _is_view(p, r1.tags_flat, 27, (15,), I32)
    with pytest.raises(IndexError):
        p.rank(2)
    h = _fill(p)
    s = _bits(6, 12)
    want = {"lens": [0, 1, 2], "n_paths": [3, 4, 5], "scores": [s[0:2], s[2:4], s[4:6]],
            "tags": [list(range(12, 27)), list(range(27, 42))]}
    assert p.unpack(h) == want and p.host() == want
    assert repr(p) == "NBestPaths(batch=3, nbest=2, capacity=15, device=cpu)"


def test_nbest_paths_tolist_and_log_probs():
    p = NBestPaths(B, S, NBEST, "cpu")
    p.joint.zero_()
    p.lens.copy_(torch.tensor([2, 1, 3], dtype=I32))
    p.n_paths.copy_(torch.tensor([2, 1, 2], dtype=I32))
    p.scores.copy_(torch.tensor([[3.0, 2.0], [1.0, float("-inf")], [0.5, 0.25]]))
    p.tags[0, :6].copy_(torch.tensor([1, 2, 0, 2, 1, 0], dtype=I32))
    p.tags[1, :6].copy_(torch.tensor([1, 1, -1, 2, 2, 0], dtype=I32))
    assert p.tolist() == [[([1, 2], 3.0), ([1, 1], 2.0)], [([0], 1.0)], [([2, 1, 0], 0.5), ([2, 2, 0], 0.25)]]
    lp = p.log_probs(torch.tensor([1.0, 2.0, 0.5]))
    assert lp.dtype == F32 and lp.tolist() == [[2.0, 1.0], [-1.0, float("-inf")], [0.0, -0.25]]
    with pytest.raises(ValueError, match="log_z"):
        p.log_probs(torch.zeros(4))
