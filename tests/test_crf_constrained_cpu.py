"""CPU: the float64 oracle of the constrained CRF against an enumeration of all paths, the allowed-set helpers, and the
argument validation of ``CRF.constrained_llh`` / ``constrained_decode`` and of the three launchers (which runs before the device
check, so it can be tested without a GPU)."""
import math
import re

import pytest
import torch

import crf_constrained_oracle as CO

F32 = torch.float32


def _same(a, b, tol=1e-11):
    if a == b:              # both -inf
        return True
    return abs(a - b) <= tol * max(1.0, abs(a), abs(b))


# ------------------------------------------------------------------------------------------- oracle against enumeration
@pytest.mark.parametrize("mask_kind", ["none", "prefix", "holes", "first_off"])
@pytest.mark.parametrize("allowed_kind", ["all", "single", "random", "partial", "one_empty"])
@pytest.mark.parametrize("grid", [None, "coarse"])
def test_oracle_against_enumeration(mask_kind, allowed_kind, grid):
    B, S, C = 4, 6, 3
    seed = 11 + len(mask_kind) * 7 + len(allowed_kind)
    e, st, en, tr = CO.inputs(B, S, C, seed, grid=grid)
    mask = CO.make_mask(mask_kind, B, S, seed + 1)
    allowed = CO.allowed_sets("random" if allowed_kind == "one_empty" else allowed_kind, B, S, C, seed + 2)
    if allowed_kind == "one_empty":
        allowed[2, 0] = 0           # position 0 is an on-position under every mask
        allowed[3, 1] = 8           # only a bit at C: ignored, so empty -- where position 1 is on
    samples = CO.batch(e, mask, allowed, st, en, tr)
    for b, s in enumerate(samples):
        ref = CO.enumerate_sample(e[b].double(), None if mask is None else mask[b], allowed[b], st.double(), en.double(),
                                  tr.double())
        assert s.feasible == ref["feasible"]
        if allowed_kind == "one_empty" and b == 2:
            assert not s.feasible
        assert _same(s.log_z, ref["log_z"]) and _same(s.log_za, ref["log_za"])
        assert s.llh <= 1e-12
        assert torch.allclose(s.marg, ref["marg"], atol=1e-12) and torch.allclose(s.pair, ref["pair"], atol=1e-12)
        assert torch.allclose(s.marg_a, ref["marg_a"], atol=1e-12) and torch.allclose(s.pair_a, ref["pair_a"], atol=1e-12)
        if not s.feasible:
            assert s.llh == -math.inf and not bool(s.d_e.any())
        elif allowed_kind == "all":
            assert abs(s.llh) < 1e-12 and float(s.d_e.abs().max()) < 1e-12
        path, score = s.viterbi()
        if grid is not None:        # exact sums: the tie rule decides, and the enumeration knows it
            assert (path, score) == ref["best"], (b, path, score, ref["best"])
        else:
            assert path == ref["best"][0] and _same(score, ref["best"][1])
        if s.feasible:
            assert all(path[i] in s.sets[i] for i in range(s.L)) and _same(s.score(path), score)
            assert len(path) == s.L == 1 + (S - 1 if mask is None else int(mask[b, 1:].sum()))


def test_tie_rule_on_a_flat_model():
    """all scores zero: every path ties, and the rule picks the smallest allowed tag at every position"""
    S, C = 5, 3
    z = torch.zeros
    allowed = torch.tensor([[0b110, 0b111, 0b100, 0b101, 0b010]])
    s = CO.batch(z(1, S, C), None, allowed, z(C), z(C), z(C, C))[0]
    assert s.viterbi() == ([1, 0, 2, 0, 1], 0.0)
    assert CO.enumerate_sample(z(S, C), None, allowed[0], z(C), z(C), z(C, C))["best"] == ([1, 0, 2, 0, 1], 0.0)
    assert _same(s.llh, math.log(2 * 3 * 1 * 2 * 1) - S * math.log(3))


# ------------------------------------------------------------------------------------------------- allowed-set helpers
def test_allowed_from_tags():
    from icka_amd.crf import CRF
    tags = torch.tensor([[0, 2, -1, 4], [-1, -1, 1, 3]])
    a = CRF.allowed_from_tags(tags, 5)
    assert a.dtype == torch.int64 and a.tolist() == [[1, 4, 31, 16], [31, 31, 2, 8]]
    a = CRF.allowed_from_tags(tags.to(torch.int32), 5, unknown_index=4)
    assert a.tolist() == [[1, 4, 0, 31], [0, 0, 2, 8]]       # -1 now names no tag: nothing is allowed there
    a = CRF.allowed_from_tags(torch.tensor([63, 0, -1, 62]), 64)
    assert a.tolist() == [-(1 << 63), 1, -1, 1 << 62]
    assert CO.tag_set(a[0], 64) == [63] and CO.tag_set(a[2], 64) == list(range(64))
    with pytest.raises(ValueError):
        CRF.allowed_from_tags(tags, 65)
    with pytest.raises(ValueError):
        CRF.allowed_from_tags(tags.float(), 5)


@pytest.mark.parametrize("C", [1, 3, 13, 63, 64])
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_pack_allowed(C, dtype):
    from icka_amd.crf import CRF
    g = torch.Generator().manual_seed(C)
    bits = torch.rand(3, 7, C, generator=g) < 0.5
    bits[0, 0] = True
    bits[0, 1] = False
    bits[0, 2] = False
    bits[0, 2, C - 1] = True
    packed = CRF.pack_allowed(bits.to(torch.uint8) * 3 if dtype == torch.uint8 else bits)
    assert packed.dtype == torch.int64 and tuple(packed.shape) == (3, 7)
    for b in range(3):
        for t in range(7):
            assert CO.tag_set(packed[b, t], C) == [j for j in range(C) if bits[b, t, j]]
    assert int(packed[0, 0]) == CO.every(C) and int(packed[0, 1]) == 0
    if C == 64:
        assert int(packed[0, 2]) == -(1 << 63)
    with pytest.raises(ValueError):
        CRF.pack_allowed(torch.zeros(2, 3, 65, dtype=torch.bool))
    with pytest.raises(ValueError):
        CRF.pack_allowed(torch.zeros(2, 3, 4))


# ------------------------------------------------------------------------------------------------------- validation
def test_module_validation_runs_before_the_device_check():
    from icka_amd import ConstrainedPaths   # noqa: F401  (exported)
    from icka_amd.crf import CRF
    B, S, C = 2, 5, 4
    crf = CRF(C, batch_first=True)
    e = torch.zeros(B, S, C)
    ok = torch.full((B, S), 15, dtype=torch.int64)
    for fn in (crf.constrained_llh, crf.constrained_decode):
        with pytest.raises(ValueError, match="allowed"):
            fn(e, ok[0])                                                   # rank
        with pytest.raises(ValueError, match="allowed"):
            fn(e, ok[:, :4])                                               # shape
        with pytest.raises(ValueError, match="allowed"):
            fn(e, ok.to(torch.int32))                                      # dtype
        with pytest.raises(ValueError, match="allowed"):
            fn(e, torch.ones(B, S, C + 1, dtype=torch.bool))               # bool layout of another tag count
        with pytest.raises(ValueError, match="allowed"):
            fn(e, [[15] * S] * B)
        with pytest.raises(TypeError, match="no CPU path"):
            fn(e, ok)
        with pytest.raises(TypeError, match="no CPU path"):
            fn(e, torch.ones(B, S, C, dtype=torch.bool), mask=torch.ones(B, S))
    with pytest.raises(ValueError, match="reduction"):
        crf.constrained_llh(e, ok, reduction="avg")
    with pytest.raises(ValueError, match="12288"):
        crf.constrained_llh(torch.zeros(1, 3073, C), torch.zeros(1, 3073, dtype=torch.int64))
    with pytest.raises(ValueError, match="12288"):
        CRF(C).constrained_decode(torch.zeros(3073, 1, C), torch.zeros(3073, 1, dtype=torch.int64))     # sequence-first


def _operands(B, S, C):
    f = lambda *s: torch.zeros(*s, dtype=F32)
    return dict(e=f(B, S, C), al=torch.zeros(B, S, dtype=torch.int64), st=f(C), en=f(C), tr=f(C, C))


def test_launcher_validation_runs_before_the_device_check():
    from icka_amd import kernels as K
    f = lambda *s: torch.zeros(*s, dtype=F32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)

    def llh(B, S, C, **kw):
        o = _operands(B, S, C); o.update(kw)
        K.crf_constrained_llh(o["e"], o.get("mask"), o["al"], o["st"], o["en"], o["tr"], o.get("llh", f(B)), f(B), f(B),
                              o.get("inf"))

    def grad(B, S, C, **kw):
        o = _operands(B, S, C); o.update(kw)
        K.crf_constrained_grad(o["e"], o.get("mask"), o["al"], o["st"], o["en"], o["tr"], f(B), o.get("de", f(B, S, C)), f(C),
                               f(C), o.get("dtr", f(C, C)))

    def dec(B, S, C, **kw):
        o = _operands(B, S, C); o.update(kw)
        K.crf_constrained_decode(o["e"], o.get("mask"), o["al"], o["st"], o["en"], o["tr"], i32(B), o.get("flat", i32(B * S)),
                                 f(B), o.get("inf"))

    for fn in (llh, grad, dec):
        with pytest.raises(ValueError, match="64"):
            fn(1, 2, 65)
        with pytest.raises(ValueError, match="12288"):
            fn(1, 193, 64)                                     # S * C = 12352
        with pytest.raises(ValueError, match="allowed"):
            fn(2, 3, 4, al=torch.zeros(2, 3, dtype=torch.int32))
        with pytest.raises(ValueError, match="allowed"):
            fn(2, 3, 4, al=torch.zeros(2, 4, dtype=torch.int64))
        with pytest.raises(ValueError, match="allowed"):
            fn(2, 3, 4, al=torch.zeros(3, 2, dtype=torch.int64).t())       # not contiguous
        with pytest.raises(ValueError, match="mask"):
            fn(2, 3, 4, mask=torch.zeros(2, 3, dtype=torch.bool))
        with pytest.raises(ValueError, match="emissions"):
            fn(2, 3, 4, e=torch.zeros(2, 3, 4, dtype=torch.float64))
        with pytest.raises(TypeError, match="no CPU path"):
            fn(2, 3, 4)
        with pytest.raises(TypeError, match="no CPU path"):
            fn(2, 3, 4, mask=torch.ones(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="2048"):
        dec(2049, 1, 2)
    with pytest.raises(TypeError, match="no CPU path"):
        llh(2049, 1, 2)                                        # only the decode entry sums offsets
    with pytest.raises(ValueError, match="tags_flat"):
        dec(2, 3, 4, flat=i32(5))
    with pytest.raises(ValueError, match="infeasible"):
        dec(2, 3, 4, inf=i32(2))
    with pytest.raises(ValueError, match="llh"):
        llh(2, 3, 4, llh=f(3))
    with pytest.raises(ValueError, match="d_emissions"):
        grad(2, 3, 4, de=f(2, 3, 5))


def test_the_three_entries_are_declared():
    import os
    from icka_amd import _lib
    names = ["icka_crf_constrained_llh", "icka_crf_constrained_grad", "icka_crf_constrained_decode"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icka_hip.h")).read()
    for n in names:
        assert n in _lib.PROTOTYPES
        assert re.search(r"\bint %s\(" % n, header)
    n_args = {n: len(_lib.PROTOTYPES[n][1]) for n in names}
    assert n_args == {names[0]: 15, names[1]: 17, names[2]: 16}
