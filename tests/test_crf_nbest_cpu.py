"""CPU: the float64 K-list Viterbi of tests/crf_nbest_oracle.py against enumeration of all paths (the tie rule included), its
rank 0 against the package's Viterbi, the export of icka_crf_nbest and the host-side checks of ``kernels.crf_nbest`` (no
device)."""
import ctypes

import pytest
import torch

import crf_nbest_oracle as NO

F32 = torch.float32


@pytest.mark.parametrize("grid", ["coarse", "fine"])
@pytest.mark.parametrize("C,L", [(1, 1), (1, 5), (2, 1), (3, 1), (2, 2), (2, 3), (3, 4), (4, 5), (3, 7), (5, 4), (13, 3)])
def test_viterbi_equals_enumeration(grid, C, L):
    B = 6
    e, st, en, tr = NO.GRIDS[grid](B, L, C, seed=C * 100 + L)
    for K in (1, 2, 3, 4, 7, 8):
        got = NO.nbest_batch(e, None, st, en, tr, K)
        ref = NO.nbest_batch(e, None, st, en, tr, K, fn=NO.brute)
        for b in range(B):
            assert len(got[b]) == min(K, C ** L), (K, b)                # K > C^L: the sample has C^L ranks
            assert got[b] == ref[b], (K, b, got[b], ref[b])              # scores bit for bit, paths in the pinned order
            assert len({tuple(p) for _, p in got[b]}) == len(got[b])
            x = NO.rows_of(e, None, b)
            for s, p in got[b]:
                assert s == NO.score(x, *(t.double().numpy() for t in (st, en, tr)), p)


def test_ties_are_present_on_the_coarse_grid():
    e, st, en, tr = NO.coarse(8, 5, 3, seed=1)
    rows = NO.nbest_batch(e, None, st, en, tr, 8)
    assert sum(a[0] == b[0] for r in rows for a, b in zip(r, r[1:])) >= 8


@pytest.mark.parametrize("kind", ["prefix", "holes"])
def test_masks_select_the_on_positions(kind):
    B, S, C, K = 5, 6, 3, 4
    e, st, en, tr = NO.coarse(B, S, C, seed=9)
    mask = NO.prefix_mask(B, S, 3) if kind == "prefix" else NO.holes_mask(B, S, 3)
    got = NO.nbest_batch(e, mask, st, en, tr, K)
    for b in range(B):
        L = 1 + int(mask[b, 1:].sum())
        assert all(len(p) == L for _, p in got[b]) and len(got[b]) == min(K, C ** L)
        assert got[b] == NO.brute(NO.rows_of(e, mask, b), *(t.double().numpy() for t in (st, en, tr)), K)


@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_rank_0_is_the_package_viterbi_on_prefix_masks(grid):
    from oracle import crf_oracle as O
    B, S, C = 6, 40, 5
    e, st, en, tr = NO.GRIDS[grid](B, S, C, seed=12)
    mask = NO.prefix_mask(B, S, 5)
    ref = O.crf_decode(e.double(), mask, st.double(), en.double(), tr.double())
    got = NO.nbest_batch(e, mask, st, en, tr, 4)
    assert [r[0][1] for r in got] == ref


def test_library_exports_the_entry():
    from icka_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "icka_crf_nbest") and "icka_crf_nbest" in _lib.PROTOTYPES


def _operands(B=2, S=4, C=3, K=2, cap=None):
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt)
    return dict(emissions=z(B, S, C), mask=z(B, S, dt=torch.int64), start=z(C), end=z(C), trans=z(C, C), nbest=K,
                lens=z(B, dt=torch.int32), n_paths=z(B, dt=torch.int32), scores=z(B, K),
                tags_flat=z(K, B * S if cap is None else cap, dt=torch.int32))


def _call(op):
    from icka_amd import kernels as K
    return K.crf_nbest(*(op[k] for k in ("emissions", "mask", "start", "end", "trans", "nbest", "lens", "n_paths", "scores",
                                         "tags_flat")))


def test_wrapper_reaches_the_device_check_with_good_operands():
    with pytest.raises(TypeError):            # well-formed operands reach the device check: there is no CPU path
        _call(_operands())
    with pytest.raises(TypeError):
        _call(dict(_operands(), mask=None))
    with pytest.raises(TypeError):            # S * C * K = 49152 exactly, and more room than needed
        _call(_operands(1, 512, 12, 8, cap=600))


@pytest.mark.parametrize("B,S,C,K,word", [(2, 4, 17, 2, "num_tags"), (2, 4, 3, 0, "nbest"), (2, 4, 3, 9, "nbest"),
                                          (1, 385, 16, 8, "49152"),        # 49280: one position over the limit
                                          (1, 512, 13, 8, "49152"), (1, 513, 3, 2, "S <="), (2049, 1, 3, 2, "B <=")])
def test_wrapper_names_the_limit_before_any_device_check(B, S, C, K, word):
    with pytest.raises(ValueError, match=word):
        _call(_operands(B, S, C, max(K, 1)) | {"nbest": K})


def test_wrapper_refuses_one_over_the_back_pointer_budget():
    """49153 has no factorisation inside the limits: the nearest shapes on both sides of 49152."""
    for S, C, K in ((384, 16, 8), (512, 12, 8), (512, 16, 6)):        # 49152: served
        with pytest.raises(TypeError):
            _call(_operands(1, S, C, K))
    for S, C, K in ((385, 16, 8), (439, 16, 7), (473, 13, 8)):        # 49280, 49168, 49192: the smallest excess per (C, K)
        with pytest.raises(ValueError, match="49152"):
            _call(_operands(1, S, C, K))


def test_wrapper_refuses_bad_operands_without_a_device():
    op = _operands()
    bad = {"emissions": op["emissions"].double(), "mask": op["mask"].int(), "start": torch.zeros(4), "end": torch.zeros(3).double(),
           "trans": torch.zeros(3, 4), "lens": torch.zeros(2, dtype=torch.int64), "n_paths": torch.zeros(3, dtype=torch.int32),
           "scores": torch.zeros(2, 2).double(), "tags_flat": torch.zeros(2, 8, dtype=torch.int64), "nbest": 2.0}
    for name, t in bad.items():
        with pytest.raises(ValueError):
            _call(dict(op, **{name: t}))
    with pytest.raises(ValueError):
        _call(dict(op, emissions=torch.zeros(2, 4, 6)[:, :, ::2]))                       # not contiguous
    with pytest.raises(ValueError):
        _call(dict(op, scores=torch.zeros(2, 3)))                                        # [B, K]
    with pytest.raises(ValueError, match="tags_flat"):
        _call(dict(op, tags_flat=torch.zeros(2, 7, dtype=torch.int32)))                  # short: capacity < B * S
    with pytest.raises(ValueError, match="tags_flat"):
        _call(dict(op, tags_flat=torch.zeros(1, 8, dtype=torch.int32)))                  # a row per rank
    with pytest.raises(ValueError, match="tags_flat"):
        _call(dict(op, tags_flat=torch.zeros(16, dtype=torch.int32)))
