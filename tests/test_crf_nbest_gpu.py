"""GPU: icka_crf_nbest, CRF.decode_nbest / NBestPaths and EntityDecoder.nbest against the float64 K-list Viterbi of
tests/crf_nbest_oracle.py.

On the two grids of that module every partial sum of a score is exact in f32, so paths (the pinned tie order included),
scores (bit for bit), n_paths and lens are compared for EQUALITY.  On ordinary inputs neighbouring ranks lie within f32
roundoff of each other often enough that f32 may order them differently (11 % to 15 % of neighbours at S = 128 to 200 are
within 1e-3), so there the tests check what every valid answer satisfies, at the project's bar for log_z and seq_logp: rtol
2e-5, atol 2e-4 (tests/test_crf_gpu.py:37)."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import crf_nbest_oracle as NO
import crf_posterior_oracle as PO
import kernel_check as kc

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
RTOL, ATOL = 2e-5, 2e-4
MARG_BAR, ENT_CONF_BAR = 1e-3, 1.9e-4        # tests/test_crf_posterior_gpu.py
SHAPES = [(4, 1, 3, 8),        # L = 1: n_paths = 3
          (3, 2, 2, 8),        # 4 paths for 8 ranks
          (5, 7, 3, 4),        # also against enumeration
          (3, 65, 5, 1),       # one position past a mask word
          (6, 33, 13, 8),
          (4, 128, 16, 8),
          (2, 512, 13, 7)]     # 46592 of the 49152 back-pointer bytes
MASKED = [(5, 7, 3, 4), (6, 33, 13, 8)]      # the shapes that also run without a mask, with holes and sequence-first


def _close(a, b):
    return abs(a - b) <= ATOL + RTOL * abs(b)


@functools.lru_cache(maxsize=None)
def _case(grid, B, S, C, K, kind):
    """(e, mask, start, end, trans, reference) -- computed once, shared, never modified."""
    e, st, en, tr = NO.GRIDS[grid](B, S, C, seed=B * 1000 + S * 10 + C)
    mask = {"prefix": lambda: NO.prefix_mask(B, S, S + C), "holes": lambda: NO.holes_mask(B, S, S + C), "none": lambda: None}[kind]()
    return e, mask, st, en, tr, NO.nbest_batch(e, mask, st, en, tr, K)


def _crf(C, params=None, seed=0, batch_first=True):
    from icka_amd.crf import CRF
    torch.manual_seed(seed)
    crf = CRF(C, batch_first=batch_first).cuda()
    if params is not None:
        with torch.no_grad():
            for p, v in zip((crf.start_transitions, crf.end_transitions, crf.transitions), params):
                p.copy_(v)
    return crf


def _params(crf):
    return [p.detach().cpu() for p in (crf.start_transitions, crf.end_transitions, crf.transitions)]


def _assert_equals_reference(h, ref, K, what):
    """host() of an NBestPaths against the oracle rows: everything equal, scores bit for bit, -inf / -1 at the missing ranks."""
    off = 0
    for b, rows in enumerate(ref):
        L = len(rows[0][1])
        assert h["lens"][b] == L and h["n_paths"][b] == len(rows), (what, b, h["lens"][b], h["n_paths"][b], L, len(rows))
        want = torch.tensor([s for s, _ in rows] + [-math.inf] * (K - len(rows)), dtype=torch.float64).to(F32)
        got = torch.tensor(h["scores"][b], dtype=F32)
        assert torch.equal(got.view(I32), want.view(I32)), (what, b, got, want)
        for r in range(K):
            path = rows[r][1] if r < len(rows) else [-1] * L
            assert h["tags"][r][off:off + L] == path, (what, b, r)
        off += L


def _guarded_launch(e, mask, st, en, tr, K, spare=5):
    """icka_crf_nbest into over-allocated, sentinel-filled buffers (tags_flat with ``spare`` more columns than B * S) -> the
    dict of NBestPaths.host(); asserts that nothing outside [:B], [:B, :K] and [r, :sum(lens)] changed."""
    from icka_amd import kernels as Kn
    B, S, _ = e.shape
    cap = B * S + spare
    (lens, c1), (npth, c2) = kc.guarded(1, B, I32), kc.guarded(1, B, I32)
    scores, c3 = kc.guarded(B, K, F32)
    tags, c4 = kc.guarded(K, cap, I32)
    m = None if mask is None else mask.long().cuda()
    Kn.crf_nbest(e.cuda(), m, st.cuda(), en.cuda(), tr.cuda(), K, lens[0], npth[0], scores, tags)
    torch.cuda.synchronize()
    for chk in (c1, c2, c3, c4):
        chk()
    total = int(lens[0].sum())
    assert bool((tags[:, total:] == kc.SENTINEL[I32]).all()), "entries past sum(lens) were written"
    assert bool((tags[:, :total] != kc.SENTINEL[I32]).all()) and not bool(torch.isnan(scores).any())
    return {"lens": lens[0].tolist(), "n_paths": npth[0].tolist(), "scores": scores.tolist(), "tags": tags.tolist()}


@pytest.mark.parametrize("grid", ["coarse", "fine"])
@pytest.mark.parametrize("B,S,C,K", SHAPES)
def test_exact_on_prefix_masks_with_guard_bands(grid, B, S, C, K):
    e, mask, st, en, tr, ref = _case(grid, B, S, C, K, "prefix")
    lens = mask.sum(1).tolist()
    assert lens[0] == S and (B == 1 or lens[1] == 1)
    h = _guarded_launch(e, mask, st, en, tr, K)
    _assert_equals_reference(h, ref, K, "%s %s" % (grid, (B, S, C, K)))
    if (B, S, C, K) == (5, 7, 3, 4):
        assert ref == NO.nbest_batch(e, mask, st, en, tr, K, fn=NO.brute)
    # the public interface gives the same, and its rank 0 is decode's path
    crf = _crf(C, (st, en, tr))
    out = crf.decode_nbest(e.cuda(), mask.cuda(), nbest=K)
    hp = out.host()
    total = sum(lens)
    assert hp["lens"] == h["lens"] and hp["n_paths"] == h["n_paths"] and hp["scores"] == h["scores"]
    assert [row[:total] for row in hp["tags"]] == [row[:total] for row in h["tags"]]
    assert out.rank(0).tolist() == crf.decode(e.cuda(), mask=mask.cuda())
    assert out.tolist() == [[(p, float(np.float32(s))) for s, p in rows] for rows in ref]


@pytest.mark.parametrize("grid", ["coarse", "fine"])
@pytest.mark.parametrize("kind", ["none", "holes", "sequence_first"])
@pytest.mark.parametrize("B,S,C,K", MASKED)
def test_exact_without_mask_with_holes_and_sequence_first(grid, kind, B, S, C, K):
    e, mask, st, en, tr, ref = _case(grid, B, S, C, K, "prefix" if kind == "sequence_first" else kind)
    if kind == "holes":
        assert [len(r[0][1]) for r in ref] == [1 + int(mask[b, 1:].sum()) for b in range(B)] and len(ref[B - 1][0][1]) == 1
    if kind == "sequence_first":
        crf = _crf(C, (st, en, tr), batch_first=False)
        out = crf.decode_nbest(e.transpose(0, 1).cuda(), mask.transpose(0, 1).cuda(), nbest=K)
    else:
        _assert_equals_reference(_guarded_launch(e, mask, st, en, tr, K), ref, K, "%s %s guarded" % (grid, kind))
        out = _crf(C, (st, en, tr)).decode_nbest(e.cuda(), None if mask is None else mask.cuda(), nbest=K)
    _assert_equals_reference(out.host(), ref, K, "%s %s %s" % (grid, kind, (B, S, C, K)))


@functools.lru_cache(maxsize=None)
def _ordinary(B, S, C, K):
    g = torch.Generator().manual_seed(S + C)
    e = torch.randn(B, S, C, generator=g) * 2.0
    mask = NO.prefix_mask(B, S, C)
    crf = _crf(C, seed=S)
    return e, mask, crf, NO.nbest_batch(e, mask, *_params(crf), K)


@pytest.mark.parametrize("B,S,C,K", [(8, 128, 13, 8), (8, 40, 15, 4)])
def test_ordinary_inputs(B, S, C, K):
    e, mask, crf, ref = _ordinary(B, S, C, K)
    st, en, tr = (p.double().numpy() for p in _params(crf))
    out = crf.decode_nbest(e.cuda(), mask.cuda(), nbest=K)
    h = out.host()
    got = out.paths_of(h)
    worst = 0.0
    for b in range(B):
        L = int(mask[b].sum())
        x = NO.rows_of(e, mask, b)
        assert h["lens"][b] == L and h["n_paths"][b] == min(K, C ** L) == len(ref[b]) == len(got[b])
        assert len({tuple(p) for p, _ in got[b]}) == len(got[b]), b                       # pairwise distinct
        for r, (p, s) in enumerate(got[b]):
            assert len(p) == L and all(0 <= y < C for y in p), (b, r)
            exact = NO.score(x, st, en, tr, p)
            worst = max(worst, abs(s - exact), abs(s - ref[b][r][0]))
            assert _close(s, exact), (b, r, s, exact)                                     # the reported score is the path's
            assert _close(s, ref[b][r][0]), (b, r, s, ref[b][r][0])                       # and the r-th best score
            assert r == 0 or s <= got[b][r - 1][1], (b, r)                                # non-increasing
    print("NBEST ordinary %s worst |score error| %.3e" % ((B, S, C, K), worst))


@pytest.mark.parametrize("B,S,C,K", [(8, 128, 13, 8), (8, 40, 15, 4)])
def test_ranks_compose_with_the_posterior(B, S, C, K):
    e, mask, crf, _ = _ordinary(B, S, C, K)
    out = crf.decode_nbest(e.cuda(), mask.cuda(), nbest=K)
    assert int(out.n_paths.min()) == K                     # C >= K: every sample has every rank
    posts = [crf.posterior(e.cuda(), out.rank(r), mask.cuda()) for r in range(K)]
    lp = out.log_probs(posts[0].log_z).cpu()
    for r, post in enumerate(posts):
        assert int(post.bad.item()) == 0
        assert torch.allclose(post.seq_logp.cpu(), lp[:, r], rtol=RTOL, atol=ATOL), (r, post.seq_logp, lp[:, r])
        assert post.tags.tolist() == out.rank(r).tolist()
    assert float(lp.exp().sum(1).max()) <= 1 + 1e-4


def test_all_paths_of_a_short_sample_sum_to_one():
    B, S, C, K = 5, 7, 3, 8
    g = torch.Generator().manual_seed(3)
    e = torch.randn(B, S, C, generator=g) * 2.0
    mask = NO.prefix_mask(B, S, 1)
    crf = _crf(C, seed=2)
    out = crf.decode_nbest(e.cuda(), mask.cuda(), nbest=K)
    lp = out.log_probs(crf.posterior(e.cuda(), None, mask.cuda()).log_z).cpu()
    n = out.n_paths.tolist()
    small = [b for b in range(B) if C ** int(mask[b].sum()) <= K]
    assert 1 in small and n[1] == 3
    for b in small:
        assert abs(float(lp[b, :n[b]].exp().sum()) - 1) < 1e-4, b
        assert bool(torch.isinf(lp[b, n[b]:]).all())
    assert float(lp.exp().sum(1).max()) <= 1 + 1e-4


NAMES = ["O", "B-PER", "I-PER", "B-LOC", "I-LOC"]


def test_entity_decoder_nbest():
    """5 labels, L <= 6: everything is enumerated.  Emissions and parameters on the fine grid, so the paths are the oracle's."""
    from icka_amd import EntityDecoder, metrics
    B, S, C, K = 5, 6, 5, 8
    e, st, en, tr = NO.fine(B, S, C, seed=77)
    mask = torch.arange(S)[None, :] < torch.tensor([6, 1, 3, 5, 2])[:, None]
    crf = _crf(C, (st, en, tr))
    ref = NO.nbest_batch(e, mask, st, en, tr, K)
    assert len(ref[1]) == 5 and all(len(r) == K for b, r in enumerate(ref) if b != 1)       # one sample lacks ranks
    ents = EntityDecoder(crf, NAMES).nbest(e.cuda(), mask=mask.cuda(), nbest=K)
    got = ents.tolist()
    assert all(int(p.bad.item()) == 0 for p in ents.posteriors)
    assert ents.paths.tolist() == [[(p, float(np.float32(s))) for s, p in rows] for rows in ref]
    P = [t.double().numpy() for t in (st, en, tr)]
    n_ent = n_multi = 0
    for b in range(B):
        x = NO.rows_of(e, mask, b)
        L = x.shape[0]
        allp = np.array(list(itertools.product(range(C), repeat=L)))
        sc = np.array([NO.score(x, *P, list(p)) for p in allp])
        prob = np.exp(sc - sc.max())
        prob /= prob.sum()
        prob_of = {tuple(p): float(q) for p, q in zip(allp, prob)}
        want, spellings = {}, {}
        for r, (_, path) in enumerate(ref[b]):
            for ty, s, t in metrics.chunks(path, NAMES):
                want.setdefault((ty, s, t), []).append(r)
                spellings.setdefault((ty, s, t), set()).add(tuple(path[s:t]))
        assert sorted((g[0], g[1], g[2], g[4]) for g in got[b]) == sorted(k + (tuple(v),) for k, v in want.items()), b
        for ty, s, t, conf, ranks in got[b]:
            # ranks may spell one entity with different tags (B-PER I-PER / I-PER I-PER at the start of a path): the events
            # exclude each other, the confidence is the sum of their span posteriors, each held to the existing bar
            spans = spellings[(ty, s, t)]
            exact = sum(float(prob[(allp[:, s:t] == np.array(span)).all(1)].sum()) for span in spans)
            assert abs(conf - exact) < len(spans) * (MARG_BAR if t - s == 1 else ENT_CONF_BAR), (b, ty, s, t, conf, exact)
            assert conf >= sum(prob_of[tuple(ref[b][r][1])] for r in ranks) - 1e-4, (b, ty, s, t)
            n_ent += 1
            n_multi += len(spans) > 1
        assert got[b] == sorted(got[b], key=lambda g: (-g[3], g[1], g[2], g[0])), b
    print("NBEST entities: %d, of them %d spelled in more than one way" % (n_ent, n_multi))
    assert n_ent > 20


def test_decode_nbest_is_capturable():
    B, S, C, K = 4, 33, 13, 8
    cases = [_case("fine", B, S, C, K, "prefix")] + [NO.fine(B, S, C, seed=500 + i) for i in range(2)]
    st, en, tr = cases[0][2:5]
    crf = _crf(C, (st, en, tr))
    static_em, static_mask = cases[0][0].cuda(), cases[0][1].cuda().long()
    crf.decode_nbest(static_em, static_mask, nbest=K)       # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # one stream, no side branches
        out = crf.decode_nbest(static_em, static_mask, nbest=K)
    for i, (e2, _, _, _) in enumerate(cases[1:]):
        mask2 = NO.prefix_mask(B, S, 40 + i)
        static_em.copy_(e2.cuda()); static_mask.copy_(mask2.cuda().long())
        graph.replay()
        torch.cuda.synchronize()
        h = out.host()
        he = crf.decode_nbest(e2.cuda(), mask2.cuda(), nbest=K).host()
        n = sum(h["lens"])
        assert h["lens"] == mask2.sum(1).tolist() == he["lens"] and h["n_paths"] == he["n_paths"] and h["scores"] == he["scores"]
        assert [row[:n] for row in h["tags"]] == [row[:n] for row in he["tags"]]
        _assert_equals_reference(h, NO.nbest_batch(e2, mask2, st, en, tr, K), K, "replay %d" % i)


@pytest.mark.parametrize("B,S,C,K,word", [(2, 4, 17, 2, "num_tags"), (2, 4, 3, 9, "nbest"), (2, 4, 3, 0, "nbest"),
                                          (1, 385, 16, 8, "49152"), (1, 512, 13, 8, "49152")])
def test_refusals_name_the_limit(B, S, C, K, word):
    crf = _crf(C)
    with pytest.raises(ValueError, match=word):
        crf.decode_nbest(torch.zeros(B, S, C, device="cuda"), nbest=K)
