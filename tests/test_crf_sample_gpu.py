"""GPU: icka_crf_sample and CRF.sample / SampledPaths against the checker of tests/crf_sample_check.py (every step conditioned
on the kernel's own next tag; tolerances derived there, borderline share capped at 5 % per case), with guard bands around every
output and the operand, determinism in the seed, a captured graph that draws fresh paths per replay, and the draws going into
icka_crf_posterior and icka_chunk_eval unchanged."""
import numpy as np
import pytest
import torch

import crf_check as CC
import crf_sample_check as SC
import kernel_check as kc

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
E_SHAPE = -1


def _words(seed_dev):
    return None if seed_dev is None else torch.from_numpy(np.array(seed_dev, dtype=np.uint32).view(np.int32)).cuda()


def _launch(inp, K, seed, seed_dev=None, pad=0, spare=5, expect=0):
    """icka_crf_sample itself into sentinel-filled, over-allocated buffers, the emissions with row stride C + pad inside NaN
    bands -> the dict the checker takes; asserts that nothing outside the documented outputs changed."""
    from icka_amd import _lib
    B, S, C = inp["e"].shape
    cap = B * S + spare
    eg = kc.Guarded(B * S, C, F32, ld=C + pad, fill=kc.NAN_FILL[F32], init=inp["e"].reshape(B * S, C).cuda())
    (lens, c1), (logz, c2) = kc.guarded(1, B, I32), kc.guarded(1, B, F32)
    scores, c3 = kc.guarded(B, K, F32)
    tags, c4 = kc.guarded(K, cap, I32)
    m = None if inp["mask"] is None else inp["mask"].long().cuda()
    st, en, tr = (inp[k].cuda().contiguous() for k in ("start", "end", "trans"))
    sd = _words(seed_dev)
    rc = _lib.load().icka_crf_sample(eg.view.data_ptr(), C + pad, None if m is None else m.data_ptr(), st.data_ptr(),
                                     en.data_ptr(), tr.data_ptr(), K, seed, None if sd is None else sd.data_ptr(),
                                     lens.data_ptr(), logz.data_ptr(), scores.data_ptr(), tags.data_ptr(), cap, B, S, C,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, rc
    for chk in (c1, c2, c3, c4):
        chk()
    eg.check(what="emissions")
    if expect != 0:        # refused: nothing written
        assert bool((lens == kc.SENTINEL[I32]).all()) and bool((tags == kc.SENTINEL[I32]).all())
        assert bool(torch.isnan(logz).all()) and bool(torch.isnan(scores).all())
        return None
    total = int(lens[0].sum())
    assert bool((tags[:, total:] == kc.SENTINEL[I32]).all()), "entries past sum(lens) were written"
    assert bool((tags[:, :total] != kc.SENTINEL[I32]).all()) and not bool(torch.isnan(scores).any())
    return {"lens": lens[0].tolist(), "log_z": logz[0].tolist(), "scores": scores.tolist(), "tags": tags.tolist()}


def _crf(inp, batch_first=True):
    from icka_amd.crf import CRF
    crf = CRF(inp["e"].shape[2], batch_first=batch_first).cuda()
    with torch.no_grad():
        for p, k in zip((crf.start_transitions, crf.end_transitions, crf.transitions), ("start", "end", "trans")):
            p.copy_(inp[k])
    return crf


def _mask(inp):
    return None if inp["mask"] is None else inp["mask"].cuda()


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_draws_match_their_uniforms_with_guard_bands(case):
    inp, K, pad = SC.make_case(case), case[4], case[7]
    out = _launch(inp, K, SC.SEED, pad=pad)
    assert SC.check(inp, out, K, SC.SEED, verbose=case[0]) <= SC.CAP
    # the public interface gives the same bits
    sp = _crf(inp).sample(inp["e"].cuda(), _mask(inp), num_samples=K, seed=SC.SEED)
    h = sp.host()
    n = sum(h["lens"])
    assert h["lens"] == out["lens"] and h["log_z"] == out["log_z"] and h["scores"] == out["scores"]
    assert [row[:n] for row in h["tags"]] == [row[:n] for row in out["tags"]]
    lp = sp.log_probs().cpu()
    assert torch.equal(lp, torch.tensor(h["scores"]) - torch.tensor(h["log_z"])[:, None])
    lst = sp.tolist()
    assert len(lst) == inp["e"].shape[0] and all(len(r) == K for r in lst)
    assert lst[0][K - 1][0] == SC.split_rows(h["lens"], h["tags"])[K - 1][0]
    assert lst[0][0][1] == h["scores"][0][0] - h["log_z"][0]


def test_size_limit_accepted_and_refused_with_nothing_written():
    g = torch.Generator().manual_seed(1)
    mk = lambda S: {"e": torch.randn(1, S, 1, generator=g), "mask": None, "start": torch.zeros(1), "end": torch.zeros(1),
                    "trans": torch.zeros(1, 1)}
    out = _launch(mk(12288), 2, 5)                    # S * C = 12288: the one path of a one-tag chain
    assert out["lens"] == [12288] and all(t == 0 for row in out["tags"] for t in row[:12288])
    _launch(mk(12289), 2, 5, expect=E_SHAPE)
    _launch(SC.make_case(SC.CASES[2]), 65, 5, expect=E_SHAPE)             # K = 65
    crf = _crf(mk(2))
    with pytest.raises(ValueError, match="12288"):
        crf.sample(torch.zeros(1, 12289, 1, device="cuda"))
    for K, word in ((0, "num_samples"), (65, "num_samples"), (True, "num_samples"), (2.0, "num_samples")):
        with pytest.raises(ValueError, match=word):
            crf.sample(torch.zeros(1, 4, 1, device="cuda"), num_samples=K)
    with pytest.raises(ValueError, match="seed"):
        crf.sample(torch.zeros(1, 4, 1, device="cuda"), seed=-1)
    with pytest.raises(ValueError, match="seed"):
        crf.sample(torch.zeros(1, 4, 1, device="cuda"), seed=torch.zeros(1, dtype=torch.int64))      # a host tensor


def test_forbidden_transitions_are_never_drawn():
    inp, K = SC.bio_case(), 64
    B, S, C = inp["e"].shape
    sp = _crf(inp).sample(inp["e"].cuda(), _mask(inp), num_samples=K, seed=77)
    h = sp.host()
    assert SC.check(inp, h, K, 77, verbose="bio") <= SC.CAP
    n = 0
    for row in SC.split_rows(h["lens"], h["tags"]):
        for y in row:
            assert not SC.bio_illegal(None, y[0]), y
            assert not any(SC.bio_illegal(a, b) for a, b in zip(y, y[1:])), y
            n += len(y)
    assert n == K * sum(h["lens"]) and len(h["lens"]) == 8


def test_same_seed_same_bits_other_seeds_other_paths():
    case = SC.CASES[2]
    inp, K = SC.make_case(case), case[4]
    crf = _crf(inp)
    e, m = inp["e"].cuda(), _mask(inp)
    a, b = crf.sample(e, m, K, seed=SC.SEED), crf.sample(e, m, K, seed=SC.SEED)
    n = int(a.lens.sum())
    assert torch.equal(a.joint[:a.slices["tags"][0]], b.joint[:b.slices["tags"][0]]) and torch.equal(a.tags[:, :n], b.tags[:, :n])
    other = crf.sample(e, m, K, seed=SC.SEED + 1)
    assert not torch.equal(other.tags[:, :n], a.tags[:, :n])
    assert SC.check(inp, other.host(), K, SC.SEED + 1) <= SC.CAP
    words = (0x8000_0003, 0x11)
    dev = _launch(inp, K, SC.SEED, seed_dev=words)
    assert [r[:n] for r in dev["tags"]] != [r[:n] for r in a.host()["tags"]]
    assert SC.check(inp, dev, K, SC.SEED, words) <= SC.CAP
    # a device tensor alone is a by-value seed of 0
    value = (words[1] << 32) | words[0]
    t = torch.from_numpy(np.array([value], dtype=np.uint64).view(np.int64)).cuda()
    assert SC.check(inp, crf.sample(e, m, K, seed=t).host(), K, 0, words) <= SC.CAP


def test_sequence_first_layout():
    case = SC.CASES[3]
    inp, K = SC.make_case(case), case[4]
    sp = _crf(inp, batch_first=False).sample(inp["e"].transpose(0, 1).cuda(), inp["mask"].transpose(0, 1).cuda(), K, seed=3)
    assert SC.check(inp, sp.host(), K, 3) <= SC.CAP


def test_captured_graph_draws_fresh_paths_per_replay():
    case = SC.CASES[2]
    inp, K = SC.make_case(case), case[4]
    crf = _crf(inp)
    e, m = inp["e"].cuda(), _mask(inp)
    seed = torch.tensor([41], dtype=torch.int64, device="cuda")
    crf.sample(e, m, K, seed=seed)                          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no side branches
        seed.add_(1)
        out = crf.sample(e, m, K, seed=seed)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        v = int(seed.item())
        h = out.host()
        assert SC.check(inp, h, K, 0, (v & SC.M32, v >> 32)) <= SC.CAP
        seen.append((v, h["tags"]))
    assert seen[0][0] + 1 == seen[1][0] and seen[0][1] != seen[1][1]


NAMES = SC.BIO_NAMES


def test_draws_go_into_posterior_and_chunk_eval_unchanged():
    from icka_amd import metrics as M
    B, S, C, K = 3, 6, len(NAMES), 5
    g = torch.Generator().manual_seed(21)
    inp = {"e": torch.randn(B, S, C, generator=g) * 2.0, "mask": CC.make_masks(B, S, "prefix", g),
           "start": torch.randn(C, generator=g) * 0.5, "end": torch.randn(C, generator=g) * 0.5,
           "trans": torch.randn(C, C, generator=g) * 0.7}
    crf = _crf(inp)
    e, m = inp["e"].cuda(), inp["mask"].cuda()
    sp = crf.sample(e, m, K, seed=9)
    h = sp.host()
    assert SC.check(inp, h, K, 9) <= SC.CAP
    lp = sp.log_probs().cpu().double()
    paths = SC.split_rows(h["lens"], h["tags"])
    labels = torch.randint(0, C, (B, S), generator=g)
    for k in range(K):
        post = crf.posterior(e, sp.draw(k), m)
        assert int(post.bad.item()) == 0 and post.tags.tolist() == paths[k]
        # seq_logp against scores - log_z: each within its own entry's bound of the float64 value
        tags = torch.zeros(B, S, dtype=torch.int64)
        for b in range(B):
            tags[b, :len(paths[k][b])] = torch.tensor(paths[k][b])
        full = dict(inp, tags=tags, gllh=torch.ones(B))
        bnd = CC.bounds(full)["llh"]
        for b in range(B):
            c = SC.chain(inp, b)
            terms = CC.path_terms(paths[k][b], c.x, c.start, c.end, c.T)
            exact = sum(terms) - float(c.log_z)
            mine = CC.viterbi_tol(c.L, terms) / 2 + SC.alpha_errors(c)[2] + 2 * SC.U_ACC * (abs(sum(terms)) + abs(float(c.log_z)))
            assert abs(float(lp[b, k]) - exact) <= mine, (b, k, float(lp[b, k]), exact, mine)
            assert abs(float(post.seq_logp[b]) - exact) <= float(bnd[b]), (b, k)
            assert abs(float(post.seq_logp[b]) - float(lp[b, k])) <= mine + float(bnd[b])
        ev = M.ChunkEvaluator(NAMES)
        ev.update(sp.draw(k), labels.cuda(), m)
        pl, gl = M.filter_batch(paths[k], labels, inp["mask"], NAMES)
        assert ev.compute().counts == M.evaluate_lists(pl, gl, NAMES).counts
