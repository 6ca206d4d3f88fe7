"""GPU: icka_crf_posterior, CRF.marginals / CRF.posterior and EntityDecoder against the float64 restatement of their definitions
(tests/crf_posterior_oracle.py), on the paths the GPU itself decoded unless a test says otherwise.

Bars.  Marginals, token_conf and the confidence of one-token chunks: 1e-3 absolute (test_crf_gpu.py:42 gives the emission
gradient, the same quantity, that bar); 2e-3 / 4e-3 in the extreme-score cases (test_crf_gpu.py:96).  log_z and seq_logp:
rtol 2e-5, atol 2e-4 (test_crf_gpu.py:37); extreme: rtol 3e-5, atol 2e-3 max(1, scale / 10) (test_crf_gpu.py:92).  The
confidence of longer chunks has no number in the project: every test prints the worst error it saw ("ENT_CONF ...") and
ENT_CONF_BAR is twice the largest of them over the ordinary cases (the extreme-score cases keep the bar of their marginals)."""
import pytest
import torch

import crf_posterior_oracle as PO
import kernel_check as kc

pytestmark = pytest.mark.gpu

F32 = torch.float32
MARG_BAR = 1e-3
ENT_CONF_BAR = 1.9e-4    # 2x the 9.14e-05 measured on MI355X (shape 2x192x64, the log-domain body; printed by the tests)


def _case(B, S, Cn, seed, ragged=True):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(B, S, Cn, generator=g) * 2.0
    lens = torch.randint(1, S + 1, (B,), generator=g) if ragged else torch.full((B,), S)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    mask = (torch.arange(S)[None, :] < lens[:, None])
    return e, mask, lens


def _crf(Cn, seed=0, batch_first=True):
    from icka_amd.crf import CRF
    torch.manual_seed(seed)
    return CRF(Cn, batch_first=batch_first).cuda()


def _params(crf):
    return [p.detach().cpu() for p in (crf.start_transitions, crf.end_transitions, crf.transitions)]


def _names(Cn):
    """A label map for any number of tags: id 0 outside every chunk, two types, every fifth tag a begin tag -- chunks of
    several tokens are common on random paths."""
    return ["O"] + [("B-" if j % 5 == 1 else "I-") + ("PER", "LOC")[j % 2] for j in range(1, Cn)]


def _split(h):
    from icka_amd.crf import split_tags
    return split_tags(h["lens"], h["tags_flat"])


def _compare(h, marg, samples, names, types, what, marg_bar=MARG_BAR, z_tol=(2e-5, 2e-4), ent_bar=None):
    """Every output of a posterior call (``h`` = CrfPosterior.host()) against the oracle ``samples`` on the paths in ``h``;
    returns the worst error of the confidence of a chunk longer than one token."""
    assert h["bad"] == 0
    paths = _split(h)
    off, worst_long, worst_tok = 0, 0.0, 0.0
    rtol, atol = z_tol
    for b, (smp, path) in enumerate(zip(samples, paths)):
        assert len(path) == smp.L, (what, b, len(path), smp.L)
        assert abs(h["log_z"][b] - smp.log_z) <= atol + rtol * abs(smp.log_z), (what, b, h["log_z"][b], smp.log_z)
        ref = smp.seq_logp(path)
        assert abs(h["seq_logp"][b] - ref) <= atol + rtol * abs(ref), (what, b, h["seq_logp"][b], ref)
        assert h["seq_logp"][b] <= atol
        tc = smp.token_conf(path)
        err = max(abs(a - r) for a, r in zip(h["token_conf"][off:off + smp.L], tc))
        worst_tok = max(worst_tok, err)
        assert err < marg_bar, (what, b, "token_conf", err)
        if marg is not None:
            err = (marg[b].double() - smp.marg).abs().max().item()
            worst_tok = max(worst_tok, err)
            assert err < marg_bar, (what, b, "marginals", err)
            offp = torch.ones(smp.S, dtype=torch.bool)
            offp[smp.pos] = False
            assert bool((marg[b][offp] == 0).all()), (what, b, "off-positions")
        if names is not None:
            ref_ent = smp.entities(path, names)
            n = h["n_ent"][b]
            got = [tuple(h["ent"][3 * k:3 * k + 3]) for k in range(off, off + n)]
            assert [(types[t], s, e) for t, s, e in got] == [r[:3] for r in ref_ent], (what, b)
            for k, (_, s, e, p) in enumerate(ref_ent):
                err = abs(h["ent_conf"][off + k] - p)
                if e - s == 1:
                    assert err < marg_bar and h["ent_conf"][off + k] == h["token_conf"][off + s], (what, b, k, err)
                else:
                    worst_long = max(worst_long, err)
        off += smp.L
    print("ENT_CONF %-40s worst |error| of chunks longer than one token %.3e; of token marginals %.3e" % (what, worst_long, worst_tok))
    assert worst_long < (ENT_CONF_BAR if ent_bar is None else ent_bar), (what, worst_long)
    return worst_long


def _posterior(crf, e, mask, names=None, paths=None, marginals=True):
    from icka_amd import metrics
    table, types = (None, None) if names is None else metrics.label_table(names, "O", ())
    post = crf.posterior(e.cuda(), paths, None if mask is None else mask.cuda(), marginals=marginals, label_table=table)
    return post, types


SHAPES = [(8, 128, 13), (8, 128, 15),            # the workload's label counts
          (3, 40, 16), (3, 40, 17),              # both sides of the register-variant boundary
          (2, 7, 64), (2, 192, 64),              # S * C = CRF_MAX_SC exactly
          (2, 512, 8), (2, 257, 16),             # at and just past the scaled tiles
          (3, 1, 13), (3, 63, 13), (3, 64, 13), (3, 65, 13),      # mask-word boundary
          (1, 9, 13), (130, 3, 13)]              # the in-kernel prefix of lens crosses two 64-lane rounds


@pytest.mark.parametrize("B,S,Cn", SHAPES)
def test_posterior_against_oracle(B, S, Cn):
    e, mask, lens = _case(B, S, Cn, seed=B * 1000 + S + Cn)
    crf = _crf(Cn, seed=S + Cn)
    names = _names(Cn)
    post, types = _posterior(crf, e, mask, names)
    h = post.host()
    assert h["lens"] == lens.tolist()
    _compare(h, post.marginals.cpu(), PO.batch(e, mask, *_params(crf)), names, types, "shape %dx%dx%d" % (B, S, Cn))


def test_definitions_against_enumeration():
    B, S, Cn = 4, 5, 3
    e, mask, lens = _case(B, S, Cn, seed=4053)
    crf = _crf(Cn, seed=2)
    names = ["O", "B-PER", "I-PER"]
    post, types = _posterior(crf, e, mask, names)
    h, marg = post.host(), post.marginals.cpu()
    st, en, tr = (p.double() for p in _params(crf))
    paths, off = _split(h), 0
    for b, path in enumerate(paths):
        ents = [tuple(h["ent"][3 * k:3 * k + 3]) for k in range(off, off + h["n_ent"][b])]
        log_z, m, logp, sp = PO.enumerate_sample(e[b].double(), mask[b], st, en, tr, path, [(s, t) for _, s, t in ents])
        assert abs(h["log_z"][b] - log_z) < 2e-4 and abs(h["seq_logp"][b] - logp) < 2e-4
        assert (marg[b].double() - m).abs().max().item() < MARG_BAR
        for k, p in enumerate(sp):
            assert abs(h["ent_conf"][off + k] - p) < MARG_BAR, (b, k)
        off += len(path)


def test_shape_beyond_the_lds_budget_is_refused():
    crf = _crf(64)
    with pytest.raises(ValueError):
        crf.posterior(torch.zeros(2, 193, 64, device="cuda"))
    with pytest.raises(ValueError):
        crf.marginals(torch.zeros(2, 193, 64, device="cuda"))


@pytest.mark.parametrize("kind", ["prefix", "holes", "first_off", "none"])
@pytest.mark.parametrize("Cn", [13, 20])
def test_masks(kind, Cn):
    B, S = 6, 70
    e, mask, lens = _case(B, S, Cn, seed=31 + Cn)
    if kind in ("holes", "first_off"):
        g = torch.Generator().manual_seed(8)
        mask = torch.rand(B, S, generator=g) < 0.6
        mask[:, 0] = kind == "holes"
        mask[2] = False                                # an all-zero row: path length 1
        mask[2, 0] = kind == "holes"
    if kind == "none":
        mask = None
    crf = _crf(Cn, seed=5)
    names = _names(Cn)
    post, types = _posterior(crf, e, mask, names)
    samples = PO.batch(e, mask, *_params(crf))
    h = post.host()
    assert h["lens"] == [s.L for s in samples]
    _compare(h, post.marginals.cpu(), samples, names, types, "mask %s C=%d" % (kind, Cn))
    m = crf.marginals(e.cuda(), None if mask is None else mask.cuda())
    assert torch.equal(m, post.marginals)              # the path-free launch computes the same marginals


@pytest.mark.parametrize("scale,forbid", [(2.0, True), (40.0, False), (60.0, True)])
def test_extreme_scores(scale, forbid):
    """The set-up of test_crf_gpu.py::test_crf_extreme_scores_against_oracle: -1e4 "forbidden" transitions and emission spreads
    up to e^+-200 -- the scaled recursion stays in range or hands the sample to the log-domain body."""
    B, S, Cn = 6, 64, 13
    e, mask, lens = _case(B, S, Cn, seed=77)
    e = e * (scale / 2.0)
    crf = _crf(Cn, seed=int(scale) * 2 + int(forbid))
    with torch.no_grad():
        if forbid:
            g = torch.Generator().manual_seed(5)
            blocked = torch.rand(Cn, Cn, generator=g) < 0.3
            blocked[torch.arange(Cn), torch.arange(Cn)] = False
            crf.transitions[blocked.cuda()] = -1e4
            crf.start_transitions[::3] = -1e4
    names = _names(Cn)
    post, types = _posterior(crf, e, mask, names)
    h = post.host()
    for k in ("log_z", "seq_logp"):
        assert all(v == v and abs(v) != float("inf") for v in h[k]), k
    assert bool(torch.isfinite(post.marginals).all())
    # a longer chunk's posterior is at most its tokens' marginals and carries the same f32 rounding of scores of size 7e3:
    # the extreme cases give it the bar they give the marginals
    bar = 2e-3 if scale < 40 else 4e-3
    _compare(h, post.marginals.cpu(), PO.batch(e, mask, *_params(crf)), names, types, "extreme scale %g forbid %d" % (scale, forbid),
             marg_bar=bar, z_tol=(3e-5, 2e-3 * max(1.0, scale / 10)), ent_bar=bar)


def test_cross_checks_against_the_existing_kernels():
    B, S, Cn = 8, 128, 13
    e, mask, lens = _case(B, S, Cn, seed=99)
    crf = _crf(Cn, seed=1)
    post, _ = _posterior(crf, e, mask)
    h, marg = post.host(), post.marginals
    paths = _split(h)
    tags = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(paths):
        tags[b, :len(p)] = torch.tensor(p)
    eg = e.cuda().requires_grad_(True)
    llh = crf(eg, tags.cuda(), mask=mask.cuda().byte(), reduction="none")
    assert torch.allclose(post.seq_logp, llh.detach(), rtol=2e-5, atol=2e-4), (post.seq_logp, llh)
    llh.sum().backward()
    onehot = torch.nn.functional.one_hot(tags, Cn).float() * mask[:, :, None]
    assert (marg.cpu() - (onehot - eg.grad.cpu())).abs().max().item() < MARG_BAR
    off = 0
    for b, p in enumerate(paths):
        gathered = marg[b, torch.arange(len(p)), torch.tensor(p)].cpu()
        assert torch.equal(gathered, torch.tensor(h["token_conf"][off:off + len(p)], dtype=F32)), b
        off += len(p)
    sums = marg.sum(-1).cpu()
    assert (sums[mask] - 1).abs().max().item() < MARG_BAR and bool((marg.cpu()[~mask] == 0).all())


def _entity_batch():
    """Paths with the chunk shapes that matter, and emissions that favour them (confidences of order 0.1 .. 1)."""
    from icka_amd import metrics
    lmap = metrics.label_list_map(metrics.REFERENCE_LABEL_LIST)
    idx = {v: k for k, v in lmap.items()}
    T = lambda s: [idx[n] for n in s.split()]
    paths = [T("B-PER B-PER I-PER O I-PER I-ORG O B-LOC I-LOC I-LOC"),     # adjacent B- / B-, a type change without B, to the end
             T("O O O O"),                                                 # no chunk
             T("B-LOC " + "I-LOC " * 40 + "O B-MISC"),                     # a long chunk, a chunk of one token at the end
             T("I-ORG"),
             T("X [CLS] B-ORG I-ORG [SEP] PAD PAD O " + "B-PER I-PER " * 30)]   # many chunks, across a 64-position word
    B, S, Cn = len(paths), 70, 15
    g = torch.Generator().manual_seed(21)
    e = torch.randn(B, S, Cn, generator=g) * 2.0
    mask = torch.zeros(B, S, dtype=torch.bool)
    for b, p in enumerate(paths):
        mask[b, :len(p)] = True
        e[b, torch.arange(len(p)), torch.tensor(p)] += 3.0
    return e, mask, paths, lmap


def test_entities_of_given_paths_and_tolist():
    from icka_amd import EntityDecoder, metrics
    e, mask, paths, lmap = _entity_batch()
    crf = _crf(15, seed=3)
    dec = EntityDecoder.for_label_list(crf, metrics.REFERENCE_LABEL_LIST)
    samples = PO.batch(e, mask, *_params(crf))
    ref = [s.entities(p, lmap) for s, p in zip(samples, paths)]
    assert ref[1] == [] and len(ref[2]) == 2 and ref[2][0][1:3] == (0, 41) and len(ref[4]) > 30
    tensor_paths = torch.zeros(mask.shape, dtype=torch.long)
    for b, p in enumerate(paths):
        tensor_paths[b, :len(p)] = torch.tensor(p)
    worst = 0.0
    for form in (paths, tensor_paths.cuda(), "device_tags"):
        if isinstance(form, str):
            from icka_amd.crf import DeviceTags
            form = DeviceTags(torch.tensor([len(p) for p in paths], dtype=torch.int32).cuda(),
                              torch.tensor([v for p in paths for v in p], dtype=torch.int32).cuda())
        ents = dec(e.cuda(), mask=mask.cuda(), paths=form)
        assert ents.tags.tolist() == paths
        got = ents.tolist()
        assert ents.n_ent.tolist() == [len(r) for r in ref]
        for b in range(len(paths)):
            assert [g[:3] for g in got[b]] == [r[:3] for r in ref[b]] == metrics.chunks(paths[b], lmap), b
            for g_, r in zip(got[b], ref[b]):
                bar = MARG_BAR if r[2] - r[1] == 1 else ENT_CONF_BAR
                worst = max(worst, abs(g_[3] - r[3]) if r[2] - r[1] > 1 else 0.0)
                assert abs(g_[3] - r[3]) < bar, (b, g_, r)
        assert abs(ents.seq_logp.cpu()[0].item() - samples[0].seq_logp(paths[0])) < 2e-4 + 2e-5 * abs(samples[0].seq_logp(paths[0]))
    print("ENT_CONF %-40s worst |error| of chunks longer than one token %.3e" % ("given paths", worst))
    # the decoder's own Viterbi paths
    ents = dec(e.cuda(), mask=mask.cuda())
    own = ents.tags.tolist()
    assert [[g[:3] for g in r] for r in ents.tolist()] == [metrics.chunks(p, lmap) for p in own]


def _guarded_outputs(B, S, Cn):
    cap = B * S
    out, checks = {}, []
    for name, rows, cols, dt, init in (("log_z", 1, B, F32, -7.0), ("seq_logp", 1, B, F32, -7.0), ("token_conf", 1, cap, F32, -7.0),
                                       ("marginals", B * S, Cn, F32, -7.0), ("ent", cap, 3, torch.int32, -77),
                                       ("ent_conf", 1, cap, F32, -7.0), ("n_ent", 1, B, torch.int32, -77),
                                       ("bad", 1, 1, torch.int32, 0)):
        v, chk = kc.guarded(rows, cols, dt, init=init)
        out[name] = v.view(B, S, Cn) if name == "marginals" else (v if name == "ent" else v[0])
        checks.append(chk)
    return out, checks


def _launch(crf, e, mask, lens, flat, table, out):
    from icka_amd import kernels as K
    K.crf_posterior(e, mask, crf.start_transitions.detach(), crf.end_transitions.detach(), crf.transitions.detach(), out["log_z"],
                    out["bad"], lens=lens, tags_flat=flat, seq_logp=out["seq_logp"], token_conf=out["token_conf"],
                    marginals=out["marginals"], label_table=table, ent=out["ent"], ent_conf=out["ent_conf"], n_ent=out["n_ent"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("Cn", [15, 20])
def test_guard_bands_and_refusals(Cn):
    from icka_amd import EntityDecoder, metrics
    from icka_amd.crf import DeviceTags
    B, S = 5, 40
    g = torch.Generator().manual_seed(3)
    e = (torch.randn(B, S, Cn, generator=g) * 2.0).cuda()
    lens_l = [S, 1, 7, 12, S - 3]
    mask = (torch.arange(S)[None, :] < torch.tensor(lens_l)[:, None]).long().cuda()
    crf = _crf(Cn, seed=4)
    names = _names(Cn)
    table = torch.tensor(metrics.label_table(names, "O", ())[0], dtype=torch.int32).cuda()
    tags = crf.decode(e, mask=mask, out=DeviceTags.empty(B, S, "cuda"))
    assert tags.lens.tolist() == lens_l
    total, offs = sum(lens_l), [sum(lens_l[:b]) for b in range(B)]

    good, checks = _guarded_outputs(B, S, Cn)
    _launch(crf, e, mask, tags.lens, tags.tags_flat, table, good)
    for chk in checks:
        chk()
    assert good["bad"].item() == 0
    n_ent = good["n_ent"].tolist()
    assert bool((good["token_conf"][total:] == -7.0).all()) and bool(torch.isfinite(good["token_conf"][:total]).all())
    for b in range(B):      # rows k >= n_ent[b] of a segment, and everything past sum(lens), are not written
        lo, hi = offs[b] + n_ent[b], offs[b] + lens_l[b]
        assert bool((good["ent"][lo:hi] == -77).all()) and bool((good["ent_conf"][lo:hi] == -7.0).all()), b
        assert bool(torch.isfinite(good["ent_conf"][offs[b]:lo]).all())
    assert bool((good["ent"][total:] == -77).all()) and bool((good["ent_conf"][total:] == -7.0).all())

    # one sample with lens off by one (the last: the offsets of the others stay), another with a tag id = C
    lens_c, flat_c = tags.lens.clone(), tags.tags_flat.clone()
    lens_c[B - 1] -= 1
    flat_c[offs[2] + 3] = Cn
    badrun, checks = _guarded_outputs(B, S, Cn)
    _launch(crf, e, mask, lens_c, flat_c, table, badrun)
    for chk in checks:
        chk()
    assert badrun["bad"].item() == 2
    for b in range(B):
        seg = slice(offs[b], offs[b] + lens_l[b])
        if b in (2, B - 1):
            n = lens_l[b] - (1 if b == B - 1 else 0)
            assert badrun["n_ent"][b].item() == 0
            assert bool(torch.isnan(badrun["log_z"][b])) and bool(torch.isnan(badrun["seq_logp"][b]))
            assert bool(torch.isnan(badrun["token_conf"][offs[b]:offs[b] + n]).all()) and bool(torch.isnan(badrun["marginals"][b]).all())
            assert bool((badrun["ent"][seg] == -77).all()) and bool((badrun["ent_conf"][seg] == -7.0).all())
        else:
            for k in ("log_z", "seq_logp", "n_ent", "marginals"):
                assert torch.equal(badrun[k][b], good[k][b]), (k, b)
            for k in ("token_conf", "ent", "ent_conf"):
                assert torch.equal(badrun[k][seg], good[k][seg]), (k, b)
    dec = EntityDecoder(crf, names)
    ents = dec(e, mask=mask, paths=DeviceTags(lens_c, flat_c))
    with pytest.raises(ValueError, match="2 sample"):
        ents.tolist()


def test_decoder_call_is_capturable():
    from icka_amd import EntityDecoder, metrics
    B, S, Cn = 4, 128, 15
    crf = _crf(Cn, seed=6)
    dec = EntityDecoder.for_label_list(crf, metrics.REFERENCE_LABEL_LIST)
    cases = [_case(B, S, Cn, seed=50 + i) for i in range(3)]
    static_em, static_mask = cases[0][0].cuda(), cases[0][1].cuda().long()
    dec(static_em, mask=static_mask)                   # warm-up outside the capture (the label table is uploaded once)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # captures on a side stream
        ents = dec(static_em, mask=static_mask)
    for e, mask, lens in cases[1:]:
        static_em.copy_(e.cuda()); static_mask.copy_(mask.cuda().long())
        graph.replay()
        torch.cuda.synchronize()
        replayed, h = ents.tolist(), ents.posterior.host()
        eager = dec(e.cuda(), mask=mask.cuda().long())
        he = eager.posterior.host()
        n = sum(h["lens"])
        assert h["lens"] == lens.tolist() == he["lens"] and replayed == eager.tolist()
        for k in ("log_z", "seq_logp", "n_ent"):
            assert h[k] == he[k], k
        assert h["tags_flat"][:n] == he["tags_flat"][:n] and h["token_conf"][:n] == he["token_conf"][:n]


def test_sequence_first_layout():
    B, S, Cn = 5, 9, 13
    e, mask, lens = _case(B, S, Cn, seed=12)
    crf_sf, crf_bf = _crf(Cn, seed=9, batch_first=False), _crf(Cn, seed=9)
    a = crf_sf.posterior(e.transpose(0, 1).cuda(), None, mask.transpose(0, 1).cuda(), marginals=True)
    b = crf_bf.posterior(e.cuda(), None, mask.cuda(), marginals=True)
    assert tuple(a.marginals.shape) == (S, B, Cn) and torch.equal(a.marginals.transpose(0, 1), b.marginals)
    assert a.tags.tolist() == b.tags.tolist() and torch.equal(a.seq_logp, b.seq_logp) and torch.equal(a.log_z, b.log_z)
    assert torch.equal(crf_sf.marginals(e.transpose(0, 1).cuda(), mask.transpose(0, 1).cuda()), a.marginals)
    tp = torch.zeros(S, B, dtype=torch.long)
    for i, p in enumerate(b.tags.tolist()):
        tp[:len(p), i] = torch.tensor(p)
    c = crf_sf.posterior(e.transpose(0, 1).cuda(), tp.cuda(), mask.transpose(0, 1).cuda())
    assert c.tags.tolist() == b.tags.tolist() and torch.equal(c.seq_logp, b.seq_logp)
    _compare(b.host(), b.marginals.cpu(), PO.batch(e, mask, *_params(crf_bf)), None, None, "sequence-first")
