"""CPU: the references, bounds, dispatch and case list of tests/crf_check.py hold together -- f32 emulations of both forms of
the CRF kernels (tests/test_crf_scaled_cpu.py) stay inside every bound on every case, and each seeded fault leaves a bound or
an exact check on at least one case: the proof that tests/test_crf_elements_gpu.py fails on a subtly wrong kernel.  A
condition, not a measurement."""
import numpy as np
import pytest
import torch

import crf_check as cc
import crf_posterior_oracle as PO
import test_crf_scaled_cpu as EM
from oracle import crf_oracle as O

F64 = torch.float64
QUANT = ("llh", "de", "dstart", "dend", "dtrans")
SHORT = [c for c in cc.CASES if c[1] <= 12]


def _np(inp, b):
    return (inp["e"][b].numpy(), inp["tags"][b].numpy(), None if inp["mask"] is None else inp["mask"][b].numpy(),
            inp["start"].numpy(), inp["end"].numpy(), inp["trans"].numpy())


def _emulate(case, form, fault=None, e_of=None):
    """One call of icka_crf_grad + icka_crf_llh on a case, every sample in ``form`` -> (the five outputs as the kernels leave
    them (parameter gradients added to the initial content, in f32), the form of each sample: a sample on which the scaled
    form gives up is redone in the log domain, as the kernel does), or None if "lin" was asked and no sample stays scaled."""
    inp = cc.make_case(case)
    B, S, C = inp["e"].shape
    fn = EM.scaled_full if form == "lin" else EM.log_full
    out = {"llh": np.zeros(B, np.float32), "de": np.zeros((B, S, C), np.float32)}
    for k in ("dstart", "dend", "dtrans"):
        out[k] = inp["init"][k].numpy().copy()
    used = []
    for b in range(B):
        a = list(_np(inp, b))
        if e_of is not None:
            a[0] = e_of(a[0])
        r = fn(*a, g=float(inp["gllh"][b]), fault=fault)
        used.append(form if r["ok"] else "log")
        if not r["ok"]:
            r = EM.log_full(*a, g=float(inp["gllh"][b]), fault=fault)
        out["llh"][b], out["de"][b] = r["llh"], r["de"]
        for k in ("dstart", "dend", "dtrans"):
            out[k] = (out[k] + r[k]).astype(np.float32)
    return (out, used) if form in used else None


def _ratios(case, out_used):
    """worst |out - ref| / bound per quantity under the bound of ``form``, and whether the exact checks hold (exact +0.0 at off
    positions of d_emissions, nothing left unwritten)"""
    out, used = out_used
    ex = cc.expected(case)
    inp = ex["inp"]
    bnd = cc.bounds(inp, ex["chains"], ex["ref"], inp["init"], force=used)
    ratios = {}
    for k in QUANT:
        ref = ex["ref"][k] if k in ("llh", "de") else ex["total"][k]
        b = bnd[k] if k in ("llh", "de") else cc.stored(bnd[k], ref, torch.float32)
        o = torch.from_numpy(np.asarray(out[k], np.float64))
        err = (o - ref).abs()
        err = torch.where(torch.isfinite(o), err, torch.full_like(err, float("inf")))
        r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
        ratios[k] = float(r.max())
    B, S, C = inp["e"].shape
    exact = True
    for b, c in enumerate(ex["chains"]):
        offp = [t for t in range(S) if t not in c.pos]
        exact = exact and all(bool((torch.from_numpy(out["de"][b, t]).view(torch.int32) == 0).all()) for t in offp)
    return ratios, exact


def _scaled_possible(case):
    B, S, C = case[:3]
    return cc.small(S, C) and S * C <= cc.CRF_LIN_SC


# --------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_the_three_statements_of_the_reference_agree(case):
    """autograd through oracle.crf_llh == 1[y] - marginal of the plain chain == the token marginals of crf_posterior_oracle"""
    ex = cc.expected(case)
    inp, ref = ex["inp"], ex["ref"]
    alt = cc.reference_from_chains(inp, ex["chains"])
    for k in QUANT:
        scale = 1.0 + float(ref[k].abs().max())
        assert float((ref[k] - alt[k]).abs().max()) <= 1e-9 * scale, k
    for b, s in enumerate(PO.batch(inp["e"], inp["mask"], inp["start"], inp["end"], inp["trans"])):
        c = ex["chains"][b]
        assert s.pos == c.pos
        assert float((s.marg[c.pos] - c.marg).abs().max()) <= 1e-12
        assert abs(s.log_z - float(c.log_z)) <= 1e-9 * (1 + abs(s.log_z))


@pytest.mark.parametrize("case", cc.BRUTE, ids=cc.case_id)
def test_reference_against_enumeration(case):
    """All C^L paths over the on positions: log Z, the marginals; and for prefix-type masks the Viterbi optimum."""
    ex = cc.expected(case)
    inp = ex["inp"]
    for b, c in enumerate(ex["chains"]):
        mrow = None if inp["mask"] is None else inp["mask"][b]
        log_z, marg, _, _ = PO.enumerate_sample(inp["e"][b].double(), mrow, inp["start"].double(), inp["end"].double(),
                                                inp["trans"].double(), [0] * c.L, [])
        assert abs(log_z - float(c.log_z)) < 1e-12
        assert float((marg[c.pos] - c.marg).abs().max()) < 1e-12
        assert abs(float(ex["ref"]["llh"][b]) - (c.num - log_z)) < 1e-12
        path, score, _, _, _ = cc.viterbi_ref(inp["e"][b], mrow, inp["start"], inp["end"], inp["trans"])
        if cc.mask_is_prefix(mrow, case[1]):
            _, best, best_s = O.brute_force(inp["e"][b].double(), len(path), inp["start"].double(), inp["end"].double(),
                                            inp["trans"].double())
            assert abs(float(best_s) - score) < 1e-12
            assert abs(sum(cc.path_terms(path, inp["e"][b], inp["start"], inp["end"], inp["trans"])) - score) < 1e-12
            if case[4] != "integer":
                assert path == best


@pytest.mark.parametrize("case", [c for c in cc.CASES if c[4] != "integer" and c[1] <= 65], ids=cc.case_id)
def test_viterbi_reference_equals_the_oracle_decode(case):
    """the package's rule for masks with holes, stated twice: plain loops here, tensors in oracle.crf_decode (no ties: random floats)"""
    inp = cc.make_case(case)
    B, S, C = inp["e"].shape
    want = O.crf_decode(inp["e"].double(), None if inp["mask"] is None else inp["mask"] != 0, inp["start"].double(),
                        inp["end"].double(), inp["trans"].double())
    for b in range(B):
        assert cc.viterbi_ref(inp["e"][b], None if inp["mask"] is None else inp["mask"][b], inp["start"], inp["end"],
                              inp["trans"])[0] == want[b]


def test_viterbi_tie_rule():
    z = torch.zeros
    path, score, _, _, bp = cc.viterbi_ref(z(5, 4), torch.tensor([1, 0, 1, 1, 0]), z(4), z(4), z(4, 4))
    assert path == [0, 0, 0] and score == 0.0 and all(a == [0] * 4 for a in bp[1:])
    e = z(3, 4)
    e[2, 1] = e[2, 3] = 1.0          # two equal final scores: the smaller tag
    assert cc.viterbi_ref(e, None, z(4), z(4), z(4, 4))[0] == [0, 0, 1]


# ------------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_emulations_stay_inside_every_bound(case):
    forms = cc.expected(case)["bounds"]["forms"]
    done = []
    for form in ("lin", "log"):
        if form == "lin" and not _scaled_possible(case):
            continue
        out = _emulate(case, form)
        if out is None:
            continue
        ratios, exact = _ratios(case, out)
        print("RATIO emulation %-4s %-32s %s" % (form, cc.case_id(case), " ".join("%s %.3f" % kv for kv in ratios.items())))
        assert exact
        assert all(r <= 1 for r in ratios.values()), (form, ratios)
        done.append(form)
    assert "log" in done


def _caught(case, form, fault, e_of=None):
    out = _emulate(case, form, fault, e_of)
    if out is None and e_of is not None:          # NaN normalisers: the kernel redoes the sample in the log domain
        out = _emulate(case, "log", fault, e_of)
    if out is None:
        return False
    ratios, exact = _ratios(case, out)
    return not exact or any(not (r <= 1) for r in ratios.values())


@pytest.mark.parametrize("fault,form", [(fa, fo) for fa in EM.FAULTS_LIN for fo in ("lin", "log")
                                        if (fa, fo) != ("norm_next", "log")])          # (the log form has no normaliser)
def test_seeded_faults_leave_a_bound(fault, form):
    hit = [cc.case_id(c) for c in SHORT if (form == "log" or _scaled_possible(c)) and _caught(c, form, fault)]
    print("\n%s / %s caught on: %s" % (fault, form, ", ".join(hit)))
    assert hit, "no short case catches the fault %s in the %s form" % (fault, form)


@pytest.mark.parametrize("form", ["lin", "log"])
def test_an_emission_row_read_with_stride_C_leaves_a_bound(form):
    """ld = C + 3: the test pads every row with three NaNs; a kernel that steps by C reads them"""
    def strided(e):
        S, C = e.shape
        buf = np.full((S, C + 3), np.nan, np.float32)
        buf[:, :C] = e
        return buf.reshape(-1)[:S * C].reshape(S, C)
    hit = [c for c in SHORT if c[1] > 1 and (form == "log" or _scaled_possible(c)) and _caught(c, form, None, strided)]
    assert len(hit) == len([c for c in SHORT if c[1] > 1 and (form == "log" or _scaled_possible(c))])


def _viterbi_f32(e, mask_row, start, end, trans, on_steps_only=False):
    """the kernels' Viterbi in f32 (first maximum wins); ``on_steps_only``: the fault -- back-pointers recorded on on steps only,
    so the back-trace walks the history of the on steps"""
    f = np.float32
    S, C = e.shape
    on, last = EM.mask_rules(mask_row, S)
    score = (start + e[0]).astype(f)
    hist = []
    for t in range(1, S):
        v = (score[:, None] + trans).astype(f)
        if on[t] or not on_steps_only:
            hist.append(v.argmax(0))
        if on[t]:
            score = (v.max(0) + e[t]).astype(f)
    fin = (score + end).astype(f)
    bt = int(fin.argmax())
    path = [bt]
    for h in reversed(hist[:last]):
        bt = int(h[bt])
        path.append(bt)
    return path[::-1], float(fin.max())


def test_back_pointers_on_on_steps_only_are_caught():
    """on the integer cases the GPU test demands the exact path of the tie-rule reference"""
    hit = []
    for case in [c for c in cc.CASES if c[4] == "integer" and c[1] <= 65]:
        inp = cc.make_case(case)
        for b in range(case[0]):
            a = _np(inp, b)
            args = (a[0], a[2], a[3], a[4], a[5])
            ref = cc.viterbi_ref(inp["e"][b], None if inp["mask"] is None else inp["mask"][b], inp["start"], inp["end"], inp["trans"])
            good, bad = _viterbi_f32(*args), _viterbi_f32(*args, on_steps_only=True)
            assert good[0] == ref[0] and good[1] == ref[1]
            if bad[0] != ref[0]:
                hit.append(cc.case_id(case))
    assert hit


# ---------------------------------------------------------------------------------------------------- the dispatch
def test_case_list_reaches_every_kernel_and_form():
    kern, fr = cc.assert_coverage()
    print("\n%d kernels; forms of the small kernels: %s" % (len(kern), {k: sorted(v) for k, v in fr.items()}))
    S_C = {(c[1], c[2]) for c in cc.CASES}
    for edge in ((1, 3), (6, 16), (6, 17), (63, 13), (64, 13), (65, 13), (315, 13), (316, 13), (512, 8), (256, 16), (257, 16),
                 (512, 16), (513, 16), (192, 64)):
        assert edge in S_C, edge
    assert 315 * 13 <= cc.CRF_LIN_SC < 316 * 13 and 256 * 16 == cc.CRF_LIN_SC and 192 * 64 == cc.CRF_MAX_SC < 193 * 64
    assert cc.small(512, 16) and not cc.small(513, 16) and not cc.small(6, 17)
    assert cc.staged(256, 16) and not cc.staged(257, 16)
    assert [cc.refused(e, 193, 64) for e in cc.ENTRIES] == [False, True, True, True]
    for case in cc.CASES:
        m = cc.make_case(case)["mask"]
        assert m is None or bool(((m != 0).sum(1) >= 1).all())
    # the short twin of every long edge: each (mask kind, form) pair also runs at S <= 8
    assert {c[3] for c in cc.CASES if c[1] <= 8} == set(cc.MASKS)


def test_pad_labels_clamp_to_what_was_there():
    n, seen = 0, set()
    for case in cc.CASES:
        inp = cc.make_case(case)
        t2 = cc.pad_labels(inp)
        C = case[2]
        assert torch.equal(cc.clamp_tags(t2, C), inp["tags"])
        n += int((t2 != inp["tags"]).sum())
        seen |= set((t2 - inp["tags"]).reshape(-1).tolist())
        if case[3] in ("holes", "first_off") and case[1] > 3:
            assert bool((t2 != inp["tags"]).any()), cc.case_id(case)
    assert n > 0 and seen == {0, -100, 6}
