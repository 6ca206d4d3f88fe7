"""GPU: every kernel of csrc/crf.hip, element by element against float64 (tests/crf_check.py: the oracle's likelihood and its
autograd gradient for any mask, a Viterbi reference with an explicit tie rule, bounds derived from the number formats), at
the shapes where the host and device dispatch change path, through the C ABI -- the only way the row strides ld and ldd can
differ from C.  Each case runs twice: contiguous, then with emissions at ld = C + 3, d_emissions at ldd = C + 5 and every
operand two elements (int64: one) off its allocation's alignment; operands sit in NaN bands, outputs in sentinel bands.
tests/test_crf_gpu.py stays the check of the module against the oracle; this file checks what that one cannot see: single
elements, masks with holes, the path boundaries, the strides, the documented fillers."""
import functools

import pytest
import torch

import crf_check as cc
import kernel_check as kc
from kernel_check import F32

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


def _gin(values, ld=None, offset=0):
    """a float operand [rows, cols] inside NaN bands and NaN pad columns"""
    values = values.reshape(1, -1) if values.dim() == 1 else values
    return kc.Guarded(values.shape[0], values.shape[1], values.dtype, ld=ld, offset=offset, fill=kc.NAN_FILL[values.dtype],
                      init=values.cuda())


def _gint(values, offset=0):
    return kc.Guarded(values.shape[0], values.shape[1], I64, offset=offset, init=values.cuda())


def _ptr(g):
    return None if g is None else g.view.data_ptr()


def _call(inp, variant, tags=None, expect_rc=None):
    """icka_crf_llh, _grad, _decode and _score_decode once each on fresh guarded buffers -> the outputs on the CPU.  variant 0:
    contiguous; variant 1: ld = C + 3, ldd = C + 5, operands off alignment.  ``expect_rc``: {entry: return code} (default 0)."""
    from icka_amd import _lib
    from icka_amd import kernels as K
    lib = _lib.load()
    B, S, C = inp["e"].shape
    off, off64 = (2, 1) if variant else (0, 0)
    ld, ldd = (C + 3, C + 5) if variant else (C, C)
    expect_rc = expect_rc or {}
    e = _gin(inp["e"].reshape(B * S, C), ld=ld, offset=off)
    st, en, tr, gl = (_gin(inp[k], offset=off) for k in ("start", "end", "trans", "gllh"))
    tg = _gint(inp["tags"] if tags is None else tags, off64)
    mk = None if inp["mask"] is None else _gint(inp["mask"], off64)
    o = {"llh": kc.Guarded(1, B, F32, offset=off), "llh_sd": kc.Guarded(1, B, F32, offset=off),
         "de": kc.Guarded(B * S, C, F32, ld=ldd, offset=off),
         "dstart": kc.Guarded(1, C, F32, offset=off, init=inp["init"]["dstart"].reshape(1, C)),
         "dend": kc.Guarded(1, C, F32, offset=off, init=inp["init"]["dend"].reshape(1, C)),
         "dtrans": kc.Guarded(C, C, F32, offset=off, init=inp["init"]["dtrans"]),
         "best": kc.Guarded(B, S, I64, offset=off64), "best_score": kc.Guarded(1, B, F32, offset=off),
         "lens": kc.Guarded(1, B, I32, offset=off), "flat": kc.Guarded(1, B * S, I32, offset=off)}
    before = {k: g.flat.clone() for k, g in o.items()}
    s = K._stream()
    rc = {"llh": lib.icka_crf_llh(_ptr(e), ld, _ptr(tg), _ptr(mk), _ptr(st), _ptr(en), _ptr(tr), _ptr(o["llh"]), B, S, C, s),
          "grad": lib.icka_crf_grad(_ptr(e), ld, _ptr(tg), _ptr(mk), _ptr(st), _ptr(en), _ptr(tr), _ptr(gl), _ptr(o["de"]), ldd,
                                    _ptr(o["dstart"]), _ptr(o["dend"]), _ptr(o["dtrans"]), B, S, C, s),
          "decode": lib.icka_crf_decode(_ptr(e), ld, _ptr(mk), _ptr(st), _ptr(en), _ptr(tr), _ptr(o["best"]), _ptr(o["best_score"]),
                                        B, S, C, s),
          "score_decode": lib.icka_crf_score_decode(_ptr(e), ld, _ptr(tg), _ptr(mk), _ptr(st), _ptr(en), _ptr(tr), _ptr(o["llh_sd"]),
                                                    _ptr(o["lens"]), _ptr(o["flat"]), B * S, B, S, C, s)}
    torch.cuda.synchronize()
    for k, v in rc.items():
        assert v == expect_rc.get(k, 0), "icka_crf_%s returned %d" % (k, v)
    for n, g in list(o.items()) + [("emissions", e), ("start", st), ("end", en), ("trans", tr), ("gllh", gl), ("tags", tg)] + \
            ([("mask", mk)] if mk is not None else []):
        g.check(what="%s (variant %d)" % (n, variant))          # bands and pad columns bit-identical to their fill
    res = {k: g.view.cpu().clone() for k, g in o.items()}
    res["untouched"] = {k: bool(torch.equal(before[k].view(kc._INT[o[k].dtype]), o[k].flat.view(kc._INT[o[k].dtype]))) for k in o}
    res["de"] = res["de"].reshape(B, S, C)
    return res


@functools.lru_cache(maxsize=None)
def _run(case, variant):
    return _call(cc.make_case(case), variant)


def _bits(t):
    return t.contiguous().view(I32) if t.dtype == F32 else t.contiguous()


def _same(a, b, what):
    ne = _bits(a) != _bits(b)
    assert not bool(ne.any()), "%s: %d elements differ bitwise" % (what, int(ne.sum()))


def _label(forms, i):
    f = {x[i] for x in forms}
    return f.pop() if len(f) == 1 else "mixed"


def _raw_len(inp, b):
    S = inp["e"].shape[1]
    return S if inp["mask"] is None else max(int((inp["mask"][b] != 0).sum()), 1)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_likelihood_and_gradient_elements(case):
    ex = cc.expected(case)
    inp, ref, bnd, forms = ex["inp"], ex["ref"], ex["bounds"], ex["bounds"]["forms"]
    B, S, C = inp["e"].shape
    runs = [_run(case, 0), _run(case, 1)]
    for v, r in enumerate(runs):
        tag = "(variant %d)" % v
        for name in ("llh", "llh_sd", "de", "dstart", "dend", "dtrans"):
            assert bool(torch.isfinite(r[name]).all()), "%s %s: a NaN pad reached the result, or an element was not written" % (name, tag)
        _same(r["llh_sd"], r["llh"], "icka_crf_score_decode's llh against icka_crf_llh's " + tag)
        for b in range(B):
            kc.assert_within(r["llh"][0, b:b + 1], ref["llh"][b:b + 1], bnd["llh"][b:b + 1], "llh " + forms[b][0], verbose=False)
            kc.assert_within(r["de"][b], ref["de"][b], bnd["de"][b], "de " + forms[b][1], verbose=False)
            offp = [t for t in range(S) if t not in ex["chains"][b].pos]
            assert not offp or bool((r["de"][b, offp].view(I32) == 0).all()), "d_emissions at off positions of sample %d is not +0.0 %s" % (b, tag)
        for k in ("dstart", "dend", "dtrans"):
            kc.assert_within(r[k].reshape(ex["total"][k].shape), ex["total"][k], bnd[k], "%s %s" % (k, _label(forms, 1)), verbose=False)
    for name in ("llh", "de") + (("dstart", "dend", "dtrans") if B == 1 else ()):
        _same(runs[0][name], runs[1][name], "%s: contiguous against ld = C + 3, ldd = C + 5" % name)
    kc.report("crf_elements " + cc.case_id(case))


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_viterbi_paths_and_fillers(case):
    inp = cc.make_case(case)
    B, S, C = inp["e"].shape
    exact = case[4] == "integer"
    kind = "small staged" if cc.staged(S, C) else ("small unstaged" if cc.small(S, C) else "lds")
    runs = [_run(case, 0), _run(case, 1)]
    for v, r in enumerate(runs):
        off = 0
        for b in range(B):
            n = _raw_len(inp, b)
            row = r["best"][b].tolist()
            assert row[n:] == [-1] * (S - n), "best_tags of sample %d: -1 exactly from sum(mask) = %d on; got %s" % (b, n, row)
            assert all(t >= 0 for t in row[:n]), row
            assert int(r["lens"][0, b]) == n, ("lens", b, int(r["lens"][0, b]), n)
            flat = r["flat"][0, off:off + n].tolist()
            assert flat == row[:n], "tags_flat of sample %d at offset %d differs from icka_crf_decode's path" % (b, off)
            mrow = None if inp["mask"] is None else inp["mask"][b]
            w = cc.check_path(row[:n], float(r["best_score"][0, b]), inp["e"][b], mrow, inp["start"], inp["end"], inp["trans"],
                              exact, vref=cc.viterbi_of(case, b))
            kc.assert_within(torch.tensor([w]), torch.zeros(1), 1.0, "viterbi " + kind, verbose=False)
            off += n
        assert bool((r["flat"][0, off:] == kc.SENTINEL[I32]).all()), "tags_flat was written past sum(lens) = %d" % off
    for name in ("best", "best_score", "lens", "flat"):
        _same(runs[0][name], runs[1][name], "%s: contiguous against ld = C + 3" % name)
    kc.report("crf_viterbi " + cc.case_id(case))


@pytest.mark.parametrize("case", [c for c in cc.CASES if c[3] in ("prefix", "holes", "first_off")], ids=cc.case_id)
def test_pad_labels_at_off_positions_change_no_bit(case):
    """-100 and C + 5 where the labels at off positions were 0 and C - 1: ``tag_at`` clamps them to what every rule read before"""
    inp = cc.make_case(case)
    tags = cc.pad_labels(inp)
    if case[1] > 3:
        assert bool((tags != inp["tags"]).any())
    r, base = _call(inp, 0, tags=tags), _run(case, 0)
    for name in ("llh", "llh_sd", "de"):
        _same(r[name], base[name], "%s with pad labels" % name)
    if case[0] == 1:
        for name in ("dstart", "dend", "dtrans"):
            _same(r[name], base[name], "%s with pad labels" % name)


def test_refusals_at_S_times_C_above_12288_leave_every_output_bit():
    """(1, 193, 64): icka_crf_llh keeps nothing per position and must work; the other three return ICKA_E_SHAPE and write nothing"""
    case = cc.REFUSED_CASE
    inp = cc.make_case(case)
    ch = cc.chains(inp)
    ref = cc.reference(inp)
    e_logz = cc.log_errors(ch[0])[2]
    c = ch[0]
    e_llh = (2 * c.L + 2) * kc.U_ACC * sum(abs(t) for t in c.gold_terms) + e_logz + kc.U_ACC * (abs(c.num) + abs(float(c.log_z)))
    for v in (0, 1):
        r = _call(inp, v, expect_rc={"grad": cc.E_SHAPE, "decode": cc.E_SHAPE, "score_decode": cc.E_SHAPE})
        for k in ("llh_sd", "de", "dstart", "dend", "dtrans", "best", "best_score", "lens", "flat"):
            assert r["untouched"][k], "%s was written by a refused call" % k
        kc.assert_within(r["llh"][0], ref["llh"], kc.stored(torch.tensor([e_llh], dtype=torch.float64), ref["llh"], F32), "llh log",
                         verbose=False)
    kc.report("crf_elements " + cc.case_id(case))


def test_case_list_reaches_every_kernel_and_form():
    kern, fr = cc.assert_coverage()
    print("\n%d kernels over %d cases" % (len(kern), len(cc.CASES)))
