"""GPU: the adversarial-training kernels element by element, through the C ABI -- icka_embed_fwd_adv / _h (csrc/layernorm.hip),
icka_adv_ascend, icka_adv_init_uniform, icka_adv_bump (csrc/adversarial.hip) -- against the float64 oracle of
tests/adversarial_oracle.py inside the bounds of tests/adversarial_check.py (tests/test_adversarial_cpu.py keeps those honest).
Every operand sits in NaN bands, every output in sentinel bands, and every buffer is checked after every call."""
import numpy as np
import pytest
import torch

import adversarial_check as ac
import adversarial_oracle as ao
import embed_check as ec
import kernel_check as kc
from embed_check import BF16, F16, F32, VOCAB, SEED, EPS_LN
from test_embed_elements_gpu import Bufs, _env, _ok, _ptr, _same

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3
I64 = torch.int64
EPS = float(np.float32(0.7))


# ------------------------------------------------------------------------------------------------ forward
FWD_CASES = [ec.ecase(B, S, H, p=p, twin=twin) for H in ec.H_ALL for (B, S) in ((1, 1), (3, 5), (2, 37))
             for (p, twin) in ((0.0, "f32"), (0.1, "f16"))]


@pytest.mark.parametrize("c", FWD_CASES, ids=ec.case_id)
def test_embed_fwd_adv(c):
    lib, K, s = _env()
    inp, what = ec.embed_inputs(c), "embed_fwd_adv " + ec.case_id(c)
    lay = ec.embed_layout(c, inp)
    B, S, H, nt = c["B"], c["S"], c["H"], c["n_type"]
    M = B * S
    tw = F16 if c["twin"] == "f16" else F32
    delta = ec.rnd(M, H, seed=71, scale=0.3)
    bf = Bufs()
    ids, tt = bf.fin(inp["ids"].reshape(M, 1), "ids"), bf.fin(inp["tt"].reshape(M, 1), "tt")
    word, pos, typ = bf.fin(inp["word"], "word"), bf.fin(inp["pos"], "pos"), bf.fin(inp["typ"], "type")
    gamma, beta, dl = bf.fin(inp["gamma"], "gamma"), bf.fin(inp["beta"], "beta"), bf.fin(delta, "delta")
    plain, adv = (lib.icka_embed_fwd_h, lib.icka_embed_fwd_adv_h) if tw == F16 else (lib.icka_embed_fwd, lib.icka_embed_fwd_adv)
    o = {}
    for tag in ("plain", "null", "delta"):
        o[tag] = dict(y=bf.out(M, H, BF16, tag + " y"), twin=bf.out(M, H, tw, tag + " twin"), xhat=bf.out(M, H, BF16, tag + " xhat"),
                      rstd=bf.out(M, 1, F32, tag + " rstd"))
    head = (_ptr(ids), _ptr(tt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta))
    tail = (B, S, H, VOCAB, nt, EPS_LN, c["p"], SEED, s)
    outs = lambda t: (_ptr(o[t]["y"]), _ptr(o[t]["twin"]), _ptr(o[t]["xhat"]), _ptr(o[t]["rstd"]))
    _ok(plain(*head, *outs("plain"), *tail), "icka_embed_fwd")
    _ok(adv(*head, None, *outs("null"), *tail), "icka_embed_fwd_adv (NULL)")
    _ok(adv(*head, _ptr(dl), *outs("delta"), *tail), "icka_embed_fwd_adv")
    bf.check(what)
    for name in ("y", "twin", "xhat", "rstd"):
        _same(o["null"][name].view, o["plain"][name].view, "%s: %s with delta == NULL against icka_embed_fwd" % (what, name))
    rf = ac.fwd_adv_refs(lay, inp["word"], inp["pos"], inp["typ"], delta, inp["gamma"], inp["beta"], EPS_LN, inp["m"], tw)
    for name in ("y", "twin", "xhat", "rstd"):
        got = o["delta"][name].view
        kc.assert_within(got.reshape(-1) if name == "rstd" else got, rf[name][0], rf[name][1], "embed_fwd_adv " + name, verbose=False)
    assert not torch.equal(o["delta"]["y"].view, o["plain"]["y"].view), "the perturbation changed nothing"
    kc.report("embed_fwd_adv")


def test_embed_fwd_adv_refusals():
    lib, K, s = _env()
    z = torch.zeros(64, 8, dtype=F32, device="cuda")
    y = torch.zeros(4, 8, dtype=BF16, device="cuda")
    ids = torch.ones(4, dtype=I64, device="cuda")
    p = lambda t: t.data_ptr()
    args = (p(ids), None, p(z), p(z), p(z), p(z), p(z))
    assert lib.icka_embed_fwd_adv(*args, p(z) + 4, p(y), None, None, None, 2, 2, 8, 8, 2, EPS_LN, 0.0, 0, s) == E_ALIGN
    assert lib.icka_embed_fwd_adv(*args, p(z), p(y), None, None, None, 2, 2, 12, 8, 2, EPS_LN, 0.0, 0, s) == E_SHAPE
    assert lib.icka_embed_fwd_adv(*args, p(z), None, None, None, None, 2, 2, 8, 8, 2, EPS_LN, 0.0, 0, s) == E_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ ascent
def _ascend_case(lib, s, shape, alpha, from_zero, verbose=False):
    B, S, H = shape
    delta, grad, mask = ac.ascend_inputs(B, S, H, zero_sample=1 if B >= 4 else None, inf_sample=3 if B >= 4 else None)
    if from_zero:
        delta = torch.where((mask != 0)[:, :, None], torch.zeros_like(delta), delta)
    what = "adv_ascend %s alpha %g%s" % (shape, alpha, " from 0" if from_zero else "")
    nws = int(lib.icka_adv_workspace_floats(B, S, H))
    assert nws == 2 * B * ((S + 7) // 8)
    runs = []
    for rep in range(2):
        bf = Bufs()
        d = bf.out(B * S, H, F32, "delta", delta.reshape(B * S, H))
        g, m = bf.fin(grad.reshape(B * S, H), "grad"), bf.fin(mask.reshape(B * S, 1), "mask")
        norms, ws = bf.out(B, 2, F32, "norms"), bf.out(nws, 1, F32, "workspace")
        _ok(lib.icka_adv_ascend(_ptr(d), _ptr(g), _ptr(m), _ptr(norms), B, S, H, alpha, EPS, _ptr(ws), s), "icka_adv_ascend")
        bf.check(what)
        runs.append((d.view.reshape(B, S, H).cpu(), norms.view.cpu()))
    refs = ac.ascend_refs(delta, grad, mask, alpha, EPS)
    ac.compare_ascend(runs[0][0], runs[0][1], delta, refs, what, verbose=verbose)
    _same(runs[0][0], runs[1][0], what + ": delta of two runs")
    _same(runs[0][1], runs[1][1], what + ": norms of two runs")
    return refs, runs[0]


@pytest.mark.parametrize("shape", ac.ASCEND_SHAPES, ids=lambda t: "x".join(map(str, t)))
def test_adv_ascend(shape):
    lib, K, s = _env()
    small, large = float(np.float32(1e-3)), float(np.float32(5.0))
    refs, _ = _ascend_case(lib, s, shape, small, False)
    assert not bool(ao.ascend64(*ac.ascend_inputs(*shape, zero_sample=1 if shape[0] >= 4 else None,
                                                  inf_sample=3 if shape[0] >= 4 else None), small, EPS)["shrunk"].any())
    refs, (d, n) = _ascend_case(lib, s, shape, large, False)
    o = ao.ascend64(*ac.ascend_inputs(*shape, zero_sample=1 if shape[0] >= 4 else None, inf_sample=3 if shape[0] >= 4 else None),
                    large, EPS)
    assert bool(o["shrunk"][o["stepped"]].all()) and bool(o["stepped"].any())
    refs, (d, n) = _ascend_case(lib, s, shape, EPS, True)           # the FGM step: every sample that steps lands on the sphere
    st = refs["stepped"]
    assert bool(((n[st, 1].double() - EPS).abs() <= refs["norms"][1][st, 1]).all())
    kc.report("adv_ascend %s" % (shape,))


def test_adv_ascend_refusals():
    lib, K, s = _env()
    z = torch.zeros(4096, dtype=F32, device="cuda")
    m = torch.ones(64, dtype=I64, device="cuda")
    p = lambda t: t.data_ptr()
    assert lib.icka_adv_ascend(p(z), p(z), p(m), p(z), 2, 2, 12, 1.0, 1.0, p(z), s) == E_SHAPE           # H % 8
    assert lib.icka_adv_ascend(p(z), p(z), p(m), p(z), 1, 1, 2056, 1.0, 1.0, p(z), s) == E_SHAPE         # H > 2048
    assert lib.icka_adv_ascend(p(z), p(z), p(m), p(z), 1, 1025, 8, 1.0, 1.0, p(z), s) == E_SHAPE         # S > 1024
    assert lib.icka_adv_ascend(p(z) + 4, p(z), p(m), p(z), 2, 2, 8, 1.0, 1.0, p(z), s) == E_ALIGN
    assert lib.icka_adv_ascend(p(z), p(z), p(m), p(z), 2, 2, 8, 1.0, 1.0, None, s) == E_ARG
    assert lib.icka_adv_workspace_floats(1, 1025, 8) == 0 and lib.icka_adv_workspace_floats(2, 9, 8) == 8
    assert lib.icka_adv_init_uniform(p(z), p(m), 1, 1025, 8, 1.0, 0, None, s) == E_SHAPE
    assert lib.icka_adv_init_uniform(None, p(m), 2, 2, 8, 1.0, 0, None, s) == E_ARG
    assert lib.icka_adv_bump(None, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(z.ne(0).any())


# ------------------------------------------------------------------------------------------------ uniform start
@pytest.mark.parametrize("shape", [(3, 5, 72), (4, 37, 520), (2, 128, 768)], ids=lambda t: "x".join(map(str, t)))
def test_adv_init_uniform_is_bitwise_the_restatement(shape):
    lib, K, s = _env()
    B, S, H = shape
    junk, _, mask = ac.ascend_inputs(B, S, H)
    for seed in (0, (0x9E37 << 32) + 0xFFFFFFFE):
        for counter in (None, 0, 5):
            bf = Bufs()
            d = bf.out(B * S, H, F32, "delta", junk.reshape(B * S, H))
            m = bf.fin(mask.reshape(B * S, 1), "mask")
            cnt = None if counter is None else bf.out(1, 1, I64, "counter", torch.tensor([[counter]], dtype=I64))
            _ok(lib.icka_adv_init_uniform(_ptr(d), _ptr(m), B, S, H, EPS, seed, _ptr(cnt), s), "icka_adv_init_uniform")
            if cnt is not None:
                _ok(lib.icka_adv_bump(_ptr(cnt), s), "icka_adv_bump")
            bf.check("adv_init_uniform %s" % (shape,))
            want = ao.uniform_start_f32(mask, H, EPS, seed, counter or 0)
            _same(d.view.reshape(B, S, H), want, "adv_init_uniform %s seed %#x counter %s" % (shape, seed, counter))
            if cnt is not None:
                assert int(cnt.view.cpu()[0, 0]) == counter + 1, "the bump node advances the counter by 1"
