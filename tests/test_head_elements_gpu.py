"""GPU: every entry point of csrc/fusion.hip (per-sample gates, crs classifier, classifier head) and the contrastive kernels
of csrc/objective.hip element by element against float64 (tests/head_check.py: references and bounds derived from the number
formats), through the C ABI, at the smallest shapes at which each kernel's structure can go wrong.  Every operand sits in
NaN bands with NaN pad columns, every output in sentinel bands prefilled with NaN, and every buffer is checked after every
call.  Each case runs twice: natural strides and pointers, then padded row strides (ld + 8; ldv + 16) wherever the entry
point takes one and every pointer moved by 16 bytes; the two runs are bitwise equal for everything without float atomics.
tests/test_head_check_cpu.py keeps the bounds used here honest."""
import pytest
import torch

import head_check as hc
import kernel_check as kc
from head_check import BF16, F16, F32

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3          # include/icka_hip.h


def _env():
    from icka_amd import _lib
    from icka_amd import kernels as K
    return _lib.load(), K, K._stream()


def _ptr(g):
    return None if g is None else g.view.data_ptr()


def _ok(rc, name):
    assert rc == 0, "%s returned %d" % (name, rc)


class Bufs:
    """The guarded buffers of one call; ``check`` runs on all of them.  variant 0: natural strides and pointers; variant 1:
    ld = cols + ``pad`` where the caller says the ABI takes a stride, every pointer 16 bytes further into its allocation."""

    def __init__(self, variant):
        self.v, self.all = variant, []

    def _off(self, dtype):
        return self.v * (16 // torch.empty(0, dtype=dtype).element_size())

    def _keep(self, g, name):
        self.all.append((name, g))
        return g

    def fin(self, values, name, pad=0):
        """an operand [rows, cols] (1-D: one row) inside NaN bands and NaN pad columns"""
        values = values.reshape(1, -1) if values.dim() == 1 else values
        return self._keep(kc.Guarded(values.shape[0], values.shape[1], values.dtype, ld=values.shape[1] + pad * self.v,
                                     offset=self._off(values.dtype), fill=kc.NAN_FILL[values.dtype], init=values.cuda()), name)

    def out(self, rows, cols, dtype, name, pad=0, init=None):
        """an output inside sentinel bands, prefilled with NaN (or ``init``)"""
        return self._keep(kc.Guarded(rows, cols, dtype, ld=cols + pad * self.v, offset=self._off(dtype),
                                     init=None if init is None else init.reshape(rows, cols).cuda()), name)

    def flat(self, values, name):
        """a contiguous operand of n elements: an [n, 1] matrix with ld = 1 (bands of GUARD_ROWS elements)"""
        return self._keep(kc.Guarded(values.numel(), 1, values.dtype, ld=1, offset=self._off(values.dtype),
                                     fill=kc.NAN_FILL[values.dtype], init=values.reshape(-1, 1).cuda()), name)

    def flat_out(self, n, dtype, name, init=None):
        return self._keep(kc.Guarded(n, 1, dtype, ld=1, offset=self._off(dtype),
                                     init=None if init is None else init.reshape(-1, 1).cuda()), name)

    def check(self, what):
        torch.cuda.synchronize()
        for name, g in self.all:
            g.check(what="%s: %s (variant %d)" % (what, name, self.v))


def _cu(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _same(runs, names, what):
    """the two variants of a case gave the same bits"""
    for n in names:
        if runs[0].get(n) is not None:
            assert torch.equal(runs[0][n].contiguous().view(torch.int16 if runs[0][n].element_size() == 2 else torch.int32),
                               runs[1][n].contiguous().view(torch.int16 if runs[1][n].element_size() == 2 else torch.int32)), \
                "%s: %s differs between the stride variants" % (what, n)


# ---------------------------------------------------------------------------------------------------- sample gates
def _gate_case(lib, s, B, S, H, mode, with_c, with_dc, saturated=False, zero_prefill=False):
    a, c, d, gate, pre = hc.gate_inputs(B, S, H, mode, saturated)
    if zero_prefill:
        pre = torch.zeros_like(pre)
    if not with_c:
        c = None
    what = "sample_gate B=%d S=%d H=%d mode=%d c=%d dc=%d" % (B, S, H, mode, with_c, with_dc)
    ca, cc, cd, cg, cp = _cu(a, c, d, gate, pre)
    rf = hc.sample_gate_fwd_refs(ca, cc, cg, mode, B, S)
    rb = hc.sample_gate_bwd_refs(cd, ca, cc, cg, mode, B, S, cp, with_dc)
    runs = []
    for v in (0, 1):
        bf = Bufs(v)
        ga, gd, gg = bf.fin(a, "a", 8), bf.fin(d, "dout", 8), bf.flat(gate, "gate")
        gc = bf.fin(c, "c", 8) if with_c else None
        out, da = bf.out(B * S, H, BF16, "out", 8), bf.out(B * S, H, BF16, "da", 8)
        dc = bf.out(B * S, H, BF16, "dc", 8) if with_dc else None
        dg = bf.flat_out(pre.numel(), F32, "dgate", init=pre)
        _ok(lib.icka_sample_gate_fwd(_ptr(ga), ga.ld, _ptr(gc), gc.ld if gc else 0, _ptr(gg), mode, _ptr(out), out.ld, B, S, H, s),
            "icka_sample_gate_fwd")
        bf.check(what + " fwd")
        _ok(lib.icka_sample_gate_bwd(_ptr(gd), gd.ld, _ptr(ga), ga.ld, _ptr(gc), gc.ld if gc else 0, _ptr(gg), mode, _ptr(da), da.ld,
                                     _ptr(dc), dc.ld if dc else 0, _ptr(dg), B, S, H, s), "icka_sample_gate_bwd")
        bf.check(what + " bwd")
        o = {"out": out.view, "da": da.view, "dc": dc.view if dc else None, "dgate": dg.view.reshape(rb["dgate"][0].shape)}
        hc.compare(o, rf, "sample_gate_fwd")
        hc.compare(o, rb, "sample_gate_bwd")
        if mode == 1 and zero_prefill and S * (H // 8) <= 256:
            # one live block per sample: the words are -t and +t of one t (with more live blocks the atomics of the two
            # words may arrive in different orders)
            w = dg.view.reshape(B, 2)
            hc.same_bits(w[:, 0], -w[:, 1], what + " dgate[b, 0] == -dgate[b, 1]")
        runs.append(o)
    _same(runs, ("out", "da", "dc"), what)


@pytest.mark.parametrize("B,S,H", hc.GATE_SHAPES)
def test_sample_gate_fwd_bwd(B, S, H):
    lib, _K, s = _env()
    for with_c, with_dc in ((True, True), (False, False), (True, False)):
        _gate_case(lib, s, B, S, H, 0, with_c, with_dc)
    _gate_case(lib, s, B, S, H, 1, False, False)
    _gate_case(lib, s, B, S, H, 1, False, False, zero_prefill=True)
    _gate_case(lib, s, B, S, H, 0, True, True, saturated=True)
    _gate_case(lib, s, B, S, H, 1, False, False, saturated=True)
    kc.report("sample_gate B=%d S=%d H=%d" % (B, S, H))


@pytest.mark.parametrize("B,S,H", hc.GATE_SHAPES)
def test_sample_gate_fwd_h(B, S, H):
    lib, _K, s = _env()
    for mode in (0, 1):
        a, gate = hc.gate_h_inputs(B, S, H, mode)
        refs = hc.sample_gate_fwd_h_refs(a.cuda(), gate.cuda(), mode, B, S)
        runs = []
        for v in (0, 1):
            bf = Bufs(v)
            ga, gg = bf.fin(a, "a16", 8), bf.flat(gate, "gate")
            out, out16 = bf.out(B * S, H, BF16, "out", 8), bf.out(B * S, H, F16, "out16", 8)
            _ok(lib.icka_sample_gate_fwd_h(_ptr(ga), ga.ld, _ptr(gg), mode, _ptr(out), _ptr(out16), out.ld, B, S, H, s),
                "icka_sample_gate_fwd_h")
            bf.check("sample_gate_fwd_h")
            o = {"out": out.view, "out16": out16.view}
            hc.compare(o, refs, "sample_gate_fwd_h")
            # the planted +-65504 under a saturated gate stay finite, and out16 is not the bf16 value rounded again
            assert float(out16.view[0, 0]) == hc.FP16_MAX and float(out16.view[0, H - 1]) == -hc.FP16_MAX
            assert bool((out.view.to(F16) != out16.view).any()), "out16 equals fp16(bf16 out) everywhere"
            runs.append(o)
        _same(runs, ("out", "out16"), "sample_gate_fwd_h")
    kc.report("sample_gate_fwd_h B=%d S=%d H=%d" % (B, S, H))


# ------------------------------------------------------------------------------------------------- crs classifier
@pytest.mark.parametrize("B,S,H", hc.CRS_SHAPES)
def test_crs_fwd(B, S, H):
    lib, _K, s = _env()
    seq, cross, W, bias, pre, _d, _w, _b = hc.crs_inputs(B, S, H)
    for with_bias in (True, False):
        refs = hc.crs_fwd_refs(*_cu(seq, cross, W, bias if with_bias else None, pre), B, S, H)
        for v in (0, 1):
            bf = Bufs(v)
            gs, gc, gw = bf.fin(seq, "seq", 8), bf.fin(cross, "cross", 8), bf.flat(W, "W")
            gb = bf.flat(bias, "bias") if with_bias else None
            crs = bf.flat_out(2 * B, F32, "crs", init=pre)
            _ok(lib.icka_crs_fwd(_ptr(gs), gs.ld, _ptr(gc), gc.ld, _ptr(gw), _ptr(gb), _ptr(crs), B, S, H, s), "icka_crs_fwd")
            bf.check("crs_fwd")
            hc.compare({"crs": crs.view}, refs, "crs_fwd")
    kc.report("crs_fwd B=%d S=%d H=%d" % (B, S, H))


def _crs_bwd_case(lib, s, B, S, H, accumulate, with_db, inputs, refs):
    seq, cross, W, _bias, _pre, dcrs, dW0, db0 = inputs
    runs = []
    for v in (0, 1):
        bf = Bufs(v)
        gs, gc, gw = bf.fin(seq, "seq", 8), bf.fin(cross, "cross", 8), bf.flat(W, "W")
        gd = bf.flat(dcrs, "dcrs")
        dseq, dcross = bf.out(B * S, H, BF16, "dseq"), bf.out(B * S, H, BF16, "dcross")
        dW = bf.flat_out(2 * S * 2 * H, F32, "dW", init=dW0 if accumulate else None)
        db = bf.flat_out(2, F32, "dbias", init=db0 if accumulate else None) if with_db else None
        _ok(lib.icka_crs_bwd(_ptr(gd), _ptr(gs), gs.ld, _ptr(gc), gc.ld, _ptr(gw), _ptr(dseq), _ptr(dcross), _ptr(dW), _ptr(db),
                             B, S, H, accumulate, s), "icka_crs_bwd")
        bf.check("crs_bwd")
        o = {"dseq": dseq.view, "dcross": dcross.view, "dW": dW.view, "dbias": db.view if db else None}
        hc.compare(o, refs, "crs_bwd")
        runs.append(o)
    _same(runs, ("dseq", "dcross", "dW", "dbias"), "crs_bwd")


@pytest.mark.parametrize("B,S,H", hc.CRS_SHAPES)
def test_crs_bwd(B, S, H):
    lib, _K, s = _env()
    inputs = hc.crs_inputs(B, S, H)
    seq, cross, W, _bias, _pre, dcrs, dW0, db0 = _cu(*inputs)
    for accumulate in (0, 1):
        refs = hc.crs_bwd_refs(dcrs, seq, cross, W, B, S, H, accumulate, dW0, db0)
        _crs_bwd_case(lib, s, B, S, H, accumulate, True, inputs, refs)
        _crs_bwd_case(lib, s, B, S, H, accumulate, False, inputs, refs)
    kc.report("crs_bwd B=%d S=%d H=%d" % (B, S, H))


def test_crs_bwd_second_trip_of_the_capped_dgrad_grid():
    lib, _K, s = _env()
    B, S, H = hc.CRS_BIG
    assert hc.crs_dgrad_trips(B, S, H) == 2
    inputs = hc.crs_inputs(B, S, H)
    seq, cross, W, _bias, _pre, dcrs, dW0, db0 = _cu(*inputs)
    refs = hc.crs_bwd_refs(dcrs, seq, cross, W, B, S, H, 0, dW0, db0)
    _crs_bwd_case(lib, s, B, S, H, 0, True, inputs, refs)
    kc.report("crs_bwd B=%d S=%d H=%d" % (B, S, H))


# ------------------------------------------------------------------------------------------------ classifier head
def _cls_fwd_case(lib, s, M, H, C, dtype, with_bias):
    seq, gated, W, bias, _dl, _g, _c = hc.cls_inputs(M, H, C, dtype)
    refs = hc.cls_head_fwd_refs(*_cu(seq, gated, W, bias if with_bias else None))
    fn = lib.icka_cls_head_fwd_h if dtype == F16 else lib.icka_cls_head_fwd
    runs = []
    for v in (0, 1):
        bf = Bufs(v)
        gs, gg, gw = bf.fin(seq, "seq"), bf.fin(gated, "gated"), bf.fin(W, "W")
        gb = bf.flat(bias, "bias") if with_bias else None
        logits = bf.out(M, C, F32, "logits")
        _ok(fn(_ptr(gs), _ptr(gg), _ptr(gw), _ptr(gb), _ptr(logits), M, H, C, s), "icka_cls_head_fwd")
        bf.check("cls_head_fwd M=%d H=%d C=%d" % (M, H, C))          # exactly [M, C] written: the band starts at row M
        o = {"logits": logits.view}
        hc.compare(o, refs, "cls_head_fwd")
        runs.append(o)
    _same(runs, ("logits",), "cls_head_fwd")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_cls_head_fwd(dtype):
    lib, _K, s = _env()
    n = 0
    for H in hc.CLS_FWD_H:
        for C in hc.CLS_FWD_C:
            if not hc.cls_fwd_ok(H, C):
                continue
            for M in hc.CLS_FWD_M:
                _cls_fwd_case(lib, s, M, H, C, dtype, with_bias=(M != 2))
                n += 1
    assert n == 39
    M, H = hc.CLS_FWD_BIG
    assert hc.cls_fwd_trips(M) == 2 and M % 2 == 1
    _cls_fwd_case(lib, s, M, H, 13, dtype, True)
    kc.report("cls_head_fwd %s" % dtype)


def _cls_bwd_run(lib, s, M, H, C, ldd, v, inputs):
    seq, gated, W, _bias, dl, gate, cross = inputs
    bf = Bufs(v)
    gdl = bf._keep(kc.Guarded(M, C, BF16, ld=ldd, offset=bf._off(BF16), fill=kc.NAN_FILL[BF16], init=dl.cuda()), "dl")
    gs, gg, gt, gc, gw = bf.fin(seq, "seq"), bf.fin(gated, "gated"), bf.fin(gate, "gate"), bf.fin(cross, "cross"), bf.fin(W, "W")
    dseq, du, dcross = bf.out(M, H, BF16, "dseq"), bf.out(M, H, BF16, "du"), bf.out(M, H, BF16, "dcross")
    ns, sf = lib.icka_cls_head_bwd_slabs(M), lib.icka_cls_head_slab_floats(H, C)
    assert (ns, sf) == (hc.cls_slabs(M), hc.cls_slab_floats(H, C))
    part = bf.out(ns, sf, F32, "partials")
    _ok(lib.icka_cls_head_bwd(_ptr(gdl), ldd, _ptr(gs), _ptr(gg), _ptr(gt), _ptr(gc), _ptr(gw), _ptr(dseq), _ptr(du), _ptr(dcross),
                              _ptr(part), M, H, C, s), "icka_cls_head_bwd")
    bf.check("cls_head_bwd M=%d H=%d C=%d ldd=%d" % (M, H, C, ldd))      # nothing past the last slab
    return {"dseq": dseq.view, "du": du.view, "dcross": dcross.view, "slab_w": part.view[:, :C * 2 * H].reshape(ns, C, 2 * H),
            "slab_b": part.view[:, C * 2 * H:], "_part": part}


@pytest.mark.parametrize("H", hc.CLS_BWD_H)
def test_cls_head_bwd(H):
    lib, _K, s = _env()
    for M in hc.CLS_BWD_M:
        for C in hc.CLS_BWD_C:
            inputs = hc.cls_inputs(M, H, C)
            seq, gated, W, _bias, dl, gate, cross = _cu(*inputs)
            refs = hc.cls_head_bwd_refs(dl, seq, gated, gate, cross, W)
            for ldd in (C, C + 3):
                runs = []
                for v in (0, 1):
                    o = _cls_bwd_run(lib, s, M, H, C, ldd, v, inputs)
                    hc.compare(o, refs, "cls_head_bwd")
                    runs.append(o)
                _same(runs, ("dseq", "du", "dcross", "slab_w", "slab_b"), "cls_head_bwd")
    kc.report("cls_head_bwd H=%d" % H)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_cls_head_bwd_slabs_sum_to_the_weight_gradient(accumulate):
    """the wiring of icka_amd/ops.py: two slab reductions riding on one grouped launch"""
    lib, K, s = _env()
    M, H, C = 19, 24, 13
    inputs = hc.cls_inputs(M, H, C)
    seq, gated, W, _bias, dl, gate, cross = _cu(*inputs)
    refs = hc.cls_head_bwd_refs(dl, seq, gated, gate, cross, W)
    o = _cls_bwd_run(lib, s, M, H, C, C + 3, 0, inputs)
    ns, sf = hc.cls_slabs(M), hc.cls_slab_floats(H, C)
    ws = o["_part"].view.reshape(-1)
    assert ws.is_contiguous() and ws.numel() == ns * sf
    dW0, db0 = hc.rnd(C, 2 * H, seed=31).cuda(), hc.rnd(C, seed=32).cuda()
    dW, db = (dW0.clone(), db0.clone()) if accumulate else (torch.full_like(dW0, float("nan")), torch.full_like(db0, float("nan")))
    K.gemm_grouped([], reductions=[K.slab_reduction(ws, ns, C * 2 * H, (dW.view(-1),), bool(accumulate), slab_stride=sf),
                                   K.slab_reduction(ws, ns, C, (db,), bool(accumulate), slab_stride=sf, offset=C * 2 * H)])
    torch.cuda.synchronize()
    hc.compare({"dW": dW, "db": db}, hc.cls_wiring_refs(refs, accumulate, dW0, db0), "cls_head_bwd wiring")
    kc.report("cls_head_bwd wiring accumulate=%d" % accumulate)


# ---------------------------------------------------------------------------------------------------- contrastive
def _cl_case(lib, s, dtype, B, D, temp, tl, n_neg, tie=False):
    t, v, crs = hc.cl_inputs(B, D, dtype, tie)
    with_crs = n_neg is not None
    nn = n_neg if with_crs else 0
    dcl, dcrs_loss = 0.75, -1.25
    refs = hc.contrastive_refs(t.cuda(), v.cuda(), temp, tl, crs.cuda() if with_crs else None, nn, dcl, dcrs_loss)
    what = "contrastive B=%d D=%d temp=%g tl=%g n_neg=%s" % (B, D, temp, tl, n_neg)
    code = {F32: 0, BF16: 1, F16: 2}[dtype]
    nws = lib.icka_contrastive_workspace_floats(B)
    assert nws == hc.contrastive_ws_floats(B)
    runs = []
    for var in (0, 1):
        bf = Bufs(var)
        gt, gv = bf.fin(t, "t", 8), bf.fin(v, "v", 16)
        gc = bf.flat(crs, "crs") if with_crs else None
        g1, g2 = bf.flat(torch.tensor([dcl]), "dcl"), bf.flat(torch.tensor([dcrs_loss]), "dcrs_loss")
        stats, ws = bf.flat_out(2, F32, "stats"), bf.flat_out(nws, F32, "ws")
        dt, dv = bf.out(B, D, F32, "dt"), bf.out(B, D, F32, "dv")
        dcrs = bf.flat_out(2 * B, F32, "dcrs") if with_crs else None
        _ok(lib.icka_contrastive_fwd(_ptr(gt), gt.ld, _ptr(gv), gv.ld, code, B, D, temp, tl, _ptr(gc), nn, _ptr(stats), _ptr(ws), s),
            "icka_contrastive_fwd")
        bf.check(what + " fwd")                                               # ws: exactly B B + 6 B floats written
        _ok(lib.icka_contrastive_bwd(_ptr(gt), gt.ld, _ptr(gv), gv.ld, code, B, D, temp, tl, _ptr(ws), _ptr(g1), _ptr(g2), _ptr(dt),
                                     _ptr(dv), _ptr(gc), nn, _ptr(dcrs), s), "icka_contrastive_bwd")
        bf.check(what + " bwd")                                               # dt, dv untouched past [B, D]
        o = {"stats": stats.view.reshape(2), "ws": ws.view.reshape(-1), "dt": dt.view, "dv": dv.view,
             "dcrs": dcrs.view if with_crs else None}
        hc.compare(o, refs, "contrastive")
        if not with_crs:
            assert float(stats.view[1, 0]) == 0.0
        if B == 1:
            assert float(stats.view[0, 0]) == 0.0 and float(dt.view.abs().max()) == 0.0 and float(dv.view.abs().max()) == 0.0
        runs.append(o)
    _same(runs, ("stats", "ws", "dt", "dv", "dcrs"), what)


@pytest.mark.parametrize("dtype", hc.CL_DTYPES, ids=["f32", "bf16", "fp16"])
def test_contrastive_fwd_bwd(dtype):
    lib, _K, s = _env()
    for B, D, temp, tl, n_neg in hc.cl_cases():
        _cl_case(lib, s, dtype, B, D, temp, tl, n_neg)
    for B in (2, 33):                      # two identical rows: a tie for the row and the column maximum
        _cl_case(lib, s, dtype, B, hc.cl_D(B)[1], 0.05, 0.7, 1, tie=True)
        _cl_case(lib, s, dtype, B, 8, 1.0, 0.7, B, tie=True)
    kc.report("contrastive %s" % dtype)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_buffer_untouched():
    lib, K, s = _env()
    bf = Bufs(0)
    x = bf.out(64, 2080, BF16, "bf16 scratch")          # every 16-bit operand and output of the refused calls
    f = bf.out(64, 2080, F32, "f32 scratch")
    x0, f0 = x.flat.view(torch.int16).clone(), f.flat.view(torch.int32).clone()
    p, q = x.view.data_ptr(), f.view.data_ptr()
    calls = {
        "sample_gate_fwd H % 8": (lib.icka_sample_gate_fwd(p, 16, p, 16, q, 0, p, 16, 1, 2, 12, s), E_SHAPE),
        "sample_gate_fwd ld % 8": (lib.icka_sample_gate_fwd(p, 20, p, 16, q, 0, p, 16, 1, 2, 16, s), E_ALIGN),
        "sample_gate_fwd pointer off 16 bytes": (lib.icka_sample_gate_fwd(p + 2, 16, p, 16, q, 0, p, 16, 1, 2, 16, s), E_ALIGN),
        "sample_gate_fwd mode 2": (lib.icka_sample_gate_fwd(p, 16, p, 16, q, 2, p, 16, 1, 2, 16, s), E_ARG),
        "sample_gate_fwd_h H % 8": (lib.icka_sample_gate_fwd_h(p, 16, q, 1, p, p, 16, 1, 2, 12, s), E_SHAPE),
        "sample_gate_fwd_h mode 2": (lib.icka_sample_gate_fwd_h(p, 16, q, 2, p, p, 16, 1, 2, 16, s), E_SHAPE),
        "sample_gate_fwd_h ldo % 8": (lib.icka_sample_gate_fwd_h(p, 16, q, 1, p, p, 20, 1, 2, 16, s), E_ALIGN),
        "sample_gate_bwd mode 2": (lib.icka_sample_gate_bwd(p, 16, p, 16, p, 16, q, 2, p, 16, p, 16, q, 1, 2, 16, s), E_ARG),
        "sample_gate_bwd H % 8": (lib.icka_sample_gate_bwd(p, 16, p, 16, p, 16, q, 0, p, 16, p, 16, q, 1, 2, 12, s), E_SHAPE),
        "sample_gate_bwd dc off 16 bytes": (lib.icka_sample_gate_bwd(p, 16, p, 16, p, 16, q, 0, p, 16, p + 2, 16, q, 1, 2, 16, s), E_ALIGN),
        "crs_fwd H % 8": (lib.icka_crs_fwd(p, 16, p, 16, p, q, q, 1, 2, 12, s), E_SHAPE),
        "crs_fwd lds % 8": (lib.icka_crs_fwd(p, 20, p, 16, p, q, q, 1, 2, 16, s), E_ALIGN),
        "crs_fwd W off 16 bytes": (lib.icka_crs_fwd(p, 16, p, 16, p + 2, q, q, 1, 2, 16, s), E_ALIGN),
        "crs_bwd H % 8": (lib.icka_crs_bwd(q, p, 16, p, 16, p, p, p, q, q, 1, 2, 12, 0, s), E_SHAPE),
        "crs_bwd dseq off 16 bytes": (lib.icka_crs_bwd(q, p, 16, p, 16, p, p + 2, p, q, q, 1, 2, 16, 0, s), E_ALIGN),
        "cls_head_fwd C = 17": (lib.icka_cls_head_fwd(p, p, p, q, q, 2, 16, 17, s), E_SHAPE),
        "cls_head_fwd H % 8": (lib.icka_cls_head_fwd(p, p, p, q, q, 2, 12, 2, s), E_SHAPE),
        "cls_head_fwd 2H/8 > 256": (lib.icka_cls_head_fwd(p, p, p, q, q, 9, 1032, 2, s), E_SHAPE),
        "cls_head_fwd_h 2H/8 > 256": (lib.icka_cls_head_fwd_h(p, p, p, q, q, 9, 1032, 2, s), E_SHAPE),
        "cls_head_fwd W off 16 bytes": (lib.icka_cls_head_fwd(p, p, p + 2, q, q, 2, 16, 2, s), E_ALIGN),
        "cls_head_bwd C = 17": (lib.icka_cls_head_bwd(p, 24, p, p, p, p, p, p, p, p, q, 2, 16, 17, s), E_SHAPE),
        "cls_head_bwd ldd < C": (lib.icka_cls_head_bwd(p, 12, p, p, p, p, p, p, p, p, q, 2, 16, 13, s), E_SHAPE),
        "cls_head_bwd 2H/8 > 256": (lib.icka_cls_head_bwd(p, 2, p, p, p, p, p, p, p, p, q, 2, 1032, 2, s), E_SHAPE),
        "cls_head_bwd du off 16 bytes": (lib.icka_cls_head_bwd(p, 2, p, p, p, p, p, p, p + 2, p, q, 2, 16, 2, s), E_ALIGN),
        "contrastive_fwd n_neg > B": (lib.icka_contrastive_fwd(q, 16, q, 16, 0, 4, 16, 0.05, 0.7, q, 5, q, q, s), E_SHAPE),
        "contrastive_fwd ldt < D": (lib.icka_contrastive_fwd(q, 8, q, 16, 0, 4, 16, 0.05, 0.7, None, 0, q, q, s), E_SHAPE),
        "contrastive_fwd dtype 3": (lib.icka_contrastive_fwd(q, 16, q, 16, 3, 4, 16, 0.05, 0.7, None, 0, q, q, s), E_ARG),
        "contrastive_bwd n_neg > B": (lib.icka_contrastive_bwd(q, 16, q, 16, 0, 4, 16, 0.05, 0.7, q, q, q, q, q, q, 5, q, s), E_SHAPE),
        "contrastive_bwd ldv < D": (lib.icka_contrastive_bwd(q, 16, q, 8, 0, 4, 16, 0.05, 0.7, q, q, q, q, q, None, 0, None, s), E_SHAPE),
        "contrastive_bwd dtype 3": (lib.icka_contrastive_bwd(q, 16, q, 16, 3, 4, 16, 0.05, 0.7, q, q, q, q, q, None, 0, None, s), E_ARG),
        "contrastive_bwd crs without dcrs": (lib.icka_contrastive_bwd(q, 16, q, 16, 0, 4, 16, 0.05, 0.7, q, q, q, q, q, q, 1, None, s), E_ARG),
    }
    torch.cuda.synchronize()
    for name, (rc, want) in calls.items():
        assert rc == want, "%s returned %d, not %d" % (name, rc, want)
    assert torch.equal(x.flat.view(torch.int16), x0) and torch.equal(f.flat.view(torch.int32), f0)
    # the forward of the classifier head left the last gated columns of H > 1024 out of every logit (C = 2, H = 1032 passed its
    # 44 KiB check and returned 0): both forms refuse it now, and so does the wrapper, before any launch
    for dtype in (BF16, F16):
        seq, gated, W, bias, _dl, _g, _c = _cu(*hc.cls_inputs(9, 1032, 2, dtype))
        logits = torch.full((9, 2), float("nan"), device="cuda")
        with pytest.raises(ValueError, match="2H/8 <= 256"):
            K.cls_head_fwd(seq, gated, W, bias, logits)
        assert bool(torch.isnan(logits).all())
    kc.report("refusals")
