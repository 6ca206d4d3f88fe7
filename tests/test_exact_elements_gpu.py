"""GPU: every entry point of the fp32-exact mode (csrc/exact.hip, icka_x_*) element by element against float64
(tests/exact_check.py: references and bounds derived from the number formats), through the C ABI, at the smallest shapes at
which each kernel's structure can go wrong: lane-stride tails, a partial block of 4 rows, a second grid-stride trip, every
stride the ABI takes.  Every operand sits in NaN bands with NaN pad columns, every output in sentinel bands prefilled with
NaN, and every buffer is checked after every call.  Each case runs twice: natural strides and aligned pointers, then padded
strides (ld = cols + 3 wherever the ABI takes one) with every f32 pointer one element off its alignment.
tests/test_exact_gpu.py stays the check of the composed blocks against ATen; tests/test_exact_check_cpu.py keeps the
bounds used here honest."""
import ctypes as C

import pytest
import torch

import exact_check as xc
import kernel_check as kc
from exact_check import F32

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9abc
I32, I64 = torch.int32, torch.int64
E_SHAPE, E_ARG = -1, -3          # ICKA_E_SHAPE, ICKA_E_ARG (include/icka_hip.h)
NAN = float("nan")


def _env():
    from icka_amd import _lib
    from icka_amd import kernels as K
    K.set_dropout_nonce(None)
    return _lib.load(), K, K._stream()


def _ptr(g):
    return None if g is None else g.view.data_ptr()


class Bufs:
    """The guarded buffers of one case; ``check`` runs on all of them.  variant 0: natural strides, aligned pointers;
    variant 1: ld = cols + 3 where the caller says the ABI takes a stride, every f32 buffer one element off its alignment."""

    def __init__(self, variant):
        self.v, self.all = variant, []

    def _keep(self, g, name):
        self.all.append((name, g))
        return g

    def fin(self, values, name, ld=False, ld_natural=None):
        """an f32 operand [rows, cols] (1-D: one row) inside NaN bands and NaN pad columns"""
        values = values.reshape(1, -1) if values.dim() == 1 else values.reshape(values.shape[0], -1)
        cols = values.shape[1]
        nat = cols if ld_natural is None else ld_natural
        return self._keep(kc.Guarded(values.shape[0], cols, F32, ld=nat + 3 if (ld and self.v) else nat, offset=self.v,
                                     fill=kc.NAN_FILL[F32], init=values.to(F32).cuda()), name)

    def flat(self, values, name):
        """a contiguous f32 operand of n elements: a [n, 1] matrix with ld = 1 (bands of GUARD_ROWS elements)"""
        return self._keep(kc.Guarded(values.numel(), 1, F32, ld=1, offset=self.v, fill=kc.NAN_FILL[F32],
                                     init=values.reshape(-1, 1).cuda()), name)

    def ints(self, values, name, dtype=I64):
        return self._keep(kc.Guarded(1, values.numel(), dtype, init=values.reshape(1, -1).cuda()), name)

    def out(self, rows, cols, name, ld=False, init=None):
        """an f32 output inside sentinel bands, prefilled with NaN (or ``init``)"""
        return self._keep(kc.Guarded(rows, cols, F32, ld=cols + 3 if (ld and self.v) else cols, offset=self.v, init=init), name)

    def flat_out(self, n, name):
        return self._keep(kc.Guarded(n, 1, F32, ld=1, offset=self.v), name)

    def check(self, what):
        torch.cuda.synchronize()
        for name, g in self.all:
            g.check(what="%s: %s (variant %d)" % (what, name, self.v))


def _ok(rc, name):
    assert rc == 0, "%s returned %d" % (name, rc)


def _bits(g):
    return g.flat.view(kc._INT[g.dtype]).clone()


def _cu(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


# ------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_case(lib, K, s, M, H, p, v, bare=False, mean100=False):
    x0, r0, gamma0, beta0, dy0, z = xc.ln_inputs(M, H, mean100)
    with_res = not (bare or mean100)
    b = Bufs(v)
    x, res = b.fin(x0, "x", ld=True), (b.fin(r0, "residual", ld=True) if with_res else None)
    gamma, beta = b.fin(gamma0, "gamma"), b.fin(beta0, "beta")
    y = b.out(M, H, "y")
    xhat, rstd = (None, None) if bare else (b.out(M, H, "xhat"), b.out(1, M, "rstd"))
    _ok(lib.icka_x_ln_fwd(_ptr(x), x.ld, _ptr(res), res.ld if with_res else 0, _ptr(gamma), _ptr(beta), _ptr(y), _ptr(xhat),
                          _ptr(rstd), M, H, xc.EPS_LN, p, SEED, s), "icka_x_ln_fwd")
    b.check("ln_fwd")
    m = K.dropout_mask(M * H, p, SEED, "cuda").view(M, H) if p > 0 else torch.ones(M, H, device="cuda")
    refs = xc.ln_fwd_refs(x.view, m, res.view if with_res else None, gamma.view[0], beta.view[0], xc.EPS_LN)
    tag = "ln_fwd mean-100" if mean100 else "ln_fwd"
    xc.compare({"y": y.view, "xhat": None if bare else xhat.view, "rstd": None if bare else rstd.view[0]}, refs, tag)
    if z is not None:
        xc.same_bits(y.view[z], beta0, "all-zero row: y == beta")
    if bare:
        return
    dy = b.fin(dy0, "dy", ld=True)
    dpre, dd = b.out(M, H, "dpre"), (b.out(M, H, "ddense") if (p > 0 or v) else None)
    _ok(lib.icka_x_ln_bwd(_ptr(dy), dy.ld, _ptr(xhat), _ptr(rstd), _ptr(gamma), _ptr(dpre), _ptr(dd), M, H, p, SEED, s),
        "icka_x_ln_bwd")
    b.check("ln_bwd")
    refs = xc.ln_bwd_refs(dy.view, xhat.view, rstd.view[0], gamma.view[0], m)
    xc.compare({"dpre": dpre.view, "ddense": None if dd is None else dd.view}, refs, "ln_bwd mean-100" if mean100 else "ln_bwd")


@pytest.mark.parametrize("H", xc.ROW_H)
def test_ln_fwd_bwd(H):
    lib, K, s = _env()
    for M in xc.LN_M:
        for p in xc.P_DROP:
            for v in (0, 1):
                _ln_case(lib, K, s, M, H, p, v)
        _ln_case(lib, K, s, M, H, 0.1, 1, bare=True)          # residual, xhat and rstd NULL
    xc.report("x_ln H=%d" % H)


def test_ln_rows_of_mean_100():
    lib, K, s = _env()
    for v in (0, 1):
        _ln_case(lib, K, s, 5, 200, 0.0, v, mean100=True)
    xc.report("x_ln mean-100")


# ------------------------------------------------------------------------------------------------------ column sum
@pytest.mark.parametrize("M", xc.COLSUM_M)
def test_colsum(M):
    lib, K, s = _env()
    for N in xc.COLSUM_N:
        for with_b in (False, True):
            for acc in (0, 1):
                for v in (0, 1):
                    bf = Bufs(v)
                    a = bf.fin(xc.rnd(M, N, seed=1), "a", ld=True)
                    b = bf.fin(xc.rnd(M, N, seed=2), "b", ld=True) if with_b else None
                    out = bf.out(1, N, "out", init=0.5)
                    _ok(lib.icka_x_colsum(_ptr(a), a.ld, _ptr(b), b.ld if with_b else 0, _ptr(out), M, N, acc, s), "icka_x_colsum")
                    bf.check("colsum")
                    refs = xc.colsum_refs(a.view, b.view if with_b else None, acc, torch.full((N,), 0.5, device="cuda"))
                    xc.compare({"out": out.view[0]}, refs, "colsum")
    xc.report("x_colsum M=%d" % M)


# ------------------------------------------------------------------------------------------------------ embeddings
def _tables(H, vocab, types, max_pos):
    return xc.rnd(vocab, H, seed=21), xc.rnd(max_pos, H, seed=22), xc.rnd(types, H, seed=23)


def _padding_row_untouched(g, padding_idx, H, what):
    xc.same_bits(g.view[padding_idx], torch.full((H,), 0.5), what + ": padding row")


@pytest.mark.parametrize("H", xc.ROW_H)
def test_embed_fwd_scatter(H):
    lib, K, s = _env()
    e = xc.EMBED
    B, S = e["B"], e["S"]
    ids0 = xc.embed_ids(B, S, e["vocab"])
    word0, pos0, typ0 = _tables(H, e["vocab"], e["types"], e["max_pos"])
    gamma0, beta0, dpre0 = xc.rnd(H, seed=4) + 1.0, xc.rnd(H, seed=5), xc.rnd(B * S, H, seed=6)
    sizes = (e["vocab"], e["max_pos"], e["types"])
    for with_tt in (False, True):
        tt0 = (torch.arange(B * S).reshape(B, S) % 2) if with_tt else None
        for v in (0, 1):
            b = Bufs(v)
            ids, tt = b.ints(ids0, "ids"), (b.ints(tt0, "token_type") if with_tt else None)
            word, pos, typ = b.fin(word0, "word"), b.fin(pos0, "pos"), b.fin(typ0, "type")
            gamma, beta = b.fin(gamma0, "gamma"), b.fin(beta0, "beta")
            y = b.out(B * S, H, "y")
            save = with_tt or not v                     # one combination runs with xhat and rstd NULL
            xhat, rstd = (b.out(B * S, H, "xhat"), b.out(1, B * S, "rstd")) if save else (None, None)
            _ok(lib.icka_x_embed_fwd(_ptr(ids), _ptr(tt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta), _ptr(y),
                                     _ptr(xhat), _ptr(rstd), B, S, H, xc.EPS_LN, s), "icka_x_embed_fwd")
            b.check("embed_fwd")
            ids_c, tt_c = _cu(ids0, tt0)
            refs = xc.embed_fwd_refs(ids_c, tt_c, word.view, pos.view, typ.view, gamma.view[0], beta.view[0], S, xc.EPS_LN)
            xc.compare({"y": y.view, "xhat": xhat.view if save else None, "rstd": rstd.view[0] if save else None}, refs, "embed_fwd")
            dpre = b.fin(dpre0, "dpre")
            tabs = [b.out(n, H, name, init=0.5) for n, name in zip(sizes, ("dword", "dpos", "dtyp"))]
            _ok(lib.icka_x_embed_scatter(_ptr(dpre), _ptr(ids), _ptr(tt), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), B, S, H,
                                         e["padding_idx"], s), "icka_x_embed_scatter")
            b.check("embed_scatter")
            refs = xc.embed_scatter_refs(dpre.view, ids_c, tt_c, S, sizes, e["padding_idx"], 0.5)
            xc.compare({"dword": tabs[0].view, "dpos": tabs[1].view, "dtyp": tabs[2].view}, refs, "embed_scatter")
            _padding_row_untouched(tabs[0], e["padding_idx"], H, "embed_scatter")
    xc.report("x_embed H=%d" % H)


@pytest.mark.parametrize("H", xc.ROW_H)
def test_embed_prompt_fwd_scatter(H):
    lib, K, s = _env()
    c = xc.PROMPT
    B, S_in, S, P = c["B"], c["S_in"], c["S"], c["P"]
    ids0 = xc.embed_ids(B, S_in, c["vocab"])
    src0 = torch.tensor(c["src"], dtype=I32)
    word0, pos0, typ0 = _tables(H, c["vocab"], 2, c["max_pos"])
    prompt0 = xc.rnd(B, P, H, seed=24)
    gamma0, beta0, dpre0 = xc.rnd(H, seed=4) + 1.0, xc.rnd(H, seed=5), xc.rnd(B * S, H, seed=6)
    sizes = (c["vocab"], c["max_pos"], 2)
    for off in c["pos_offsets"]:
        for v in (0, 1):
            b = Bufs(v)
            ids, src = b.ints(ids0, "ids"), b.ints(src0, "src", I32)
            prompt = b.fin(prompt0.reshape(B * P, H), "prompt")
            word, pos, typ = b.fin(word0, "word"), b.fin(pos0, "pos"), b.fin(typ0, "type")
            gamma, beta = b.fin(gamma0, "gamma"), b.fin(beta0, "beta")
            y, xhat, rstd = b.out(B * S, H, "y"), b.out(B * S, H, "xhat"), b.out(1, B * S, "rstd")
            _ok(lib.icka_x_embed_prompt_fwd(_ptr(ids), _ptr(src), _ptr(prompt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma),
                                            _ptr(beta), _ptr(y), _ptr(xhat), _ptr(rstd), B, S_in, S, P, H, off, xc.EPS_LN, s),
                "icka_x_embed_prompt_fwd")
            b.check("prompt_fwd")
            ids_c, src_c = _cu(ids0, src0)
            refs = xc.prompt_fwd_refs(ids_c, src_c, prompt.view, word.view, pos.view, typ.view, gamma.view[0], beta.view[0],
                                      B, S_in, S, P, off, xc.EPS_LN)
            xc.compare({"y": y.view, "xhat": xhat.view, "rstd": rstd.view[0]}, refs, "prompt_fwd")
            dpre = b.fin(dpre0, "dpre")
            tabs = [b.out(n, H, name, init=0.5) for n, name in zip(sizes, ("dword", "dpos", "dtyp"))]
            dprompt = b.out(B * P, H, "dprompt")
            _ok(lib.icka_x_embed_prompt_scatter(_ptr(dpre), _ptr(ids), _ptr(src), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]),
                                                _ptr(dprompt), B, S_in, S, P, H, off, c["padding_idx"], s),
                "icka_x_embed_prompt_scatter")
            b.check("prompt_scatter")
            refs = xc.prompt_scatter_refs(dpre.view, ids_c, src_c, B, S_in, S, P, off, sizes, c["padding_idx"], 0.5)
            xc.compare({"dword": tabs[0].view, "dpos": tabs[1].view, "dtyp": tabs[2].view}, refs, "prompt_scatter")
            assert bool((refs["dprompt_source"] >= 0).all())
            xc.same_bits(dprompt.view, dpre0[refs["dprompt_source"].cpu()], "dprompt rows")
            _padding_row_untouched(tabs[0], c["padding_idx"], H, "prompt_scatter")
    xc.report("x_embed_prompt H=%d" % H)


# --------------------------------------------------------------------------------------------------------- softmax
def _softmax_case(lib, K, s, Skv, scale, p, kind, v, pd_given=True):
    c = xc.SOFTMAX
    B, heads, Sq = c["B"], c["heads"], c["Sq"]
    rows = B * heads * Sq
    b = Bufs(v)
    P0 = xc.rnd(rows, Skv, seed=1, scale=2.0)
    P = b.out(rows, Skv, "P", init=P0.cuda())                       # in place
    mask = b.fin(xc.softmax_mask(Skv, kind), "mask")
    Pd = b.out(rows, Skv, "Pd") if pd_given else None
    before = _bits(Pd) if pd_given else None
    _ok(lib.icka_x_softmax_fwd(_ptr(P), _ptr(Pd), _ptr(mask), B, heads, Sq, Skv, scale, p, SEED, s), "icka_x_softmax_fwd")
    b.check("softmax_fwd")
    m = K.attn_dropout_mask(rows, Skv, p, SEED, "cuda") if p > 0 else torch.ones(rows, Skv, device="cuda")
    refs = xc.softmax_fwd_refs(P0.cuda(), mask.view, m, scale, heads * Sq)
    xc.compare({"P": P.view, "Pd": Pd.view if (p > 0) else None}, refs, "softmax_fwd" + (" all-masked" if kind == "all" else ""))
    if pd_given and p == 0:
        assert torch.equal(before, _bits(Pd)), "Pd was written although p_drop == 0"
    saved = _bits(P)
    dPd0 = xc.rnd(rows, Skv, seed=3)
    dS = b.out(rows, Skv, "dS", init=dPd0.cuda())                   # in place
    _ok(lib.icka_x_softmax_bwd(_ptr(P), _ptr(dS), B, heads, Sq, Skv, scale, p, SEED, s), "icka_x_softmax_bwd")
    b.check("softmax_bwd")
    assert torch.equal(saved, _bits(P)), "softmax_bwd wrote its saved P"
    xc.compare({"dS": dS.view}, xc.softmax_bwd_refs(P.view, dPd0.cuda(), m, scale), "softmax_bwd")


@pytest.mark.parametrize("Skv", xc.SOFTMAX["Skv"])
def test_softmax_fwd_bwd(Skv):
    lib, K, s = _env()
    for v in (0, 1):
        for scale in xc.SOFTMAX["scales"]:
            for p in xc.P_DROP:
                _softmax_case(lib, K, s, Skv, scale, p, "tail", v)
        _softmax_case(lib, K, s, Skv, 1.0, 0.1, "all", v)
    _softmax_case(lib, K, s, Skv, 0.125, 0.0, "tail", 1, pd_given=False)
    xc.report("x_softmax Skv=%d" % Skv)


# ---------------------------------------------------------------------------------------------------- flat kernels
@pytest.mark.parametrize("n", xc.FLAT_N)
def test_act_dropout_scale_by_ratio(n):
    lib, K, s = _env()
    x0 = xc.uniform(n, seed=1, planted=xc.PLANTED)
    aux0, dy0 = xc.rnd(n, seed=2), xc.rnd(n, seed=3)
    for v in (0, 1):
        for mode in (0, 1, 2):
            b = Bufs(v)
            x, aux, dy = b.flat(x0, "x"), (b.flat(aux0, "aux") if mode == 2 else None), b.flat(dy0, "dy")
            y, y2 = b.flat_out(n, "y"), (b.flat_out(n, "y2") if mode == 2 else None)
            _ok(lib.icka_x_act_fwd(_ptr(x), _ptr(aux), _ptr(y), _ptr(y2), n, mode, s), "icka_x_act_fwd")
            b.check("act_fwd")
            refs = xc.act_fwd_refs(mode, x.view, aux.view if mode == 2 else None)
            xc.compare({"y": y.view, "y2": y2.view if mode == 2 else None}, refs, "act_fwd mode %d" % mode)
            saved = (x, y, y2)[mode]
            dx, dx2 = b.flat_out(n, "dx"), (b.flat_out(n, "dx2") if mode == 2 else None)
            _ok(lib.icka_x_act_bwd(_ptr(dy), _ptr(saved), _ptr(aux), _ptr(dx), _ptr(dx2), n, mode, s), "icka_x_act_bwd")
            b.check("act_bwd")
            refs = xc.act_bwd_refs(mode, dy.view, saved.view, aux.view if mode == 2 else None)
            xc.compare({"dx": dx.view, "dx2": dx2.view if mode == 2 else None}, refs, "act_bwd mode %d" % mode)
        b = Bufs(v)
        x, y = b.flat(x0, "x"), b.flat_out(n, "y")
        _ok(lib.icka_x_dropout(_ptr(x), _ptr(y), n, 0.1, SEED, s), "icka_x_dropout")
        b.check("dropout")
        xc.compare({"y": y.view}, xc.mul_refs(x.view, K.dropout_mask(n, 0.1, SEED, "cuda")[:, None]), "dropout")
        for num0, den0 in ((None, None), (3.0, 7.0), (3.0, 0.0), (None, 5.0), (0.25, None)) if n < 1000 else ((3.0, 7.0),):
            b = Bufs(v)
            x, y = b.flat(x0, "x"), b.flat_out(n, "y")
            num = None if num0 is None else b.fin(torch.tensor([num0]), "num")
            den = None if den0 is None else b.fin(torch.tensor([den0]), "den")
            _ok(lib.icka_x_scale_by_ratio(_ptr(x), _ptr(y), _ptr(num), _ptr(den), n, s), "icka_x_scale_by_ratio")
            b.check("scale_by_ratio")
            xc.compare({"y": y.view}, xc.scale_ratio_refs(x.view, num0, den0), "scale_by_ratio")
    xc.report("x flat n=%d" % n)


# ---------------------------------------------------------------------------------------------- strided 2-D kernels
def test_add_concat_regions():
    lib, K, s = _env()
    for v in (0, 1):
        for M, N in xc.ADD_MN:
            bf = Bufs(v)
            a, b = bf.fin(xc.rnd(M, N, seed=1), "a", ld=True), bf.fin(xc.rnd(M, N, seed=2), "b", ld=True)
            out = bf.out(M, N, "out", ld=True)
            _ok(lib.icka_x_add(_ptr(a), a.ld, _ptr(b), b.ld, _ptr(out), out.ld, M, N, s), "icka_x_add")
            bf.check("add")
            xc.compare({"out": out.view}, xc.add_refs(a.view, b.view), "add")
        for M, Ha, Hb in xc.CONCAT:                          # every element carries its own index
            bf = Bufs(v)
            a0 = torch.arange(M * Ha, dtype=F32).reshape(M, Ha)
            b0 = torch.arange(M * Hb, dtype=F32).reshape(M, Hb) + 100000.0
            a, b, out = bf.fin(a0, "a", ld=True), bf.fin(b0, "b", ld=True), bf.out(M, Ha + Hb, "out")
            _ok(lib.icka_x_concat2(_ptr(a), a.ld, Ha, _ptr(b), b.ld, Hb, _ptr(out), M, s), "icka_x_concat2")
            bf.check("concat2")
            xc.same_bits(out.view, torch.cat([a0, b0], 1), "concat2")
        for B, R, Cc in xc.REGIONS:
            for layout in (0, 1):
                bf = Bufs(v)
                src0 = torch.arange(B * R * Cc, dtype=F32)
                src, dst = bf.flat(src0, "src"), bf.out(B * R, Cc, "dst")
                _ok(lib.icka_x_regions_to_tokens(_ptr(src), _ptr(dst), B, R, Cc, layout, s), "icka_x_regions_to_tokens")
                bf.check("regions_to_tokens")
                want = src0.reshape(B, Cc, R).transpose(1, 2).reshape(B * R, Cc) if layout else src0.reshape(B * R, Cc)
                xc.same_bits(dst.view, want, "regions_to_tokens layout %d" % layout)
    xc.report("x add / concat2 / regions")


# ----------------------------------------------------------------------------------------------------- sample gates
@pytest.mark.parametrize("B,S,H", xc.SAMPLE_GATE)
def test_sample_gate_fwd_bwd(B, S, H):
    lib, K, s = _env()
    a0, c0, d0 = xc.rnd(B * S, H, seed=1), xc.rnd(B * S, H, seed=2), xc.rnd(B * S, H, seed=3)
    for mode in (0, 1):
        gate0 = xc.rnd(B * (mode + 1), seed=4, scale=2.0)
        for with_c, with_dc in ((False, False), (True, True), (True, False)):
            for v in (0, 1):
                bf = Bufs(v)
                a, c = bf.fin(a0, "a", ld=True), (bf.fin(c0, "c", ld=True) if with_c else None)
                gate, dout = bf.fin(gate0, "gate"), bf.fin(d0, "dout", ld=True)
                out = bf.out(B * S, H, "out", ld=True)
                _ok(lib.icka_x_sample_gate_fwd(_ptr(a), a.ld, _ptr(c), c.ld if with_c else 0, _ptr(gate), mode, _ptr(out), out.ld,
                                               B, S, H, s), "icka_x_sample_gate_fwd")
                bf.check("sample_gate_fwd")
                cv = c.view if with_c else None
                xc.compare({"out": out.view}, xc.sample_gate_fwd_refs(a.view, cv, gate.view[0], mode, B, S), "sample_gate_fwd")
                da, dc = bf.out(B * S, H, "da", ld=True), (bf.out(B * S, H, "dc", ld=True) if with_dc else None)
                dgate = bf.out(1, B * (mode + 1), "dgate", init=7.0)       # OVERWRITTEN: the prefill must not survive
                _ok(lib.icka_x_sample_gate_bwd(_ptr(dout), dout.ld, _ptr(a), a.ld, _ptr(c), c.ld if with_c else 0, _ptr(gate), mode,
                                               _ptr(da), da.ld, _ptr(dc), dc.ld if with_dc else 0, _ptr(dgate), B, S, H, s),
                    "icka_x_sample_gate_bwd")
                bf.check("sample_gate_bwd")
                refs = xc.sample_gate_bwd_refs(dout.view, a.view, cv, gate.view[0], mode, B, S)
                xc.compare({"da": da.view, "dc": dc.view if with_dc else None, "dgate": dgate.view[0]}, refs, "sample_gate_bwd")
                if mode == 1:
                    w = dgate.view[0].reshape(B, 2)
                    xc.same_bits(w[:, 0], -w[:, 1], "dgate words are -t and +t")
    xc.report("x_sample_gate B=%d S=%d H=%d" % (B, S, H))


# -------------------------------------------------------------------------------------------------------- LSTM cell
def _others_untouched(before, after, blocks, what):
    """``blocks``: (row, first column, columns) the call may write; everything else is bitwise as before"""
    b, a = before.clone(), after.clone()
    for r, c0, n in blocks:
        b[r, c0:c0 + n] = 0.0
        a[r, c0:c0 + n] = 0.0
    xc.same_bits(a, b, what)


@pytest.mark.parametrize("B,S,H", xc.LSTM)
def test_lstm_cell_fwd_bwd(B, S, H):
    lib, K, s = _env()
    z0 = xc.uniform(B, S, 2, 4, H, seed=1, lo=-4.0, hi=4.0, planted=(40.0, -40.0))
    dy0 = xc.rnd(B, S, 2, H, seed=2)
    dh0 = [xc.rnd(2, B, H, seed=10 + k) for k in range(S)]
    z = z0.cuda()
    v5 = lambda g: g.view.reshape(B, S, 2, -1, H) if g.cols == 8 * H else g.view.reshape(B, S, 2, H)
    for v in (0, 1):
        bf = Bufs(v)
        gates = bf.out(B * S, 8 * H, "gates", init=z0.reshape(B * S, 8 * H).cuda())          # in place
        c_all, y, hprev = (bf.out(B * S, 2 * H, n) for n in ("c_all", "y", "hprev"))
        rows_of = lambda t: [b_ * S + t for b_ in range(B)]
        for k in range(S):
            before = [g.view.clone() for g in (gates, c_all, y, hprev)]
            _ok(lib.icka_x_lstm_cell_fwd(_ptr(gates), _ptr(c_all), _ptr(y), _ptr(hprev), B, S, H, k, s), "icka_x_lstm_cell_fwd")
            bf.check("lstm_cell_fwd k=%d" % k)
            refs = xc.lstm_fwd_refs(z, v5(c_all), v5(y), B, S, H, k)
            for d, r in enumerate(refs):
                t = xc.lstm_rows(B, S, k)[d][0]
                xc.compare({"act": v5(gates)[:, t, d], "c": v5(c_all)[:, t, d], "y": v5(y)[:, t, d]}, r, "lstm_cell_fwd")
                xc.same_bits(v5(hprev)[:, t, d], r["hprev"], "hprev is the neighbouring y row (k=%d, direction %d)" % (k, d))
            for g, bef in zip((gates, c_all, y, hprev), before):
                w = g.cols // 2
                blocks = [(r_, d * w, w) for d in (0, 1) for r_ in rows_of(xc.lstm_rows(B, S, k)[d][0])]
                _others_untouched(bef, g.view, blocks, "lstm_cell_fwd k=%d: rows of other steps" % k)
        act = gates.view.clone().reshape(B, S, 2, 4, H)
        dy = bf.fin(dy0.reshape(B * S, 2 * H), "dy")
        dh_rec = bf.fin(torch.full((2 * B, H), NAN), "dh_rec")
        dc = bf.out(2 * B, H, "dc_carry")                                                    # NaN until the first call wrote it
        call = _bits(c_all)
        for k in range(S - 1, -1, -1):
            first = int(k == S - 1)
            if not first:
                dh_rec.view.copy_(dh0[k].reshape(2 * B, H))
            dc_in = dc.view.clone().reshape(2, B, H)
            before = gates.view.clone()
            _ok(lib.icka_x_lstm_cell_bwd(_ptr(dy), _ptr(dh_rec), _ptr(dc), _ptr(gates), _ptr(c_all), B, S, H, k, first, s),
                "icka_x_lstm_cell_bwd")
            bf.check("lstm_cell_bwd k=%d" % k)
            refs = xc.lstm_bwd_refs(v5(dy), dh_rec.view.reshape(2, B, H), dc_in, act, v5(c_all), B, S, H, k, bool(first))
            for d, r in enumerate(refs):
                t = xc.lstm_rows(B, S, k)[d][0]
                xc.compare({"dgates": v5(gates)[:, t, d], "dc_carry": dc.view.reshape(2, B, H)[d]}, r, "lstm_cell_bwd")
            blocks = [(r_, d * 4 * H, 4 * H) for d in (0, 1) for r_ in rows_of(xc.lstm_rows(B, S, k)[d][0])]
            _others_untouched(before, gates.view, blocks, "lstm_cell_bwd k=%d: rows of other steps" % k)
        assert torch.equal(call, _bits(c_all)), "lstm_cell_bwd wrote c_all"
    xc.report("x_lstm_cell B=%d S=%d H=%d" % (B, S, H))


# ------------------------------------------------------------------------------------------------------------ GEMM
def _desc(op, M, N, K, A, lda, a_bs, Bm, ldb, b_bs, Cm, ldc, c_bs, nb0, nb1, bias, alpha, beta):
    from icka_amd._lib import XGemmDesc
    d = XGemmDesc()
    d.op, d.M, d.N, d.K = op, M, N, K
    d.A, d.lda, d.a_bs0, d.a_bs1 = A, lda, a_bs[0], a_bs[1]
    d.B, d.ldb, d.b_bs0, d.b_bs1 = Bm, ldb, b_bs[0], b_bs[1]
    d.C, d.ldc, d.c_bs0, d.c_bs1 = Cm, ldc, c_bs[0], c_bs[1]
    d.nb0, d.nb1, d.bias, d.alpha, d.beta = nb0, nb1, bias, alpha, beta
    return d


def _gemm_shapes(op, M, N, K):
    return ((M, K) if op in (xc.NT, xc.NN) else (K, M)), ((N, K) if op in (xc.NT, xc.TT) else (K, N))


def _up4(n):
    return (n + 3) // 4 * 4


def _gemm_case(lib, s, op, M, N, K, with_bias, alpha, beta, v):
    """variant 0: leading dimensions rounded up to a multiple of 4 and aligned pointers (the 16-byte load path, with its
    scalar tail where K or the row length is no multiple of 4); variant 1: ld = cols + 3, pointers one element off"""
    sa, sb = _gemm_shapes(op, M, N, K)
    A0, B0, bias0, c0 = xc.rnd(*sa, seed=1), xc.rnd(*sb, seed=2), xc.rnd(N, seed=3), xc.rnd(M, N, seed=4)
    bf = Bufs(v)
    A, Bm = bf.fin(A0, "A", ld=True, ld_natural=_up4(sa[1])), bf.fin(B0, "B", ld=True, ld_natural=_up4(sb[1]))
    bias = bf.fin(bias0, "bias") if with_bias else None
    Cm = bf._keep(kc.Guarded(M, N, F32, ld=N + 3 if v else _up4(N), offset=v, init=c0.cuda() if beta != 0 else None), "C")
    d = _desc(op, M, N, K, _ptr(A), A.ld, (0, 0), _ptr(Bm), Bm.ld, (0, 0), _ptr(Cm), Cm.ld, (0, 0), 1, 1, _ptr(bias), alpha, beta)
    _ok(lib.icka_x_gemm(C.byref(d), s), "icka_x_gemm")
    bf.check("x_gemm")
    refs = xc.gemm_refs(op, A.view, Bm.view, bias.view[0] if with_bias else None, alpha, beta, c0.cuda())
    xc.compare({"C": Cm.view}, refs, "x_gemm")


class Batched:
    """nb0 x nb1 matrices [rows, cols] (row stride ld, batch strides bs0 / bs1 elements) inside ONE flat allocation; every
    element that belongs to no matrix -- the bands in front and behind AND the gaps between consecutive slices -- holds
    ``fill``, and ``check`` compares integer views against it."""

    PAD = 1024

    def __init__(self, nb0, nb1, rows, cols, ld, bs0, bs1, fill, off, init=None):
        assert bs1 >= rows * ld and bs0 >= nb1 * bs1
        self.geom = ((nb0, nb1, rows, cols), (bs0, bs1, ld, 1), self.PAD + off)
        n = _up4(2 * self.PAD + off + (nb0 - 1) * bs0 + (nb1 - 1) * bs1 + rows * ld)
        self.fill, self.ld, self.bs = fill, ld, (bs0, bs1)
        self.flat = torch.full((n,), fill, dtype=I32, device="cuda").view(F32)
        self.view = self.flat.as_strided(*self.geom)
        self.view.copy_(init.cuda()) if init is not None else self.view.fill_(NAN)

    def check(self, what):
        inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device="cuda")
        inside.as_strided(*self.geom).fill_(True)
        bad = ~inside & (self.flat.view(I32) != self.fill)
        assert not bool(bad.any()), "%s: %d elements outside the batch slices were written; first at flat index %d" % (
            what, int(bad.sum()), int(torch.nonzero(bad)[0, 0]) - self.geom[2])


def _gemm_batched(lib, s, op, vec):
    """nb0 = 2, nb1 = 3.  vec: every leading dimension and batch stride a multiple of 4, pointers aligned (both vector flags
    on); else odd batch strides (both flags off).  The gaps between the slices of C hold the sentinel."""
    M, N, K, nb0, nb1 = 5, 9, 18, 2, 3
    sa, sb = _gemm_shapes(op, M, N, K)

    def make(shape, fill, seed, init=True):
        rows, cols = shape
        ld = _up4(cols) if vec else cols + 3
        bs1 = _up4(rows * ld) + 4 if vec else (rows * ld + 2) | 1
        bs0 = _up4(nb1 * bs1) + 8 if vec else (nb1 * bs1 + 2) | 1
        return Batched(nb0, nb1, rows, cols, ld, bs0, bs1, fill, 0 if vec else 1,
                       xc.rnd(nb0, nb1, rows, cols, seed=seed) if init else None)

    A, Bm = make(sa, kc.NAN_FILL[F32], 1), make(sb, kc.NAN_FILL[F32], 2)
    c0 = xc.rnd(nb0, nb1, M, N, seed=4)
    bias0 = xc.rnd(N, seed=3)
    for alpha, beta in xc.GEMM_AB:
        Cm = make((M, N), kc.SENTINEL[F32], 4, init=beta != 0)
        bias = kc.Guarded(1, N, F32, fill=kc.NAN_FILL[F32], init=bias0.reshape(1, N).cuda())
        d = _desc(op, M, N, K, A.view.data_ptr(), A.ld, A.bs, Bm.view.data_ptr(), Bm.ld, Bm.bs, Cm.view.data_ptr(), Cm.ld, Cm.bs,
                  nb0, nb1, bias.view.data_ptr(), alpha, beta)
        _ok(lib.icka_x_gemm(C.byref(d), s), "icka_x_gemm")
        torch.cuda.synchronize()
        for g, n in ((A, "A"), (Bm, "B"), (Cm, "C")):
            g.check("x_gemm batched %s (%s)" % (n, "vector" if vec else "scalar"))
        bias.check(what="x_gemm batched bias")
        xc.compare({"C": Cm.view}, xc.gemm_refs(op, A.view, Bm.view, bias.view[0], alpha, beta, c0.cuda()), "x_gemm batched")


@pytest.mark.parametrize("op", [xc.NT, xc.NN, xc.TN, xc.TT])
def test_gemm(op):
    lib, K_, s = _env()
    for i, (M, N) in enumerate(xc.GEMM_MN):
        for j, K in enumerate(xc.GEMM_K):
            alpha, beta = xc.GEMM_AB[(i + j) % 2]
            for v in (0, 1):
                _gemm_case(lib, s, op, M, N, K, (i + j) % 3 != 0, alpha, beta, v)
    for K in (17, 50):                         # both (alpha, beta) and both bias forms at the two k-tail sizes above 16
        for alpha, beta in xc.GEMM_AB:
            for with_bias in (False, True):
                _gemm_case(lib, s, op, 129, 127, K, with_bias, alpha, beta, 1)
    _gemm_batched(lib, s, op, vec=False)
    _gemm_batched(lib, s, op, vec=True)
    xc.report("x_gemm op %d" % op)


# --------------------------------------------------------------------------------------------------------- token CE
@pytest.mark.parametrize("C_,ld", xc.CE_C_LD)
@pytest.mark.parametrize("M", xc.CE_M)
def test_token_ce(M, C_, ld):
    """A row counts iff mask != 0 and 0 <= label < C in 64 bits; a row that does not count has an all-zero gradient row and
    adds nothing to loss_sum / count (include/icka_hip.h).  Labels -100, C and 2^32 + 3 sit on valid rows."""
    lib, K, s = _env()
    x0, labels0, mask0 = xc.ce_inputs(M, C_)
    for v in (0, 1):
        b = Bufs(v)
        x = b._keep(kc.Guarded(M, C_, F32, ld=ld + 3 * v, offset=v, fill=kc.NAN_FILL[F32], init=x0.cuda()), "logits")
        labels, mask = b.ints(labels0, "labels"), b.ints(mask0, "mask")
        acc = b.out(1, 2, "accumulators", init=torch.tensor([[0.5, 2.0]]))
        dl = b.out(M, C_, "dlogits")
        _ok(lib.icka_x_token_ce(_ptr(x), x.ld, _ptr(labels), _ptr(mask), acc.view[0, 0:1].data_ptr(), acc.view[0, 1:2].data_ptr(),
                                _ptr(dl), M, C_, s), "icka_x_token_ce")
        b.check("token_ce")
        refs = xc.token_ce_refs(x.view, *_cu(labels0, mask0))
        xc.compare({"dlogits": dl.view, "loss_sum": acc.view[0, 0:1]}, refs, "token_ce")
        assert float(acc.view[0, 1]) == refs["count"], ("count", float(acc.view[0, 1]), refs["count"])
    xc.report("x_token_ce M=%d C=%d ld=%d" % (M, C_, ld))


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_the_documented_code_and_write_nothing():
    """NULL required pointer: ICKA_E_ARG; a dimension out of range: ICKA_E_SHAPE; an unknown mode / op: ICKA_E_ARG; n <= 0 in
    the flat kernels: 0 and no launch.  All of these return before any launch: the buffers keep every bit."""
    lib, K, s = _env()
    f = kc.Guarded(64, 64, F32)
    i = kc.Guarded(1, 64, I64, init=torch.zeros(1, 64, dtype=I64))
    before = _bits(f), _bits(i)
    p, q, ld = _ptr(f), _ptr(i), 64

    def gemm(**kw):
        a = dict(op=0, M=4, N=4, K=4, A=p, lda=ld, a_bs=(0, 0), Bm=p, ldb=ld, b_bs=(0, 0), Cm=p, ldc=ld, c_bs=(0, 0), nb0=1, nb1=1,
                 bias=None, alpha=1.0, beta=0.0)
        a.update(kw)
        return lib.icka_x_gemm(C.byref(_desc(**a)), s)

    got = {
        "gemm A NULL": (gemm(A=None), E_ARG), "gemm desc NULL": (lib.icka_x_gemm(None, s), E_ARG), "gemm M = 0": (gemm(M=0), E_SHAPE),
        "gemm K = -1": (gemm(K=-1), E_SHAPE), "gemm nb0 nb1 = 65536": (gemm(nb0=256, nb1=256), E_SHAPE), "gemm op = 4": (gemm(op=4), E_ARG),
        "ln_fwd x NULL": (lib.icka_x_ln_fwd(None, ld, p, ld, p, p, p, p, p, 4, 4, 1e-12, 0.0, 0, s), E_ARG),
        "ln_fwd M = 0": (lib.icka_x_ln_fwd(p, ld, p, ld, p, p, p, p, p, 0, 4, 1e-12, 0.0, 0, s), E_SHAPE),
        "ln_bwd rstd NULL": (lib.icka_x_ln_bwd(p, ld, p, None, p, p, p, 4, 4, 0.0, 0, s), E_ARG),
        "ln_bwd H = 0": (lib.icka_x_ln_bwd(p, ld, p, p, p, p, p, 4, 0, 0.0, 0, s), E_SHAPE),
        "colsum out NULL": (lib.icka_x_colsum(p, ld, None, 0, None, 4, 4, 0, s), E_ARG),
        "colsum N = 0": (lib.icka_x_colsum(p, ld, None, 0, p, 4, 0, 0, s), E_SHAPE),
        "embed_fwd ids NULL": (lib.icka_x_embed_fwd(None, None, p, p, p, p, p, p, p, p, 2, 2, 4, 1e-12, s), E_ARG),
        "embed_fwd B = 0": (lib.icka_x_embed_fwd(q, None, p, p, p, p, p, p, p, p, 0, 2, 4, 1e-12, s), E_SHAPE),
        "embed_scatter dtyp NULL": (lib.icka_x_embed_scatter(p, q, None, p, p, None, 2, 2, 4, 0, s), E_ARG),
        "embed_scatter S = 0": (lib.icka_x_embed_scatter(p, q, None, p, p, p, 2, 0, 4, 0, s), E_SHAPE),
        "softmax_fwd mask NULL": (lib.icka_x_softmax_fwd(p, p, None, 1, 1, 2, 4, 1.0, 0.0, 0, s), E_ARG),
        "softmax_fwd Skv = 0": (lib.icka_x_softmax_fwd(p, p, p, 1, 1, 2, 0, 1.0, 0.0, 0, s), E_SHAPE),
        "softmax_fwd p_drop > 0, Pd NULL": (lib.icka_x_softmax_fwd(p, None, p, 1, 1, 2, 4, 1.0, 0.1, 0, s), E_ARG),
        "softmax_bwd dS NULL": (lib.icka_x_softmax_bwd(p, None, 1, 1, 2, 4, 1.0, 0.0, 0, s), E_ARG),
        "softmax_bwd B = 0": (lib.icka_x_softmax_bwd(p, p, 0, 1, 2, 4, 1.0, 0.0, 0, s), E_SHAPE),
        "act_fwd y NULL": (lib.icka_x_act_fwd(p, None, None, None, 4, 0, s), E_ARG),
        "act_fwd mode = 3": (lib.icka_x_act_fwd(p, p, p, p, 4, 3, s), E_ARG),
        "act_fwd mode 2 without y2": (lib.icka_x_act_fwd(p, p, p, None, 4, 2, s), E_ARG),
        "act_fwd n = 0": (lib.icka_x_act_fwd(p, p, p, p, 0, 0, s), 0),
        "act_bwd saved NULL": (lib.icka_x_act_bwd(p, None, None, p, None, 4, 0, s), E_ARG),
        "act_bwd mode = 3": (lib.icka_x_act_bwd(p, p, p, p, p, 4, 3, s), E_ARG),
        "act_bwd n = -1": (lib.icka_x_act_bwd(p, p, p, p, p, -1, 0, s), 0),
        "dropout y NULL": (lib.icka_x_dropout(p, None, 4, 0.1, 0, s), E_ARG),
        "dropout n = 2^32": (lib.icka_x_dropout(p, p, 2 ** 32, 0.1, 0, s), E_SHAPE),
        "dropout n = 0": (lib.icka_x_dropout(p, p, 0, 0.1, 0, s), 0),
        "add b NULL": (lib.icka_x_add(p, ld, None, ld, p, ld, 4, 4, s), E_ARG),
        "add M = 0": (lib.icka_x_add(p, ld, p, ld, p, ld, 0, 4, s), E_SHAPE),
        "concat2 out NULL": (lib.icka_x_concat2(p, ld, 2, p, ld, 2, None, 4, s), E_ARG),
        "concat2 Ha = 0": (lib.icka_x_concat2(p, ld, 0, p, ld, 2, p, 4, s), E_SHAPE),
        "regions src NULL": (lib.icka_x_regions_to_tokens(None, p, 1, 2, 2, 0, s), E_ARG),
        "regions R = 0": (lib.icka_x_regions_to_tokens(p, p, 1, 0, 2, 0, s), E_SHAPE),
        "sample_gate_fwd gate NULL": (lib.icka_x_sample_gate_fwd(p, ld, None, 0, None, 0, p, ld, 1, 2, 4, s), E_ARG),
        "sample_gate_fwd mode = 2": (lib.icka_x_sample_gate_fwd(p, ld, None, 0, p, 2, p, ld, 1, 2, 4, s), E_ARG),
        "sample_gate_fwd H = 0": (lib.icka_x_sample_gate_fwd(p, ld, None, 0, p, 0, p, ld, 1, 2, 0, s), E_SHAPE),
        "sample_gate_fwd B = 65536": (lib.icka_x_sample_gate_fwd(p, ld, None, 0, p, 0, p, ld, 65536, 2, 4, s), E_SHAPE),
        "sample_gate_bwd dgate NULL": (lib.icka_x_sample_gate_bwd(p, ld, p, ld, None, 0, p, 0, p, ld, None, 0, None, 1, 2, 4, s), E_ARG),
        "sample_gate_bwd mode = 2": (lib.icka_x_sample_gate_bwd(p, ld, p, ld, None, 0, p, 2, p, ld, None, 0, p, 1, 2, 4, s), E_ARG),
        "sample_gate_bwd S = 0": (lib.icka_x_sample_gate_bwd(p, ld, p, ld, None, 0, p, 0, p, ld, None, 0, p, 1, 0, 4, s), E_SHAPE),
        "lstm_cell_fwd hprev NULL": (lib.icka_x_lstm_cell_fwd(p, p, p, None, 1, 2, 4, 0, s), E_ARG),
        "lstm_cell_fwd B = 0": (lib.icka_x_lstm_cell_fwd(p, p, p, p, 0, 2, 4, 0, s), E_SHAPE),
        "lstm_cell_fwd k = S": (lib.icka_x_lstm_cell_fwd(p, p, p, p, 1, 2, 4, 2, s), E_SHAPE),
        "lstm_cell_fwd k = -1": (lib.icka_x_lstm_cell_fwd(p, p, p, p, 1, 2, 4, -1, s), E_SHAPE),
        "lstm_cell_bwd dy NULL": (lib.icka_x_lstm_cell_bwd(None, p, p, p, p, 1, 2, 4, 0, 1, s), E_ARG),
        "lstm_cell_bwd H = 0": (lib.icka_x_lstm_cell_bwd(p, p, p, p, p, 1, 2, 0, 0, 1, s), E_SHAPE),
        "lstm_cell_bwd k = S": (lib.icka_x_lstm_cell_bwd(p, p, p, p, p, 1, 2, 4, 2, 1, s), E_SHAPE),
        "embed_prompt_fwd prompt NULL": (lib.icka_x_embed_prompt_fwd(q, q, None, p, p, p, p, p, p, p, p, 1, 2, 3, 1, 4, 0, 1e-12, s), E_ARG),
        "embed_prompt_fwd P = 0": (lib.icka_x_embed_prompt_fwd(q, q, p, p, p, p, p, p, p, p, p, 1, 2, 3, 0, 4, 0, 1e-12, s), E_SHAPE),
        "embed_prompt_fwd pos_offset = -1": (lib.icka_x_embed_prompt_fwd(q, q, p, p, p, p, p, p, p, p, p, 1, 2, 3, 1, 4, -1, 1e-12, s), E_SHAPE),
        "embed_prompt_scatter dprompt NULL": (lib.icka_x_embed_prompt_scatter(p, q, q, p, p, p, None, 1, 2, 3, 1, 4, 0, 0, s), E_ARG),
        "embed_prompt_scatter S_in = 0": (lib.icka_x_embed_prompt_scatter(p, q, q, p, p, p, p, 1, 0, 3, 1, 4, 0, 0, s), E_SHAPE),
        "token_ce count NULL": (lib.icka_x_token_ce(p, ld, q, q, p, None, p, 4, 4, s), E_ARG),
        "token_ce M = 0": (lib.icka_x_token_ce(p, ld, q, q, p, p, p, 0, 4, s), E_SHAPE),
        "token_ce ld < C": (lib.icka_x_token_ce(p, 3, q, q, p, p, p, 4, 4, s), E_SHAPE),
        "scale_by_ratio x NULL": (lib.icka_x_scale_by_ratio(None, p, None, None, 4, s), E_ARG),
        "scale_by_ratio n = 0": (lib.icka_x_scale_by_ratio(p, p, None, None, 0, s), 0),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not wrong, "(returned, documented): %s" % wrong
    assert torch.equal(before[0], _bits(f)) and torch.equal(before[1], _bits(i)), "a refused call wrote to its buffers"
    f.check(what="refusals f32 buffer")
    i.check(what="refusals int buffer")
