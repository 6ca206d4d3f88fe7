"""GPU: the embedding family of csrc/layernorm.hip (icka_embed_fwd, _fwd_h, _bwd, _bwd_rows, _scatter_rows, _prompt_fwd,
_prompt_bwd) and the flat-buffer kernels (csrc/optim.hip, the casts of csrc/dp.hip, icka_copy_many, icka_zero_f32,
icka_loss_accumulate, icka_scalar_ratio) element by element against float64 (tests/embed_check.py: references and bounds
derived from the number formats), through the C ABI, at the smallest shapes that reach each path: both backward kernels
(position-major, and row-major for S > 1024), NCH 1 .. 4, the wave loops over the batch and over the rows, every option.
Ids and token types sit in int64 buffers with sentinel bands, every other operand in NaN bands, every table row no token
may legally read is NaN, every output sits in sentinel bands, and every buffer is checked after every call.
tests/test_embed_check_cpu.py keeps the bounds used here honest."""
import ctypes as C

import pytest
import torch

import embed_check as ec
import kernel_check as kc
from embed_check import BF16, F16, F32, VOCAB, SEED, EPS_LN

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3          # include/icka_hip.h
I64 = torch.int64


def _env():
    from icka_amd import _lib
    from icka_amd import kernels as K
    K.set_dropout_nonce(None)
    return _lib.load(), K, K._stream()


def _ptr(g):
    return None if g is None else g.view.data_ptr()


def _ok(rc, name):
    assert rc == 0, "%s returned %d" % (name, rc)


class Bufs:
    """The guarded buffers of one case; ``check`` runs on all of them."""

    def __init__(self):
        self.all = []

    def _keep(self, g, name):
        self.all.append((name, g))
        return g

    def fin(self, values, name):
        """an operand [rows, cols] (1-D: one row) inside NaN bands (int64: sentinel bands)"""
        if values is None:
            return None
        values = values.reshape(1, -1) if values.dim() == 1 else values
        fill = kc.NAN_FILL.get(values.dtype, kc.SENTINEL.get(values.dtype))
        return self._keep(kc.Guarded(values.shape[0], values.shape[1], values.dtype, fill=fill, init=values.contiguous().cuda()), name)

    def out(self, rows, cols, dtype, name, init=None):
        """an output inside sentinel bands, prefilled with NaN (or ``init``)"""
        return self._keep(kc.Guarded(rows, cols, dtype, init=None if init is None else init.reshape(rows, cols).cuda()), name)

    def check(self, what):
        torch.cuda.synchronize()
        for name, g in self.all:
            g.check(what="%s: %s" % (what, name))


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _same(a, b, what):
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    ba, bb = _bits(a), _bits(b)
    ne = ba != bb
    if bool(ne.any()):
        at = int(torch.nonzero(ne.reshape(-1))[0, 0])
        raise AssertionError("%s: %d of %d elements differ bitwise; first at flat index %d: %#x against %#x"
                             % (what, int(ne.sum()), ne.numel(), at, int(ba.reshape(-1)[at]), int(bb.reshape(-1)[at])))


TWIN = {"none": None, "f32": F32, "f16": F16}


# ------------------------------------------------------------------------------------------------------- embeddings
def _embed_case(lib, s, c):
    """Forward (with the case's twin, then once more with twin / xhat / rstd NULL), then the backward from the kernel's own
    saved xhat and rstd.  Ids outside [0, VOCAB) are clamped by both (-3 is row 0, VOCAB + 2 is row VOCAB - 1) and the padding
    id is compared with the CLAMPED id: that is what ``ec.clamped_rows`` restates and what dword / dtok are held to."""
    inp, what = ec.embed_inputs(c), "embed " + ec.case_id(c)
    lay = ec.embed_layout(c, inp)
    B, S, H, nt, acc, pre = c["B"], c["S"], c["H"], c["n_type"], c["acc"], inp["pre"]
    M, npos = B * S, inp["npos"]
    bf = Bufs()
    ids, tt = bf.fin(inp["ids"].reshape(M, 1), "ids"), bf.fin(None if inp["tt"] is None else inp["tt"].reshape(M, 1), "tt")
    word, pos, typ = bf.fin(inp["word"], "word"), bf.fin(inp["pos"], "pos"), bf.fin(inp["typ"], "type")
    gamma, beta, dy = bf.fin(inp["gamma"], "gamma"), bf.fin(inp["beta"], "beta"), bf.fin(inp["dy"], "dy")
    tw = TWIN[c["twin"]]
    y, y2 = bf.out(M, H, BF16, "y"), bf.out(M, H, BF16, "y (no saves)")
    twin = None if tw is None else bf.out(M, H, tw, "twin")
    xhat, rstd = bf.out(M, H, BF16, "xhat"), bf.out(M, 1, F32, "rstd")
    fn = lib.icka_embed_fwd_h if tw == F16 else lib.icka_embed_fwd
    _ok(fn(_ptr(ids), _ptr(tt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(twin), _ptr(xhat),
           _ptr(rstd), B, S, H, VOCAB, nt, EPS_LN, c["p"], SEED, s), "icka_embed_fwd")
    _ok(fn(_ptr(ids), _ptr(tt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta), _ptr(y2), None, None, None,
           B, S, H, VOCAB, nt, EPS_LN, c["p"], SEED, s), "icka_embed_fwd (no saves)")
    bf.check(what + " fwd")
    rf = ec.fwd_refs(lay, inp["word"], inp["pos"], inp["typ"], None, inp["gamma"], inp["beta"], EPS_LN, inp["m"], tw)
    o = {"y": y.view, "twin": None if twin is None else twin.view, "xhat": xhat.view, "rstd": rstd.view.reshape(-1)}
    for name in ("y", "twin", "xhat", "rstd"):
        if o[name] is not None:
            kc.assert_within(o[name], rf[name][0], rf[name][1], "embed " + name, verbose=False)
    _same(y.view, y2.view, what + ": y without twin / xhat / rstd")
    if c["const"]:          # all-equal rows: variance 0, xhat 0, rstd = eps^-1/2, y == beta after its rounding
        assert not bool((_bits(xhat.view) & 0x7FFF).ne(0).any()), what + ": xhat of an all-equal row is not zero"
        _same(y.view, inp["beta"].to(BF16)[None].expand(M, H), what + ": y == bf16(beta)")
        if tw == F16:
            _same(twin.view, inp["beta"].to(F16)[None].expand(M, H), what + ": twin == fp16(beta)")
    # ---- backward
    dword = None if c["rows"] else bf.out(VOCAB, H, F32, "dword", pre["dword"])
    dtok = bf.out(M, H, F32, "dtok") if c["rows"] else None
    dpos = bf.out(npos, H, F32, "dpos", pre["dpos"])
    dtyp = bf.out(nt, H, F32, "dtype", pre["dtype"] if acc else None)
    dgam = bf.out(1, H, F32, "dgamma", pre["dgamma"] if acc else None)          # NaN where the call must overwrite
    dbet = bf.out(1, H, F32, "dbeta", pre["dbeta"] if acc else None)
    part = bf.out(int(lib.icka_ln_bwd_workspace_floats(H)), 1, F32, "partials")
    if c["rows"]:
        _ok(lib.icka_embed_bwd_rows(_ptr(dy), _ptr(ids), _ptr(tt), _ptr(xhat), _ptr(rstd), _ptr(gamma), _ptr(dtok), _ptr(dpos),
                                    _ptr(dtyp), _ptr(dgam), _ptr(dbet), _ptr(part), B, S, H, VOCAB, nt, c["pad"], c["p"], SEED,
                                    int(acc), s), "icka_embed_bwd_rows")
    else:
        _ok(lib.icka_embed_bwd(_ptr(dy), _ptr(ids), _ptr(tt), _ptr(xhat), _ptr(rstd), _ptr(gamma), _ptr(dword), _ptr(dpos),
                               _ptr(dtyp), _ptr(dgam), _ptr(dbet), _ptr(part), B, S, H, VOCAB, nt, c["pad"], c["p"], SEED,
                               int(acc), s), "icka_embed_bwd")
    bf.check(what + " bwd")
    rb = ec.bwd_refs(lay, inp["dy"], xhat.view.cpu(), rstd.view.cpu().reshape(-1), inp["gamma"], inp["m"], (VOCAB, npos, nt), nt,
                     c["pad"], acc, pre, rows=c["rows"])
    ob = {"dword": None if dword is None else dword.view, "dtok": None if dtok is None else dtok.view, "dpos": dpos.view,
          "dtype": dtyp.view, "dgamma": dgam.view.reshape(-1), "dbeta": dbet.view.reshape(-1)}
    ec.compare_bwd(ob, rb, pre, "embed")
    return ob, inp


@pytest.mark.parametrize("c", ec.SHAPE_CASES, ids=ec.case_id)
def test_embed_shapes(c):
    """every H (NCH 1 .. 4, H = 2048 with its 64 KiB of dynamic LDS) at (B, S) = (9, 5), every (B, S) at H = 72, and the
    row-major backward (S = 1025): B = 5 makes its wave loop take a second row, B = 9 that of the forward"""
    lib, _, s = _env()
    _embed_case(lib, s, c)
    kc.report("test_embed_shapes")


@pytest.mark.parametrize("form,n_type,tt", ec.OPTION_AXES)
def test_embed_options(form, n_type, tt):
    """padding_idx x p_drop x accumulate x (bwd, bwd_rows) x twin at H = 72 for one backward form, n_type and token-type input"""
    lib, _, s = _env()
    for c in ec.option_cases(form, n_type, tt):
        _embed_case(lib, s, c)
    kc.report("test_embed_options %s n_type=%d tt=%s" % (form, n_type, tt))


@pytest.mark.parametrize("c", ec.ID_CASES + ec.CONST_CASES, ids=ec.case_id)
def test_embed_id_patterns(c):
    """one id everywhere (every atomic of the launch lands on one table row), ids -3 and VOCAB + 2 (clamped to rows 0 and
    VOCAB - 1 by forward and backward; the padding id is compared with the clamped id), and all-equal rows"""
    lib, _, s = _env()
    _embed_case(lib, s, c)
    kc.report("test_embed_id_patterns")


@pytest.mark.parametrize("T,H,bf,scale", ec.SCATTER_CASES)
def test_embed_scatter_rows(T, H, bf, scale):
    """dword[ids[t]] += scale rows[t] for the concatenated rows of two "ranks"; the padding id, -1 and VOCAB are skipped"""
    lib, _, s = _env()
    rows, ids, pre = ec.scatter_inputs(T, H, bf)
    b = Bufs()
    gr, gi = b.fin(rows, "rows"), b.fin(ids.reshape(T, 1), "ids")
    dword = b.out(VOCAB, H, F32, "dword", pre)
    _ok(lib.icka_embed_scatter_rows(_ptr(gr), int(bf), _ptr(gi), _ptr(dword), T, H, VOCAB, 0, scale, s), "icka_embed_scatter_rows")
    b.check("scatter_rows")
    ref, unt = ec.scatter_rows_refs(rows, ids, VOCAB, 0, scale, pre)
    kc.assert_within(dword.view, ref[0], ref[1], "scatter_rows dword", verbose=False)
    assert bool(unt[0]) and bool(unt[VOCAB - 1])
    ec.check_untouched(dword.view, pre, unt, "scatter_rows dword")
    _ok(lib.icka_embed_scatter_rows(_ptr(gr), int(bf), _ptr(gi), _ptr(dword), 0, H, VOCAB, 0, scale, s), "T = 0")
    kc.report("test_embed_scatter_rows")


@pytest.mark.parametrize("c", ec.PROMPT_CASES, ids=ec.case_id)
def test_embed_prompt(c):
    lib, _, s = _env()
    inp, what = ec.prompt_inputs(c), "embed_prompt " + ec.case_id(c)
    lay = ec.prompt_layout(c, inp)
    B, S_in, P, H, off, acc, pre, S = c["B"], c["S_in"], c["P"], c["H"], c["off"], c["acc"], inp["pre"], inp["S"]
    M, npos, eps = B * S, inp["npos"], 1e-5
    bf = Bufs()
    ids, src = bf.fin(inp["ids"].reshape(-1, 1), "ids"), bf.fin(inp["src"].reshape(-1, 1), "src")
    prompt = bf.fin(inp["prompt"].reshape(B * P, H), "prompt")
    word, pos, typ = bf.fin(inp["word"], "word"), bf.fin(inp["pos"], "pos"), bf.fin(inp["typ"], "type")
    gamma, beta, dy = bf.fin(inp["gamma"], "gamma"), bf.fin(inp["beta"], "beta"), bf.fin(inp["dy"], "dy")
    y, twin = bf.out(M, H, BF16, "y"), bf.out(M, H, F32, "twin")
    xhat, rstd = bf.out(M, H, BF16, "xhat"), bf.out(M, 1, F32, "rstd")
    _ok(lib.icka_embed_prompt_fwd(_ptr(ids), _ptr(src), _ptr(prompt), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta),
                                  _ptr(y), _ptr(twin), _ptr(xhat), _ptr(rstd), B, S_in, S, P, H, VOCAB, off, eps, c["p"], SEED, s),
        "icka_embed_prompt_fwd")
    bf.check(what + " fwd")
    rf = ec.fwd_refs(lay, inp["word"], inp["pos"], inp["typ"], inp["prompt"], inp["gamma"], inp["beta"], eps, inp["m"], F32)
    for name, t in (("y", y.view), ("twin", twin.view), ("xhat", xhat.view), ("rstd", rstd.view.reshape(-1))):
        kc.assert_within(t, rf[name][0], rf[name][1], "embed_prompt " + name, verbose=False)
    dword, dpos = bf.out(VOCAB, H, F32, "dword", pre["dword"]), bf.out(npos, H, F32, "dpos", pre["dpos"])
    dtyp = bf.out(1, H, F32, "dtype", pre["dtype"] if acc else None)
    dgam = bf.out(1, H, F32, "dgamma", pre["dgamma"] if acc else None)
    dbet = bf.out(1, H, F32, "dbeta", pre["dbeta"] if acc else None)
    dprompt = bf.out(B * P, H, BF16, "dprompt")
    dprompt.view.view(torch.int16).fill_(kc.SENTINEL[BF16])          # must be fully overwritten
    part = bf.out(S * int(lib.icka_ln_slab_slots()) * H, 1, F32, "partials")
    _ok(lib.icka_embed_prompt_bwd(_ptr(dy), _ptr(ids), _ptr(src), _ptr(xhat), _ptr(rstd), _ptr(gamma), _ptr(dword), _ptr(dpos),
                                  _ptr(dtyp), _ptr(dgam), _ptr(dbet), _ptr(dprompt), _ptr(part), B, S_in, S, P, H, VOCAB, off,
                                  c["pad"], c["p"], SEED, int(acc), s), "icka_embed_prompt_bwd")
    bf.check(what + " bwd")
    rb = ec.bwd_refs(lay, inp["dy"], xhat.view.cpu(), rstd.view.cpu().reshape(-1), inp["gamma"], inp["m"], (VOCAB, npos, 1), 1,
                     c["pad"], acc, pre, n_prompt=B * P)
    ob = {"dword": dword.view, "dpos": dpos.view, "dtype": dtyp.view, "dgamma": dgam.view.reshape(-1),
          "dbeta": dbet.view.reshape(-1), "dprompt": dprompt.view}
    ec.compare_bwd(ob, rb, pre, "embed_prompt")
    kc.report("test_embed_prompt")


def test_embed_refusals():
    """H % 8 != 0, H > 2048, operands moved by 2 elements, dword / dtok absent, and a prompt splice of 1025 positions: each is
    refused with its error code and nothing is launched (every buffer is large enough for the shape asked for anyway)"""
    lib, _, s = _env()
    B, S, H = 2, 3, 72
    big = 2 * 1025 * 2056
    i64 = torch.zeros(big // 64, dtype=I64, device="cuda")
    i32 = torch.zeros(2048, dtype=torch.int32, device="cuda")
    f = [torch.zeros(big, dtype=F32, device="cuda") for _ in range(8)]
    ws = torch.zeros(int(lib.icka_ln_bwd_workspace_floats(2056)), dtype=F32, device="cuda")
    h = [torch.zeros(big, dtype=BF16, device="cuda") for _ in range(4)]
    P = lambda t, off=0: t.data_ptr() + off * t.element_size()

    def fwd(H=H, ow=0, op=0, ot=0, og=0, ob=0, oy=0, ox=0):
        return lib.icka_embed_fwd(P(i64), P(i64), P(f[0], ow), P(f[1], op), P(f[2], ot), P(f[3], og), P(f[4], ob), P(h[0], oy), None,
                                  P(h[1], ox), P(f[5]), B, S, H, VOCAB, 2, EPS_LN, 0.0, 0, s)

    def bwd(H=H, od=0, ox=0, og=0, dword=True, rows=False):
        fn = lib.icka_embed_bwd_rows if rows else lib.icka_embed_bwd
        return fn(P(h[0], od), P(i64), P(i64), P(h[1], ox), P(f[5]), P(f[3], og), P(f[0]) if dword else None, P(f[1]), P(f[2]), P(f[6]),
                  P(f[7]), P(ws), B, S, H, VOCAB, 2, 0, 0.0, 0, 1, s)

    assert fwd(H=12) == E_SHAPE and fwd(H=2056) == E_SHAPE and bwd(H=12) == E_SHAPE and bwd(H=2056) == E_SHAPE
    for k in ("ow", "op", "ot", "og", "ob", "oy", "ox"):
        assert fwd(**{k: 2}) == E_ALIGN, k
    for k in ("od", "ox", "og"):
        assert bwd(**{k: 2}) == E_ALIGN, k
    assert bwd(dword=False) == E_ARG and bwd(dword=False, rows=True) == E_ARG
    rc = lib.icka_embed_prompt_bwd(P(h[0]), P(i64), P(i32), P(h[1]), P(f[5]), P(f[3]), P(f[0]), P(f[1]), P(f[2]), P(f[6]), P(f[7]),
                                   P(h[2]), P(ws), 1, 8, 1025, 1, 8, VOCAB, 0, 1, 0.0, 0, 1, s)
    assert rc == E_SHAPE, rc
    assert fwd() == 0 and bwd() == 0          # the same calls, unmoved, are accepted
    torch.cuda.synchronize()
    kc.report("test_embed_refusals")


# ----------------------------------------------------------------------------------------------------- flat buffers
def _flat(b, values, name):
    return b.out(values.numel(), 1, values.dtype, name, values)


def _table(rows):
    return torch.tensor(rows, dtype=I64, device="cuda")


def _optim_setup(lib):
    assert lib.icka_optim_chunk_elems() == ec.OPT_CHUNK and lib.icka_dp_chunk_elems() == ec.OPT_CHUNK
    g0, g1, n = ec.chunk_ranges()
    return ec.chunk_rows(g0), ec.chunk_rows(g1), n


@pytest.mark.parametrize("with_coef", (True, False))
@pytest.mark.parametrize("lr", (0.0, 1e-2))
@pytest.mark.parametrize("wd", (0.0, 0.01))
@pytest.mark.parametrize("step", (1, 1000))
def test_optim_update(step, wd, lr, with_coef):
    """sqnorm -> clip -> adamw per group against float64, then sqnorm -> prepare -> adamw_dev on fresh copies: bitwise the
    same p, m, v and shadows.  The hole between the groups, the tail behind them and the bands keep their bits."""
    lib, K, s = _env()
    from icka_amd import _lib
    r0, r1, n = _optim_setup(lib)
    rows = r0 + r1
    p0, g0, m0, v0 = ec.adam_inputs(n)
    inside = ec.in_chunks(rows, n)
    b1, b2, eps, max_norm = 0.9, 0.999, 1e-8, (1.0 if with_coef else 0.0)
    f32 = lambda x: float(torch.tensor(x, dtype=F32))
    wds = (wd, 0.0)
    results = []
    for mode in ("host", "dev", "host, no fp16 shadow", "host, no shadows"):
        if mode.startswith("host,") and not (step == 1 and wd == 0.01 and lr == 1e-2 and with_coef):
            continue
        b = Bufs()
        p, g, m, v = _flat(b, p0, "p"), _flat(b, g0, "g"), _flat(b, m0, "m"), _flat(b, v0, "v")
        sh = None if mode == "host, no shadows" else b.out(n, 1, BF16, "shadow_bf16")
        sh16 = None if mode.startswith("host,") else b.out(n, 1, F16, "shadow_f16")
        for t in (sh, sh16):
            if t is not None:
                t.view.view(torch.int16).fill_(kc.SENTINEL[t.dtype])
        part, out2 = b.out(len(rows), 1, F32, "partials"), b.out(2, 1, F32, "norm, coef")
        _ok(lib.icka_optim_sqnorm(_ptr(g), _table(rows).data_ptr(), len(rows), _ptr(part), s), "icka_optim_sqnorm")
        b.check("sqnorm")
        rs = ec.sqnorm_refs(g0, rows)["partials"]
        kc.assert_within(part.view.reshape(-1), rs[0], rs[1], "optim sqnorm partials", verbose=False)
        if mode != "dev":
            _ok(lib.icka_optim_clip(_ptr(part), len(rows), max_norm, _ptr(out2), s), "icka_optim_clip")
            norm, coef = out2.view.reshape(-1)[0:1], out2.view.reshape(-1)[1:2]
            for gi, rr in enumerate((r0, r1)):
                _ok(lib.icka_optim_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(sh), _ptr(sh16), _table(rr).data_ptr(), len(rr),
                                         coef.data_ptr() if with_coef else None, lr, b1, b2, eps, wds[gi], step, s), "icka_optim_adamw")
        else:
            st = _lib.OptimState()
            st.t, st.kind, st.n_groups = step - 1, _lib.OPTIM_SCHEDULE_CONSTANT, 2
            for gi in (0, 1):
                st.base_lr[gi], st.beta1[gi], st.beta2[gi], st.eps[gi], st.weight_decay[gi] = f32(lr), b1, b2, eps, wds[gi]
            state = K.optim_state_new("cuda")
            K.optim_state_write(state, st, 0, C.sizeof(_lib.OptimState))
            _ok(lib.icka_optim_prepare(_ptr(part), len(rows), max_norm, 0, state.data_ptr(), s), "icka_optim_prepare")
            t3 = _table(ec.chunk_rows([(lo, lo + k) for lo, k in r0], 0) + ec.chunk_rows([(lo, lo + k) for lo, k in r1], 1))
            _ok(lib.icka_optim_adamw_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(sh), _ptr(sh16), t3.data_ptr(), t3.shape[0],
                                         state.data_ptr(), s), "icka_optim_adamw_dev")
            got = K.optim_state_read(state)
            assert got.t == step and got.skip == 0
            norm = torch.tensor([got.norm], dtype=F32)
            coef = torch.tensor([got.coef], dtype=F32)
        b.check("optim " + mode)
        rn = ec.clip_refs(part.view.cpu().reshape(-1), max_norm)["norm"]
        kc.assert_within(norm.reshape(1), rn[0].reshape(1), rn[1].reshape(1), "optim norm", verbose=False)
        cr, cb = ec.clip_coef(norm, max_norm)
        kc.assert_within(coef.reshape(1), cr.reshape(1), cb, "optim coef", verbose=False)
        cval = float(coef.cpu()) if with_coef else 1.0
        o = {"p": p.view.reshape(-1).cpu(), "m": m.view.reshape(-1).cpu(), "v": v.view.reshape(-1).cpu()}
        _same(g.view.reshape(-1), g0, "optim: g is read only")
        for gi, rr in enumerate((r0, r1)):
            mk = ec.in_chunks(rr, n)
            ref = ec.adamw_refs(p0[mk], g0[mk], m0[mk], v0[mk], cval, f32(lr), f32(b1), f32(b2), f32(eps), f32(wds[gi]), step)
            for name in ("p", "m", "v"):
                kc.assert_within(o[name][mk], ref[name][0], ref[name][1], "optim adamw " + name, verbose=False)
        for name, orig in (("p", p0), ("m", m0), ("v", v0)):
            _same(o[name][~inside], orig[~inside], "optim %s outside the chunks" % name)
        if sh is not None:
            got_sh = sh.view.reshape(-1).cpu()
            _same(got_sh[inside], ec.shadow_bf16(o["p"])[inside], "bf16 shadow == bf16(p)")
            assert bool((_bits(got_sh[~inside]) == kc.SENTINEL[BF16]).all()), "bf16 shadow outside the chunks"
            o["sh"] = got_sh
        if sh16 is not None:
            got16 = sh16.view.reshape(-1).cpu()
            _same(got16[inside], ec.shadow_f16(o["p"])[inside], "fp16 shadow == fp16(clamp(p))")
            assert float(got16[9]) == ec.FP16_MAX and float(got16[8190]) == -ec.FP16_MAX
            assert bool((_bits(got16[~inside]) == kc.SENTINEL[F16]).all()), "fp16 shadow outside the chunks"
            o["sh16"] = got16
        o["norm"], o["coef"] = norm.cpu(), coef.cpu()
        results.append((mode, o))
    host, dev = results[0][1], results[1][1]
    for name in ("p", "m", "v", "sh", "sh16", "norm", "coef"):
        _same(host[name], dev[name], "adamw_dev == adamw: " + name)
    for mode, o in results[2:]:
        for name in ("p", "m", "v"):
            _same(host[name], o[name], "%s: %s" % (mode, name))
    kc.report("test_optim_update")


@pytest.mark.parametrize("n", ec.CLIP_N)
def test_optim_clip_and_prepare(n):
    """the one-block stride loop over n partials: norm against the float64 sum, the coefficient in f32 from that norm,
    max_norm <= 0 gives 1, and icka_optim_prepare gives bitwise the norm and coefficient of icka_optim_clip"""
    lib, K, s = _env()
    from icka_amd import _lib
    vals = ec.rnd(n, seed=61).abs() + 0.01
    for max_norm in (1.0, 1e3, 0.0, -1.0):
        b = Bufs()
        part, out2 = b.fin(vals, "partials"), b.out(2, 1, F32, "norm, coef")
        _ok(lib.icka_optim_clip(_ptr(part), n, max_norm, _ptr(out2), s), "icka_optim_clip")
        b.check("clip")
        norm, coef = out2.view.reshape(-1)[0].cpu(), out2.view.reshape(-1)[1].cpu()
        rn = ec.clip_refs(vals, max_norm)["norm"]
        kc.assert_within(norm.reshape(1), rn[0].reshape(1), rn[1].reshape(1), "optim_clip norm", verbose=False)
        cr, cb = ec.clip_coef(norm, max_norm)
        kc.assert_within(coef.reshape(1), cr.reshape(1), cb, "optim_clip coef", verbose=False)
        if max_norm <= 0:
            assert float(coef) == 1.0
        st = _lib.OptimState()
        st.n_groups, st.t = 1, 4
        st.base_lr[0], st.beta1[0], st.beta2[0], st.eps[0] = 1e-3, 0.9, 0.999, 1e-8
        state = K.optim_state_new("cuda")
        K.optim_state_write(state, st, 0, C.sizeof(_lib.OptimState))
        _ok(lib.icka_optim_prepare(_ptr(part), n, max_norm, 0, state.data_ptr(), s), "icka_optim_prepare")
        b.check("prepare")
        got = K.optim_state_read(state)
        _same(torch.tensor([got.norm, got.coef], dtype=F32), torch.stack([norm, coef]), "prepare == clip")
        assert got.t == 5 and got.skip == 0 and got.skipped == 0
    kc.report("test_optim_clip_and_prepare")


def test_dp_cast_chunks():
    """bitwise src.to(bf16) on the chunks (+-inf, NaN, -0.0, both halfway cases planted), the sentinel everywhere else"""
    lib, _, s = _env()
    r0, r1, n = _optim_setup(lib)
    rows = r0 + r1
    x = ec.cast_inputs(n)
    b = Bufs()
    src, dst = b.fin(x.reshape(-1, 1), "src"), b.out(n, 1, BF16, "dst")
    dst.view.view(torch.int16).fill_(kc.SENTINEL[BF16])
    _ok(lib.icka_dp_cast_chunks(_ptr(src), _ptr(dst), None, 0, s), "n_chunks = 0")
    b.check("cast_chunks, no chunk")
    assert bool((_bits(dst.view) == kc.SENTINEL[BF16]).all()), "n_chunks = 0 is a no-op"
    _ok(lib.icka_dp_cast_chunks(_ptr(src), _ptr(dst), _table(rows).data_ptr(), len(rows), s), "icka_dp_cast_chunks")
    b.check("cast_chunks")
    inside, got = ec.in_chunks(rows, n), dst.view.reshape(-1).cpu()
    # (the NaN is compared apart: which NaN torch's own conversion gives depends on the host -- 0x7fc0 on one, 0xffff on
    # another -- so there the kernel is held to the upper half of the source word, 0x7fc0, and torch only to "a NaN")
    num = inside & ~torch.isnan(x)
    _same(got[num], x.to(BF16)[num], "dp_cast_chunks == src.to(bf16)")
    assert int(torch.isnan(x[inside]).sum()) == 1 and bool(torch.isnan(x.to(BF16)[7]))
    assert int(_bits(got)[7]) == 0x7FC0, "NaN 0x7fc00000 -> %#x" % int(_bits(got)[7])
    assert _bits(got)[12] == 0x3F80 and _bits(got)[13] == 0x3F82, "ties go to the even neighbour"
    assert bool((_bits(got[~inside]) == kc.SENTINEL[BF16]).all()), "the destination outside the chunks"
    kc.report("test_dp_cast_chunks")


@pytest.mark.parametrize("n", ec.CAST_BACK_N)
def test_dp_cast_back_scaled(n):
    """dst = bf2f(src) * scale as one f32 product, bitwise; n = 2^24 + 13 takes the grid-stride loop and the tail of n & 7"""
    lib, _, s = _env()
    g = torch.Generator(device="cuda").manual_seed(71)
    x = torch.randn(n, generator=g, device="cuda").to(BF16)
    for scale in ec.CAST_SCALES:
        b = Bufs()
        src, dst = b.fin(x.reshape(-1, 1), "src"), b.out(n, 1, F32, "dst")
        _ok(lib.icka_dp_cast_back_scaled(_ptr(src), _ptr(dst), n, scale, s), "icka_dp_cast_back_scaled")
        b.check("cast_back")
        ref = ec.cast_back_ref(x, scale)
        assert torch.equal(dst.view.reshape(-1).view(torch.int32), ref.view(torch.int32)), "cast_back n=%d scale=%g" % (n, scale)
    kc.report("test_dp_cast_back_scaled")


def test_copy_many():
    """eight copies in one launch (0 .. 1 MiB; 16-byte sized and aligned ones take the vector path, the others the byte path),
    a pair moved by 2 bytes, a single copy, n = 0, and n = 9 refused; every destination bitwise, bands untouched"""
    lib, _, s = _env()

    def run(sizes, shift=0):
        b = Bufs()
        src = ec.copy_sources(sizes, shift)
        gs = [b.fin(t.reshape(-1, 1), "src %d" % i) for i, t in enumerate(src)]
        gd = [b.out(t.numel(), 1, torch.uint8, "dst %d" % i) for i, t in enumerate(src)]
        k = len(sizes)
        sp = (C.c_void_p * max(k, 1))(*[_ptr(t) + shift for t in gs])
        dp = (C.c_void_p * max(k, 1))(*[_ptr(t) + shift for t in gd])
        nb = (C.c_int64 * max(k, 1))(*sizes)
        _ok(lib.icka_copy_many(sp, dp, nb, k, s), "icka_copy_many")
        b.check("copy_many")
        for i in range(k):
            ec.same_bytes(gd[i].view.reshape(-1)[shift:], src[i][shift:], "copy %d of %d bytes" % (i, sizes[i]))
            if shift:
                assert bool((_bits(gd[i].view.reshape(-1)[:shift]) == kc.SENTINEL[torch.uint8]).all())

    run(list(ec.COPY_BYTES))
    run([4096, 65536], shift=2)          # 16-byte sizes at pointers that are not: the byte path
    run([17])
    run([4096])
    run([])
    z = (C.c_void_p * 9)()
    assert lib.icka_copy_many(z, z, (C.c_int64 * 9)(), 9, s) == E_ARG
    kc.report("test_copy_many")


@pytest.mark.parametrize("n", ec.ZERO_N)
def test_zero_f32(n):
    """the 16-byte body and the scalar tail of n & 3; the last n is beyond one pass of the capped grid"""
    lib, _, s = _env()
    b = Bufs()
    t = b.out(n, 1, F32, "p", torch.full((n,), 3.0))
    _ok(lib.icka_zero_f32(_ptr(t), n, s), "icka_zero_f32")
    b.check("zero_f32")
    assert not bool(t.view.view(torch.int32).ne(0).any()), "zero_f32 n=%d" % n
    kc.report("test_zero_f32")


def test_zero_rows_of_a_bf16_matrix():
    """kernels.zero_rows_ from an odd row of a bf16 [7, 8] matrix: rows [3, 7) are +0, rows [0, 3) and the bands keep their bits"""
    lib, K, s = _env()
    b = Bufs()
    x = ec.rnd(7, 8, seed=91).to(BF16)
    t = b.out(7, 8, BF16, "t", x)
    K.zero_rows_(t.view, 3)
    b.check("zero_rows_")
    _same(t.view[:3], x[:3], "rows in front")
    assert not bool(_bits(t.view[3:]).ne(0).any())
    kc.report("test_zero_rows_of_a_bf16_matrix")


def test_loss_accumulate_and_scalar_ratio():
    """three accumulated losses: the f64 sum is exact and the count is 3; scalar_ratio: num / max(den, 1), one f32 division"""
    lib, _, s = _env()
    b = Bufs()
    acc = torch.zeros(2, dtype=torch.float64, device="cuda")
    losses = [0.1, 1e-7, 3e5]
    for v in losses:
        loss = b.fin(torch.tensor([v], dtype=F32), "loss")
        _ok(lib.icka_loss_accumulate(_ptr(loss), acc.data_ptr(), s), "icka_loss_accumulate")
    b.check("loss_accumulate")
    want = sum(float(torch.tensor(v, dtype=F32)) for v in losses)
    got = acc.cpu()
    assert float(got[0]) == want and float(got[1]) == 3.0
    for den in (0.0, 0.5, 1.0, 7.0):
        b = Bufs()
        num, dn = b.fin(torch.tensor([2.5], dtype=F32), "num"), b.fin(torch.tensor([den], dtype=F32), "den")
        out = b.out(1, 1, F32, "out")
        _ok(lib.icka_scalar_ratio(_ptr(out), _ptr(num), _ptr(dn), s), "icka_scalar_ratio")
        b.check("scalar_ratio")
        ref = 2.5 / max(den, 1.0)
        kc.assert_within(out.view.reshape(1), torch.tensor([ref], dtype=torch.float64), kc.stored(ec.DIV_REL * ref, torch.tensor([ref]), F32),
                         "scalar_ratio", verbose=False)
        if den < 1:
            assert float(out.view) == 2.5
    kc.report("test_loss_accumulate_and_scalar_ratio")
