"""Helpers of the element-wise tests of the embedding family (csrc/layernorm.hip: icka_embed_fwd, _fwd_h, _bwd, _bwd_rows,
_scatter_rows, _prompt_fwd, _prompt_bwd) and of the flat-buffer kernels (csrc/optim.hip, csrc/dp.hip, icka_copy_many,
icka_zero_f32, icka_loss_accumulate, icka_scalar_ratio); no test functions.  For every kernel a function that takes the very
values the kernel reads and returns {output: (float64 reference, bound)}, plus the case lists and input builders that
tests/test_embed_check_cpu.py (emulations, seeded faults) and tests/test_embed_elements_gpu.py (the device) share.  The
buffers and the comparison are those of tests/kernel_check.py, the LayerNorm bounds its ``ln_fwd_bounds`` / ``ln_bwd_bounds``,
the row conventions those of tests/exact_check.py.  Nothing here is a fitted constant.

Where the bounds come from
--------------------------
* In the embedding bounds one f32 operation is charged u = U_ACC = 2^-23 of its result, as tests/kernel_check.py does (round
  to nearest, factor 2 spare); in the AdamW bound u = U = 2^-24, the unit roundoff itself.
* Forward: s = (word[id] + pos[sp + pos_offset]) + type[t] (or the bf16 prompt row in place of the word row), with the kernel's
  clamps of id and t.  ``ln_fwd_bounds`` with t_abs = |w| + |p| + |ty|; its e_s = 3 u t_abs pays the two additions (one
  rounding to spare).  The dropout multiplier m is applied to y only: e = m e_y + u |y m|, then the storage rounding of the
  format (bf16 y, f32 or fp16 twin).
* Backward: dl = dy m (one rounding, inside the 2 u |gd| of ``ln_bwd_bounds`` together with the gamma product) feeds
  ``ln_bwd_bounds``; ds is its "ds_raw".  A table row is a sum of ds rows in ANY order (wave loop, 8-wave block reduction,
  slabs + finalize, atomics): sum of the e_ds of the contributing rows + (n + 4) u (sum|ds| + |prefill|), stored in f32; the
  prefill enters exactly.  A row that receives nothing keeps its prefill BITWISE (``untouched`` says which).
* dtok = f32(ds) (exact zero rows for the padding id); dprompt = bf16(ds).
* AdamW: one u = 2^-24 per f32 operation of the kernel's formula, 2^-22 relative for sqrtf and for each division (a REQUIREMENT on
  the device, as LIBM_REL of tests/exact_check.py); see ``adamw_refs``.
"""
import math

import torch

import exact_check as xc
import kernel_check as kc
from kernel_check import BF16, F16, F32, U_ACC, assert_within, report, stored, with_beta  # noqa: F401
from exact_check import same_bits, cpu_dropout_mask  # noqa: F401

F64 = torch.float64
U = kc.EPS[F32]               # 2^-24: unit roundoff of one f32 operation (round to nearest) -- the unit of the AdamW bound
DIV_REL = 2.0 ** -22          # REQUIREMENT on sqrtf and on an f32 division of the device: relative error of the result
VOCAB = 13
EPS_LN = 1e-12
SEED = 0x1234567811
OPT_CHUNK = 8192              # icka_optim_chunk_elems() == icka_dp_chunk_elems() (the GPU test asserts both)
FP16_MAX = 65504.0


def _d(t):
    return t.double()


# =============================================================================================== embedding cases
def ecase(B, S, H, n_type=2, tt="given", pad=0, p=0.0, acc=True, rows=False, twin="f32", ids="rand", const=False):
    """One case of icka_embed_fwd + icka_embed_bwd / _bwd_rows.  tt: "given" / "none" / "oob" (holds -1 and n_type);
    twin: "none" / "f32" / "f16"; ids: "rand" (padding id at the start of sample 0, in the middle of sample 1, the whole of the
    last sample when B >= 3) / "repeat" (one id everywhere) / "oob" (holds -3 and VOCAB + 2); const: every row all-equal."""
    return dict(B=B, S=S, H=H, n_type=n_type, tt=tt, pad=pad, p=p, acc=acc, rows=rows, twin=twin, ids=ids, const=const)


def case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items())


H_ALL = (8, 72, 520, 1032, 2048)            # NCH 1, 1, 2, 3, 4, the last wave-chunk partly filled
SHAPE_CASES = ([ecase(9, 5, H) for H in H_ALL] + [ecase(B, S, 72) for B in (1, 3, 9) for S in (1, 5, 37)] +
               [ecase(9, 5, 2048, rows=True, p=0.1, twin="f16")] +
               [ecase(B, 1025, H, rows=(B == 5)) for H in (8, 72) for B in (1, 5, 9)])      # row-major backward: S > 1024
ID_CASES = [ecase(B, S, 72, ids=i, pad=pad, rows=r, n_type=3 if r else 2)
            for (B, S) in ((9, 5), (2, 1025)) for i in ("repeat", "oob") for pad in (0, -1) for r in (False, True)]
CONST_CASES = [ecase(3, 5, 8, const=True), ecase(3, 5, 2048, const=True, twin="f16")]


def option_cases(form, n_type, tt):
    """The option cross of one backward form ("pos": (B, S) = (9, 5); "row": (1, 1025)) at H = 72 for one n_type / tt"""
    B, S = (9, 5) if form == "pos" else (1, 1025)
    return [ecase(B, S, 72, n_type=n_type, tt=tt, pad=pad, p=p, acc=acc, rows=rows, twin=twin)
            for pad in (0, 1, -1) for p in (0.0, 0.1) for acc in (False, True) for rows in (False, True)
            for twin in ("none", "f32", "f16")]


OPTION_AXES = [(form, n_type, tt) for form in ("pos", "row") for n_type in (1, 2, 3) for tt in ("given", "none", "oob")]


def rnd(*shape, seed, scale=1.0):
    return xc.rnd(*shape, seed=seed, scale=scale)


def embed_inputs(c):
    """CPU tensors of a case.  Table rows no token may legally read are NaN (word rows not among the clamped ids, type rows not
    among the clamped types, position rows from S on); ``pre`` holds the non-zero prefills of every gradient output."""
    B, S, H, nt = c["B"], c["S"], c["H"], c["n_type"]
    M = B * S
    g = torch.Generator().manual_seed(11 + B + 7 * S)
    if c["ids"] == "repeat":
        ids = torch.full((B, S), 3, dtype=torch.int64)
    else:
        ids = torch.randint(2, VOCAB - 2, (B, S), generator=g)
        ids[:, 1 % S] = 3
        if c["ids"] == "oob":
            ids[0, 0] = -3
            ids[-1, S - 1] = VOCAB + 2
            ids[0, S // 2] = -3 if S > 2 else ids[0, S // 2]
        elif c["pad"] >= 0:
            ids[0, 0] = c["pad"]
            ids[min(1, B - 1), S // 2] = c["pad"]
            if B >= 3:
                ids[B - 1] = c["pad"]
    tt = None
    if c["tt"] != "none":
        tt = torch.randint(0, nt, (B, S), generator=g)
        if c["tt"] == "oob":
            tt[0, 0] = -1
            tt[-1, S - 1] = nt
            tt[B // 2, S // 2] = nt if M > 2 else tt[B // 2, S // 2]
    npos = S if S > 1024 else S + 3
    word, pos, typ = rnd(VOCAB, H, seed=1), rnd(npos, H, seed=2, scale=0.5), rnd(nt, H, seed=3, scale=0.5)
    if c["const"]:          # dyadic constants: every sum of the row is exact, so mean == s and xhat == 0 in f32 too
        word = (torch.arange(VOCAB, dtype=F32) * 0.25)[:, None].expand(VOCAB, H).contiguous()
        pos = (torch.arange(npos, dtype=F32) * 0.5)[:, None].expand(npos, H).contiguous()
        typ = torch.arange(nt, dtype=F32)[:, None].expand(nt, H).contiguous()
    wi, pi, ti = clamped_rows(ids, tt, S, nt)
    for table, used in ((word, wi), (pos, pi), (typ, ti)):
        dead = torch.ones(table.shape[0], dtype=torch.bool)
        dead[used] = False
        table[dead] = float("nan")
    m = cpu_dropout_mask(M * H, c["p"], SEED).reshape(M, H)
    pre = {"dword": rnd(VOCAB, H, seed=21), "dpos": rnd(npos, H, seed=22), "dtype": rnd(nt, H, seed=23),
           "dgamma": rnd(H, seed=24), "dbeta": rnd(H, seed=25)}
    return dict(ids=ids, tt=tt, word=word, pos=pos, typ=typ, gamma=rnd(H, seed=4) + 1.0, beta=rnd(H, seed=5),
                dy=rnd(M, H, seed=6).to(BF16), m=m, pre=pre, npos=npos)


def clamped_rows(ids, tt, S, n_type):
    """``exact_check.embed_rows`` with the kernels' clamps: id into [0, vocab), token type into [0, n_type)"""
    wi, pi, ti = xc.embed_rows(ids, tt, S)
    return wi.clamp(0, VOCAB - 1), pi, ti.clamp(0, n_type - 1)


def embed_layout(c, inp):
    """-> per output row: is_prompt, word row, prompt row, position row, type row (the plain embedding: no prompt rows)"""
    wi, pi, ti = clamped_rows(inp["ids"], inp["tt"], c["S"], c["n_type"])
    return dict(isp=torch.zeros_like(wi, dtype=torch.bool), wi=wi, prow=torch.zeros_like(wi), pi=pi, ti=ti)


# ------------------------------------------------------------------------------------------------------- prompt cases
def pcase(B, S_in, P, H, off=0, pad=1, p=0.0, src="splice", acc=True):
    """One case of icka_embed_prompt_fwd + _bwd.  src: "splice" (oracle.cross_modal_oracle.splice_index) / "first" (prompt
    block first) / "last" / "reversed" (prompt rows in reverse order in the middle)."""
    return dict(B=B, S_in=S_in, P=P, H=H, off=off, pad=pad, p=p, src=src, acc=acc)


PROMPT_CASES = ([pcase(B, 21, 10, 264, off=off, pad=pad, p=p) for B in (1, 3, 9) for (off, pad, p) in ((0, 1, 0.0), (2, -1, 0.1))] +
                [pcase(9, 21, 10, H, off=2, p=0.1, acc=False) for H in (8, 2048)] +
                [pcase(3, 21, 1, 264, off=2), pcase(9, 1, 1, 8, src="first"), pcase(3, 1, 10, 264, off=2, src="last", p=0.1),
                 pcase(1, 1, 1, 2048, src="last", acc=False)] +
                [pcase(3, 21, 10, 264, off=off, src=s, pad=pad) for s in ("first", "last", "reversed") for (off, pad) in ((0, -1), (2, 1))])


def prompt_src(c):
    S_in, P = c["S_in"], c["P"]
    if c["src"] == "splice":
        from oracle.cross_modal_oracle import splice_index
        src = splice_index(S_in, P, (3, 11) if P % 2 == 0 else (3,))
    elif c["src"] == "first":
        src = [-1 - j for j in range(P)] + list(range(S_in))
    elif c["src"] == "last":
        src = list(range(S_in)) + [-1 - j for j in range(P)]
    else:
        src = list(range(S_in // 2)) + [-1 - j for j in reversed(range(P))] + list(range(S_in // 2, S_in))
    assert sorted(-1 - v for v in src if v < 0) == list(range(P)), "the contract: every prompt row exactly once"
    return torch.tensor(src, dtype=torch.int32)


def prompt_inputs(c):
    """As ``embed_inputs``; position rows outside [off, off + S) are NaN, and so is every word row no token names.  (Every
    prompt row is read by its own sample, so none can be NaN: a prompt row taken from the neighbouring sample shows as an
    error, the rows are independent random draws.)"""
    B, S_in, P, H, off = c["B"], c["S_in"], c["P"], c["H"], c["off"]
    src = prompt_src(c)
    S = src.numel()
    M = B * S
    g = torch.Generator().manual_seed(5 + B + S_in)
    ids = torch.randint(2, VOCAB - 2, (B, S_in), generator=g)
    ids[:, S_in // 2] = 3
    if c["pad"] >= 0:
        ids[0, 0] = c["pad"]
        ids[B - 1, S_in - 1] = c["pad"]
    npos = off + S + 2
    word, pos, typ = rnd(VOCAB, H, seed=1), rnd(npos, H, seed=2, scale=0.5), rnd(2, H, seed=3, scale=0.5)
    typ[1] = float("nan")                        # every row is type 0
    prompt = rnd(B, P, H, seed=7).to(BF16)
    isp, wid, prow, prw = xc.prompt_rows(ids, src, B, S_in, S, P, off)
    for table, used in ((word, wid[~isp]), (pos, prw)):
        dead = torch.ones(table.shape[0], dtype=torch.bool)
        dead[used] = False
        table[dead] = float("nan")
    m = cpu_dropout_mask(M * H, c["p"], SEED).reshape(M, H)
    pre = {"dword": rnd(VOCAB, H, seed=21), "dpos": rnd(npos, H, seed=22), "dtype": rnd(1, H, seed=23),     # dtype: row 0 only
           "dgamma": rnd(H, seed=24), "dbeta": rnd(H, seed=25)}
    return dict(ids=ids, src=src, prompt=prompt, word=word, pos=pos, typ=typ, gamma=rnd(H, seed=4) + 1.0, beta=rnd(H, seed=5),
                dy=rnd(M, H, seed=6).to(BF16), m=m, pre=pre, npos=npos, S=S)


def prompt_layout(c, inp):
    isp, wid, prow, prw = xc.prompt_rows(inp["ids"], inp["src"], c["B"], c["S_in"], inp["S"], c["P"], c["off"])
    return dict(isp=isp, wi=wid.clamp(0, VOCAB - 1), prow=prow, pi=prw, ti=torch.zeros_like(wid))


# ================================================================================================ references: forward
def fwd_refs(lay, word, pos, typ, prompt, gamma, beta, eps, m, twin=None):
    """(y, twin, xhat, rstd) of the embedding forward -- module docstring.  ``prompt`` bf16 [B P, H] or None; ``m`` the dropout
    multiplier [M, H]; ``twin`` None / F32 / F16."""
    w = _d(word)[lay["wi"]]
    if prompt is not None:
        w = torch.where(lay["isp"][:, None], _d(prompt).reshape(-1, w.shape[1])[lay["prow"]], w)
    p, t = _d(pos)[lay["pi"]], _d(typ)[lay["ti"]]
    r = kc.ln_fwd_bounds(w.abs() + p.abs() + t.abs(), (w + p) + t, gamma, beta, eps)
    y, e_y = r["y_raw"]
    yd = y * _d(m)
    e = _d(m) * e_y + U_ACC * yd.abs()
    out = {"y": (yd, stored(e, yd, BF16)), "xhat": r["xhat"], "rstd": r["rstd"]}
    if twin is not None:
        out["twin"] = (yd, stored(e, yd, twin))
    return out


# =============================================================================================== references: backward
def table_refs(ds, e_ds, index, keep, nrows, prefill):
    """table[index[r]] (+)= ds[r] over the rows with ``keep``: -> ((reference, bound), untouched rows [nrows] bool).
    prefill None: the table is overwritten (starts from zero)."""
    H = ds.shape[1]
    ref = torch.zeros(nrows, H, dtype=F64, device=ds.device) if prefill is None else _d(prefill).clone().reshape(nrows, H)
    ab = ref.abs()
    es = torch.zeros_like(ref)
    cnt = torch.zeros(nrows, dtype=F64, device=ds.device)
    ix = index[keep]
    ref.index_add_(0, ix, ds[keep])
    ab.index_add_(0, ix, ds[keep].abs())
    es.index_add_(0, ix, e_ds[keep])
    cnt.index_add_(0, ix, torch.ones(ix.numel(), dtype=F64, device=ds.device))
    return (ref, stored(es + (cnt[:, None] + 4) * U_ACC * ab, ref, F32)), cnt == 0


def bwd_refs(lay, dy, xhat, rstd, gamma, m, sizes, n_type, pad, accumulate, pre, rows=False, n_prompt=0):
    """Every output of icka_embed_bwd / _bwd_rows / _prompt_bwd from the SAVED xhat (bf16) and rstd -- module docstring.
    sizes = rows of (word, pos, type); pre = the prefills by name.  "untouched": {table: rows that must keep their prefill
    bitwise}; "dtok_zero": rows of dtok that are exact zeros; "dprompt": the [B P, H] reference gathered per prompt row."""
    dl = _d(dy) * _d(m)
    r = kc.ln_bwd_bounds(dl, xhat, rstd, gamma)
    ds, e_ds = r["ds_raw"]
    isp = lay["isp"]
    keep_w = ~isp & (lay["wi"] != pad)
    all_rows = torch.ones_like(isp)
    out, unt = {}, {}
    if rows:
        z = torch.zeros_like(ds)
        out["dtok"] = (torch.where(keep_w[:, None], ds, z), torch.where(keep_w[:, None], stored(e_ds, ds, F32), z))
        out["dtok_zero"] = ~keep_w
        unt["dword"] = torch.ones(sizes[0], dtype=torch.bool)
    else:
        out["dword"], unt["dword"] = table_refs(ds, e_ds, lay["wi"], keep_w, sizes[0], pre["dword"])
    out["dpos"], unt["dpos"] = table_refs(ds, e_ds, lay["pi"], all_rows, sizes[1], pre["dpos"])
    # dtype follows accumulate: slab slots + finalize for n_type <= 2, atomics onto a table cleared by the call beyond
    out["dtype"], unt_t = table_refs(ds, e_ds, lay["ti"], all_rows, sizes[2], pre["dtype"] if accumulate else None)
    if accumulate:
        unt["dtype"] = unt_t
    for name in ("dgamma", "dbeta"):
        ref, b = r[name]
        if accumulate:
            ref, b = with_beta(b, ref, 1.0, pre[name])
            b = stored(b, ref, F32)
        out[name] = (ref, b)
    if n_prompt:
        source = torch.full((n_prompt,), -1, dtype=torch.long)
        source[lay["prow"][isp]] = torch.nonzero(isp)[:, 0]
        assert bool((source >= 0).all())
        out["dprompt"] = (ds[source], stored(e_ds, ds, BF16)[source])
    out["untouched"] = unt
    return out


def scatter_rows_refs(rows, ids, vocab, pad, scale, prefill):
    """icka_embed_scatter_rows: dword[ids[t]] += scale * rows[t] (one rounding: u |scale row|), then the sum bound of
    ``table_refs``; ids equal to the padding id, negative or >= vocab are skipped (the ids AS GIVEN, no clamp)."""
    v = scale * _d(rows)
    keep = (ids != pad) & (ids >= 0) & (ids < vocab)
    return table_refs(v, U_ACC * v.abs(), ids.clamp(0, vocab - 1), keep, vocab, prefill)


SCATTER_CASES = [(T, H, bf, scale) for T in (1, 5, 4 * 4096 + 3) for H in (8, 72) for bf in (False, True) for scale in (1.0, 0.5)]


def scatter_inputs(T, H, bf):
    """rows of two "ranks" concatenated (T rows in all), ids that include the padding id 0, -1 and VOCAB"""
    t0 = T // 2
    rows = torch.cat([rnd(t0, H, seed=31), rnd(T - t0, H, seed=32)], 0)
    g = torch.Generator().manual_seed(33)
    ids = torch.randint(1, VOCAB - 1, (T,), generator=g)          # VOCAB - 1 is never named: that row stays untouched
    if T >= 5:
        ids[0], ids[2], ids[T - 1], ids[T // 2] = 0, -1, VOCAB, 0
    return (rows.to(BF16) if bf else rows), ids, rnd(VOCAB, H, seed=34)


def check_untouched(out, prefill, rows, what):
    """the rows ``rows`` of a table are bitwise the prefill"""
    if bool(rows.any()):
        same_bits(out.detach().cpu().reshape(prefill.shape)[rows].float(), prefill[rows].float(), what + ": untouched rows keep the prefill")


def compare_bwd(o, refs, pre, what):
    """every output of a backward in ``o`` against ``refs`` (bounds; then the bitwise parts)"""
    for name in ("dword", "dtok", "dpos", "dtype", "dgamma", "dbeta", "dprompt"):
        if name in refs and o.get(name) is not None:
            assert_within(o[name].reshape(refs[name][0].shape), refs[name][0], refs[name][1], "%s %s" % (what, name), verbose=False)
    for name, rows in refs["untouched"].items():
        if o.get(name) is not None:
            check_untouched(o[name], pre[name], rows, "%s %s" % (what, name))
    if "dtok" in refs:
        z = o["dtok"].detach().cpu()[refs["dtok_zero"]]
        assert not bool(z.view(torch.int32).ne(0).any()), "%s dtok: rows of the padding id are not exact zeros" % what


# ==================================================================================================== flat buffers
def chunk_ranges():
    """The element ranges of the flat-buffer cases: group 0 = one full chunk of 8192, a chunk of 8, a chunk of 8184; then a hole
    of 64 elements in no table; group 1 = 8192 + 40 elements right behind the hole (a full chunk and a short one).
    -> ([(lo, hi)] of group 0, [(lo, hi)] of group 1, total elements)"""
    g0 = [(0, 8192), (8192, 8200), (8200, 16384)]
    g1 = [(16448, 16448 + 8192 + 40)]
    return g0, g1, 16448 + 8192 + 40 + 24


def chunk_rows(ranges, group=None):
    rows = []
    for lo, hi in ranges:
        while lo < hi:
            n = min(OPT_CHUNK, hi - lo)
            rows.append((lo, n) if group is None else (lo, n, group))
            lo += n
    return rows


def in_chunks(rows, n):
    m = torch.zeros(n, dtype=torch.bool)
    for r in rows:
        m[r[0]:r[0] + r[1]] = True
    return m


def adam_inputs(n):
    """p, g, m, v with the planted elements: g = v = m = 0 (denominator eps), |p| = 7e4 (fp16 clamp), v = 1e-30, g = 1e4"""
    p, g, m = rnd(n, seed=41), rnd(n, seed=42, scale=0.1), rnd(n, seed=43, scale=0.1)
    v = rnd(n, seed=44, scale=0.1).abs() ** 2
    g[5] = v[5] = m[5] = 0.0
    p[9], p[8190] = 7e4, -7e4
    v[17] = 1e-30
    g[8300] = 1e4
    g[16383] = -1e4
    return p, g, m, v


def adamw_refs(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    """icka_optim_adamw in float64 from the f32 inputs (lr, b1, b2, eps, wd are the f32 values the kernel receives); u = 2^-24:
      gc    = g coef                                  u |gc|
      p1    = p (1 - lr wd)                           3 u |p1|        (lr wd, 1 - ., the product)
      m'    = b1 m + (1 - b1) gc                      4 u (|b1 m| + |(1 - b1) gc|)      (1 - b1, gc, two products, the add)
      v'    = b2 v + ((1 - b2) gc) gc                 6 u (|b2 v| + (1 - b2) gc^2)      (1 - b2, gc twice, three products, the add)
      den   = sqrt(v') / bc2_sqrt + eps               q (e_v / (2 (v' - e_v)) + 2^-22 + u + 2^-22) + u |den|,  q = sqrt(v') / bc2_sqrt
                                                      (sqrtf, the f32 value of bc2_sqrt, the division; the add)
      ratio = m' / den                                e_m / den + |m'| e_den / (den (den - e_den)) + 2^-22 |ratio|
      upd   = (lr / bc1) ratio                        step e_ratio + (2^-22 + 2 u) |upd|    (bc1 in f32, lr / bc1, the product)
      p'    = p1 - upd                                e_p1 + e_upd + u (|p1| + |upd|)
    each stored in f32.  -> {"p", "m", "v"}"""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    gc = g * coef
    p1 = p * (1.0 - lr * wd)
    e_p1 = 3 * U * p1.abs()
    tm1, tm2 = b1 * m, (1.0 - b1) * gc
    m2 = tm1 + tm2
    e_m = 4 * U * (tm1.abs() + tm2.abs())
    tv1, tv2 = b2 * v, (1.0 - b2) * gc * gc
    v2 = tv1 + tv2
    e_v = 6 * U * (tv1.abs() + tv2.abs())
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    q = torch.sqrt(v2) / bc2s
    r_sqrt = torch.where(v2 > 0, e_v / (2 * (v2 - e_v)).clamp_min(1e-300), torch.zeros_like(v2))
    den = q + eps
    e_den = q * (r_sqrt + 2 * DIV_REL + U) + U * den.abs()
    ratio = m2 / den
    e_ratio = e_m / den + m2.abs() * e_den / (den * (den - e_den)) + DIV_REL * ratio.abs()
    st = lr / bc1
    upd = st * ratio
    e_upd = st * e_ratio + (DIV_REL + 2 * U) * upd.abs()
    p2 = p1 - upd
    e_p = e_p1 + e_upd + U * (p1.abs() + upd.abs())
    return {"p": (p2, stored(e_p, p2, F32)), "m": (m2, stored(e_m, m2, F32)), "v": (v2, stored(e_v, v2, F32))}


def shadow_bf16(p):
    return p.to(BF16)


def shadow_f16(p):
    return p.clamp(-FP16_MAX, FP16_MAX).to(F16)


def sqnorm_refs(g, rows):
    """icka_optim_sqnorm: partials[b] = sum g^2 over chunk b, an f32 sum of len squares in any order: (len + 4) u sum g^2"""
    ref = torch.stack([(_d(g[lo:lo + n]) ** 2).sum() for lo, n in rows])
    ln = torch.tensor([n for _, n in rows], dtype=F64)
    return {"partials": (ref, stored((ln + 4) * U_ACC * ref, ref, F32))}


def clip_refs(partials, max_norm):
    """icka_optim_clip / _prepare from the partials THE KERNEL produced: norm = f32(sqrt(float64 sum)) -- the float64 sum of n
    f32 values in any order is off by at most n 2^-53 of it, the sqrt halves a relative error, the conversion rounds once;
    coef = min(1, max_norm / (norm + 1e-6)) evaluated in f32 FROM THE KERNEL'S norm (``clip_coef``), 1 for max_norm <= 0."""
    s = _d(partials).sum()
    n = partials.numel()
    norm = torch.sqrt(s)
    return {"norm": (norm, stored(norm * n * 2.0 ** -53, norm, F32))}


def clip_coef(norm_f32, max_norm):
    """-> (coefficient in f32 from the f32 norm the kernel stored, bound: one f32 add and one division, u + 2^-22 relative)"""
    if max_norm <= 0:
        return torch.tensor(1.0, dtype=F64), 0.0
    c = torch.tensor(max_norm, dtype=F32) / (norm_f32.float().cpu().reshape(()) + torch.tensor(1e-6, dtype=F32))
    c = torch.minimum(c, torch.tensor(1.0))
    return c.double(), float(c) * (DIV_REL + U_ACC)


CLIP_N = (1, 3, 1024, 1025, 2049)
CAST_BACK_N = (1, 7, 8, 9, 2 ** 24 + 13)           # the last beyond 8192 * 256 * 8: the grid-stride loop
CAST_SCALES = (1.0, 1.0 / 8, 1.0 / 3)
COPY_BYTES = (0, 1, 15, 16, 17, 4096, 65536 + 2, 1 << 20)
ZERO_N = (1, 3, 4, 5, 1000003, 4096 * 256 * 4 + 5)   # the last beyond one pass of the capped grid (4096 blocks x 256 x 16 bytes)


def cast_inputs(n):
    """f32 source with +-inf, NaN, -0.0 and the value halfway between two bf16 numbers planted (ties to even, both ways)"""
    x = rnd(n, seed=51)
    for i, val in enumerate((float("inf"), float("-inf"), float("nan"), -0.0)):
        x[3 + 2 * i] = val
    bits = x.view(torch.int32)
    bits[12] = 0x3F808000          # 1 + 2^-8: halfway, the even neighbour is below
    bits[13] = 0x3F818000          # halfway, the even neighbour is above
    bits[8193] = 0x3F808000
    return x


def cast_back_ref(src_bf16, scale):
    """bf2f(x) * scale as ONE f32 product (on the device of the source)"""
    return src_bf16.float() * torch.tensor(scale, dtype=F32, device=src_bf16.device)


def same_bytes(dst, src, what):
    """bitwise equality of two uint8 tensors: a copy against its source"""
    dst, src = dst.detach().cpu().reshape(-1), src.detach().cpu().reshape(-1)
    assert dst.dtype == torch.uint8 and src.dtype == torch.uint8 and dst.shape == src.shape, (what, tuple(dst.shape), tuple(src.shape))
    ne = dst != src
    assert not bool(ne.any()), "%s: %d of %d bytes differ, first at %d" % (what, int(ne.sum()), ne.numel(), int(ne.int().argmax()))


def copy_sources(sizes, shift=0):
    """uint8 sources of the copy_many cases (``shift`` more bytes in front: the pointers moved off their alignment)"""
    g = torch.Generator().manual_seed(81)
    return [torch.randint(0, 256, (nb + shift,), dtype=torch.uint8, generator=g) for nb in sizes]
