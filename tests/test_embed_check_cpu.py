"""CPU: keeps tests/embed_check.py honest.  For the three embedding kernels of csrc/layernorm.hip and for the flat-buffer
kernels a plain torch-f32 emulation performs the kernel's operations in the kernel's own summation structure (per-lane
chunks of 8, the wave sum, the wave loop over the batch and the 8-wave block reduction of the position-major backward, the
4-wave slab flush of the row-major one, finalize_kernel's 16 slab lanes, the atomics in an arbitrary but fixed order); at
every case tests/test_embed_elements_gpu.py runs on the device it must stay inside every bound, and so must the reference
itself.  Then seeded faults, one at a time: each must leave a bound or break a bitwise check -- a fault that stays inside
means the shapes or the bound are too weak to trust the GPU test.  Last, the references are tied to torch: layer_norm and
autograd in float64 through the gathered sum, torch.optim.AdamW in float64."""
import math

import pytest
import torch

import embed_check as ec
import kernel_check as kc
from embed_check import BF16, F16, F32, VOCAB, EPS_LN
from test_head_check_cpu import wave_sum

F64 = torch.float64


def caught(fn):
    """the check fails (a bound is left or a bitwise comparison breaks)"""
    try:
        fn()
    except AssertionError:
        kc._PENDING.clear()
        return True
    kc._PENDING.clear()
    return False


# ---------------------------------------------------------------------------------------- the kernels' summation forms
def lane_sum(x):
    """[M, H] -> [M, 64]: lane l owns the chunks of 8 columns l, l + 64, ..; it adds their elements in order"""
    M, H = x.shape
    nch = H // 8
    n = (nch + 63) // 64
    pad = torch.zeros(M, n * 64, 8, dtype=F32)
    pad[:, :nch] = x.reshape(M, nch, 8)
    pad = pad.reshape(M, n, 64, 8)
    acc = torch.zeros(M, 64, dtype=F32)
    for i in range(n):
        for e in range(8):
            acc = acc + pad[:, i, :, e]
    return acc


def row_sum(x):
    return wave_sum(lane_sum(x))


def strided_seq(x, stride):
    """[N, ..] -> [stride, ..]: out[k] = ((x[k] + x[k + stride]) + x[k + 2 stride]) + .. from 0 (a loop that strides over rows)"""
    N = x.shape[0]
    trips = -(-N // stride)
    pad = torch.zeros((trips * stride,) + tuple(x.shape[1:]), dtype=F32)
    pad[:N] = x
    pad = pad.reshape((trips, stride) + tuple(x.shape[1:]))
    acc = torch.zeros_like(pad[0])
    for t in range(trips):
        acc = acc + pad[t]
    return acc


def seq(x):
    """sum over the first axis in order, from 0"""
    acc = torch.zeros_like(x[0])
    for k in range(x.shape[0]):
        acc = acc + x[k]
    return acc


def finalize(partials, prefill, accumulate):
    """finalize_kernel: [nslab, H] -> [H]: 16 slab lanes, each b = sy, sy + 16, .., then red[0] + .. + red[15] from 0"""
    t = seq(strided_seq(partials, 16))
    return prefill + t if accumulate else t


def atomics(table, index, rows, keep, seed=3):
    """f32 atomics onto ``table`` in an arbitrary but fixed order"""
    perm = torch.randperm(index.numel(), generator=torch.Generator().manual_seed(seed))
    perm = perm[keep[perm]]
    for r in perm.tolist() if perm.numel() < 64 else ():
        table[index[r]] = table[index[r]] + rows[r]
    if perm.numel() >= 64:
        table.index_add_(0, index[perm], rows[perm])
    return table


# ------------------------------------------------------------------------------------------------------- emulations
def emu_fwd(lay, inp, eps, twin, prompt=None, fault=None, raw=None):
    H = inp["word"].shape[1]
    wi, pi, ti = lay["wi"], lay["pi"], lay["ti"]
    if fault == "pos_no_offset":
        pi = pi - raw["off"]
    if fault == "tt_ignored":
        ti = torch.zeros_like(ti)
    if fault == "id_unclamped":          # a row outside the table: some other memory -- here some other row
        wi = raw["ids"] % VOCAB
    w = inp["word"][wi]
    if prompt is not None:
        w = torch.where(lay["isp"][:, None], prompt.float().reshape(-1, H)[lay["prow"]], w)
    s = (w + inp["pos"][pi]) + inp["typ"][ti]
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    mean = row_sum(s) * inv_h
    d = s - mean[:, None]
    rstd = 1.0 / torch.sqrt(row_sum(d * d) * inv_h + torch.tensor(eps, dtype=F32))
    xh = d * rstd[:, None]
    m = inp["m"]
    if fault == "drop_wrong_H":
        M = s.shape[0]
        m = ec.cpu_dropout_mask(M * (H + 8), raw["p"], ec.SEED).reshape(M, H + 8)[:, :H]
    o = (inp["gamma"] * xh + inp["beta"]) * m
    out = {"y": o.to(BF16), "xhat": xh.to(BF16), "rstd": rstd}
    if twin is not None:
        out["twin"] = o.clamp(-ec.FP16_MAX, ec.FP16_MAX).to(F16) if twin == F16 else o
    return out


def emu_bwd(lay, inp, xhat, rstd, B, S, n_type, pad, accumulate, rows, off=0, P=0, fault=None):
    M, H = xhat.shape
    pre = inp["pre"]
    xh, g = xhat.float(), inp["gamma"]
    dl = inp["dy"].float() * inp["m"]
    gd = g * dl
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    c1, c2 = row_sum(gd) * inv_h, row_sum(gd * xh) * inv_h
    ds = rstd[:, None] * (gd - c1[:, None] - xh * c2[:, None])
    ti, wi, pi, isp = lay["ti"], lay["wi"], lay["pi"], lay["isp"]
    live = torch.ones(M, 1, dtype=F32)
    if fault == "batch_row_dropped":     # the wave loop stops after its first trip: batch rows b >= 8 contribute nothing
        live = (torch.arange(M) // S < 8).float()[:, None]
    z = torch.zeros_like(ds)
    cols = [dl * xh * live, dl * live, torch.where((ti == 0)[:, None], ds, z) * live, torch.where((ti == 1)[:, None], ds, z) * live]
    keep_w = ~isp & ((wi != pad) | (fault == "pad_row_grad")) & (live[:, 0] > 0)
    dsw = ds
    if fault == "dword_chunk_dropped":
        dsw = ds.clone()
        dsw[int(torch.nonzero(keep_w)[0, 0]), 8 * (H // 16):8 * (H // 16) + 8] = 0.0
    out = {}
    dpos = pre["dpos"].clone()
    if S <= 1024:                        # position-major: one block per position, 8 waves walk the batch
        blk = lambda x: seq(strided_seq(x.reshape(B, S, H), 8))          # [S, H]
        parts = [blk(x) for x in cols]
        dpos[off:off + S] = dpos[off:off + S] + blk(ds * live)
    else:                                # row-major: wave wid takes rows wid, wid + nw, ..; 4 waves flush one slab
        grid = min(1024, (M + 3) // 4)
        parts = [seq(strided_seq(x, 4 * grid).reshape(grid, 4, H).transpose(0, 1)) for x in cols]
        atomics(dpos, pi, ds, live[:, 0] > 0, seed=5)
    out["dpos"] = dpos
    acc_g = accumulate and fault != "dgamma_no_acc"
    out["dgamma"] = finalize(parts[0], pre["dgamma"], acc_g)
    out["dbeta"] = finalize(parts[1], pre["dbeta"], accumulate)
    if n_type <= 2:
        out["dtype"] = torch.stack([finalize(parts[2 + k], pre["dtype"][k], accumulate) for k in range(n_type)])
    else:
        start = pre["dtype"].clone() if (accumulate or fault == "dtype_acc_n3") else torch.zeros_like(pre["dtype"])
        out["dtype"] = atomics(start, ti, ds, live[:, 0] > 0, seed=7)
    if rows:
        out["dtok"] = torch.where((keep_w | (fault == "dtok_pad_nonzero"))[:, None], ds, z)
    else:
        out["dword"] = atomics(pre["dword"].clone(), wi, dsw, keep_w)
    if P:
        dp = torch.zeros(B * P, H, dtype=BF16)
        src_rows = torch.nonzero(isp)[:, 0]
        dst = lay["prow"][isp]
        if fault == "dprompt_neighbour":
            dst = (dst + P) % (B * P)
        dp[dst] = ds[src_rows].to(BF16)
        out["dprompt"] = dp
    return out


def _embed_check(c, fault=None, prompt=False):
    if prompt:
        inp = ec.prompt_inputs(c)
        lay = ec.prompt_layout(c, inp)
        B, S, nt, pad, acc, rows, off, P, eps, tw = c["B"], inp["S"], 1, c["pad"], c["acc"], False, c["off"], c["P"], 1e-5, F32
        raw = {"off": off, "p": c["p"], "ids": lay["wi"]}
        sizes = (VOCAB, inp["npos"], 1)
    else:
        inp = ec.embed_inputs(c)
        lay = ec.embed_layout(c, inp)
        B, S, nt, pad, acc, rows, off, P, eps = c["B"], c["S"], c["n_type"], c["pad"], c["acc"], c["rows"], 0, 0, EPS_LN
        tw = {"none": None, "f32": F32, "f16": F16}[c["twin"]]
        raw = {"off": 0, "p": c["p"], "ids": inp["ids"].reshape(-1)}
        sizes = (VOCAB, inp["npos"], nt)
    pr, m_true = inp.get("prompt"), inp["m"]
    rf = ec.fwd_refs(lay, inp["word"], inp["pos"], inp["typ"], pr, inp["gamma"], inp["beta"], eps, inp["m"], tw)
    o = emu_fwd(lay, inp, eps, tw, pr, fault, raw)
    what = "cpu embed_prompt" if prompt else "cpu embed"
    for name in ("y", "twin", "xhat", "rstd"):
        if name in o:
            kc.assert_within(o[name], rf[name][0], rf[name][1], "%s %s" % (what, name), verbose=False)
            # the reference itself, rounded to the output's format, satisfies its bound
            kc.assert_within(rf[name][0].to(o[name].dtype), rf[name][0], rf[name][1], "%s %s (reference)" % (what, name), verbose=False)
    if c.get("const"):
        assert not bool(o["xhat"].float().ne(0).any()) and torch.equal(o["y"], inp["beta"].to(BF16)[None].expand_as(o["y"]))
    # backward from the emulation's own saved xhat / rstd, as the device test does from the kernel's
    if fault in ("pos_no_offset", "tt_ignored", "id_unclamped"):
        return
    if fault == "drop_wrong_H_bwd":          # a clean forward, then the backward with the mask indexed with the wrong H
        M, H = o["y"].shape
        inp = dict(inp, m=ec.cpu_dropout_mask(M * (H + 8), raw["p"], ec.SEED).reshape(M, H + 8)[:, :H])
    rb = ec.bwd_refs(lay, inp["dy"], o["xhat"], o["rstd"], inp["gamma"], m_true,
                     sizes, nt, pad, acc, inp["pre"], rows=rows, n_prompt=B * P)
    ob = emu_bwd(lay, inp, o["xhat"], o["rstd"], B, S, nt, pad, acc, rows, off, P, fault)
    ec.compare_bwd(ob, rb, inp["pre"], what)
    if fault is None:
        ref_as_out = {k: (v[0].to(BF16 if k == "dprompt" else F32)) for k, v in rb.items() if isinstance(v, tuple)}
        ec.compare_bwd(ref_as_out, rb, inp["pre"], what + " (reference)")


ALL_PLAIN = ec.SHAPE_CASES + ec.ID_CASES + ec.CONST_CASES


@pytest.mark.parametrize("c", ALL_PLAIN, ids=ec.case_id)
def test_embed_emulation_inside_at_every_shape_case(c):
    _embed_check(c)
    kc.report("cpu embed " + ec.case_id(c))


@pytest.mark.parametrize("form,n_type,tt", ec.OPTION_AXES)
def test_embed_emulation_inside_at_every_option_case(form, n_type, tt):
    for c in ec.option_cases(form, n_type, tt):
        _embed_check(c)
    kc.report("cpu embed options %s n_type=%d tt=%s" % (form, n_type, tt))


@pytest.mark.parametrize("c", ec.PROMPT_CASES, ids=ec.case_id)
def test_prompt_emulation_inside(c):
    _embed_check(c, prompt=True)
    kc.report("cpu embed_prompt " + ec.case_id(c))


def test_embed_seeded_faults_are_caught():
    """each fault at cases the GPU test runs (the first of them that can show it)"""
    pos9, row9 = ec.ecase(9, 5, 72), ec.ecase(9, 1025, 72)
    pr = ec.pcase(3, 21, 10, 264, off=2, pad=-1, p=0.1)
    assert pr in ec.PROMPT_CASES and pos9 in ec.SHAPE_CASES and row9 in ec.SHAPE_CASES
    assert caught(lambda: _embed_check(pr, "pos_no_offset", prompt=True)), "position row sp in place of sp + pos_offset"
    for c in (ec.ecase(9, 5, 72, n_type=2, tt="given", pad=0, p=0.0, acc=False, rows=False, twin="none"), row9):
        assert caught(lambda: _embed_check(c, "tt_ignored")), "tt ignored"
    oob = [c for c in ec.ID_CASES if c["ids"] == "oob"]
    for c in oob[:2] + oob[-2:]:
        assert caught(lambda: _embed_check(c, "id_unclamped")), "id not clamped"
    for c in (pos9, row9, ec.ecase(9, 5, 2048)):
        assert caught(lambda: _embed_check(c, "dword_chunk_dropped")), "a chunk of 8 columns of one row dropped from dword"
        assert caught(lambda: _embed_check(c, "batch_row_dropped")), "batch row 8 dropped"
        assert caught(lambda: _embed_check(c, "pad_row_grad")), "the padding row received gradient"
    # (a lost prefill of size 1 shows where the (M + 4) u sum|dl xhat| of the column sum is below it: M = 1025, not M = 9225)
    for c in (pos9, ec.ecase(1, 1025, 72), ec.ecase(9, 5, 2048)):
        assert c in ec.SHAPE_CASES
        assert caught(lambda: _embed_check(c, "dgamma_no_acc")), "accumulate ignored for dgamma"
    for c in (ec.ecase(9, 5, 2048, rows=True, p=0.1, twin="f16"), ec.ecase(5, 1025, 72, rows=True)):
        assert c in ec.SHAPE_CASES
        assert caught(lambda: _embed_check(c, "dtok_pad_nonzero")), "dtok of a padding id non-zero"
    for form in ("pos", "row"):
        cs = [c for c in ec.option_cases(form, 3, "given") if not c["acc"]]
        assert caught(lambda: _embed_check(cs[0], "dtype_acc_n3")), "dtype accumulated with accumulate = 0, n_type = 3"
        cs = [c for c in ec.option_cases(form, 2, "given") if c["p"] > 0]
        assert caught(lambda: _embed_check(cs[0], "drop_wrong_H")), "dropout mask indexed with the wrong H (forward)"
        assert caught(lambda: _embed_check(cs[0], "drop_wrong_H_bwd")), "dropout mask indexed with the wrong H (backward)"
    assert caught(lambda: _embed_check(pr, "dprompt_neighbour", prompt=True)), "dprompt from the neighbouring sample"
    assert caught(lambda: _embed_check(pr, "drop_wrong_H", prompt=True))
    assert caught(lambda: _embed_check(pr, "drop_wrong_H_bwd", prompt=True))


@pytest.mark.parametrize("T,H,bf,scale", ec.SCATTER_CASES)
def test_scatter_rows_emulation_inside_and_faults_outside(T, H, bf, scale):
    rows, ids, pre = ec.scatter_inputs(T, H, bf)
    ref, unt = ec.scatter_rows_refs(rows, ids, VOCAB, 0, scale, pre)

    def run(fault=None):
        keep = (ids != 0) & (ids >= 0) & (ids < VOCAB)
        if fault == "pad":
            keep = (ids >= 0) & (ids < VOCAB)
        if fault == "oob":
            keep = ids != 0
        out = atomics(pre.clone(), ids.clamp(0, VOCAB - 1), torch.tensor(scale, dtype=F32) * rows.float(), keep)
        kc.assert_within(out, ref[0], ref[1], "cpu scatter_rows dword", verbose=False)
        ec.check_untouched(out, pre, unt, "cpu scatter_rows")

    run()
    kc.assert_within(ref[0].float(), ref[0], ref[1], "cpu scatter_rows (reference)", verbose=False)
    if T >= 5:
        assert caught(lambda: run("pad")) and caught(lambda: run("oob"))
    kc.report("cpu scatter_rows")


# ----------------------------------------------------------------------------------------------------- flat buffers
def emu_adamw(p, g, m, v, coef, lr, b1, b2, eps, wd, step, fault=None):
    f = lambda x: torch.tensor(x, dtype=F32)
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    bc1 = f(1.0 - float(b1) ** step)
    bc2s = f(math.sqrt(1.0 - float(b2) ** step))
    if fault == "bc2_sqrt_squared":
        bc2s = bc2s * bc2s
    st, decay = lr / bc1, 1.0 - lr * wd
    gc = g * f(coef)
    p1 = p if fault == "decay_after_step" else p * decay
    m2 = b1 * m + (1.0 - b1) * gc
    v2 = b2 * v + (1.0 - b2) * gc * gc
    p2 = p1 - st * (m2 / (torch.sqrt(v2) / bc2s + eps))
    if fault == "decay_after_step":
        p2 = p2 * decay
    return p2, m2, v2


@pytest.mark.parametrize("with_coef", (True, False))
@pytest.mark.parametrize("lr", (0.0, 1e-2))
@pytest.mark.parametrize("wd", (0.0, 0.01))
@pytest.mark.parametrize("step", (1, 1000))
def test_adamw_emulation_inside_and_faults_outside(step, wd, lr, with_coef):
    r0, r1, n = ec.chunk_rows(ec.chunk_ranges()[0]), ec.chunk_rows(ec.chunk_ranges()[1]), ec.chunk_ranges()[2]
    p, g, m, v = ec.adam_inputs(n)
    f32 = lambda x: float(torch.tensor(x, dtype=F32))
    coef = 7.3e-5 if with_coef else 1.0
    args = (f32(coef), f32(lr), f32(0.9), f32(0.999), f32(1e-8), f32(wd), step)
    # group 0 (the three chunks in front of the hole, with the weight decay) and group 1 (right behind the hole, wd = 0), as
    # the device test runs them
    for rr, wd_g in ((r0, wd), (r1, 0.0)):
        _adamw_group(p, g, m, v, ec.in_chunks(rr, n), args[:5] + (f32(wd_g), step), lr, wd_g, last8=rr[0][1])
    kc.report("cpu adamw")


def _adamw_group(p, g, m, v, mk, args, lr, wd, last8):
    ref = ec.adamw_refs(p[mk], g[mk], m[mk], v[mk], *args)
    big = torch.nonzero(p[mk].abs() > ec.FP16_MAX)[:, 0]

    def run(fault=None):
        o = dict(zip("pmv", emu_adamw(p[mk], g[mk], m[mk], v[mk], *args, fault=fault)))
        if fault == "chunk_last8_skipped":
            for name, orig in (("p", p), ("m", m), ("v", v)):
                o[name][last8 - 8:last8] = orig[mk][last8 - 8:last8]
        for name in "pmv":
            kc.assert_within(o[name], ref[name][0], ref[name][1], "cpu adamw " + name, verbose=False)
        sh = ec.shadow_bf16(p[mk] if fault == "shadow_old_p" else o["p"])
        ec.same_bits(sh.float(), ec.shadow_bf16(o["p"]).float(), "bf16 shadow")
        assert bool((ec.shadow_f16(o["p"])[big].float().abs() == ec.FP16_MAX).all())

    run()
    for name in "pmv":
        kc.assert_within(ref[name][0].float(), ref[name][0], ref[name][1], "cpu adamw %s (reference)" % name, verbose=False)
    if lr > 0:
        if wd > 0:
            assert caught(lambda: run("decay_after_step")), "the decay applied after the step"
        # (bc2_sqrt is 0.03 at step 1 and 0.8 at step 1000: its square moves the denominator visibly at both)
        assert caught(lambda: run("bc2_sqrt_squared")), "bc2_sqrt squared"
        assert caught(lambda: run("shadow_old_p")), "the shadow taken from the old p"
    assert caught(lambda: run("chunk_last8_skipped")), "a chunk's last 8 elements skipped"


def test_sqnorm_clip_cast_and_copy_helpers():
    n = ec.chunk_ranges()[2]
    rows = ec.chunk_rows(ec.chunk_ranges()[0]) + ec.chunk_rows(ec.chunk_ranges()[1])
    _, g, _, _ = ec.adam_inputs(n)
    ref = ec.sqnorm_refs(g, rows)["partials"]
    # optim_sqnorm_kernel: 4 elements per thread and trip, the wave sum, (red0 + red1) + (red2 + red3)
    parts = []
    for lo, k in rows:
        x = torch.zeros(-(-k // 1024) * 1024, dtype=F32)
        x[:k] = g[lo:lo + k]
        x = x.reshape(-1, 256, 4)
        s = torch.zeros(256, dtype=F32)
        for t in range(x.shape[0]):
            s = s + (((x[t, :, 0] * x[t, :, 0] + x[t, :, 1] * x[t, :, 1]) + x[t, :, 2] * x[t, :, 2]) + x[t, :, 3] * x[t, :, 3])
        r = wave_sum(s.reshape(4, 64))
        parts.append((r[0] + r[1]) + (r[2] + r[3]))
    parts = torch.stack(parts)
    kc.assert_within(parts, ref[0], ref[1], "cpu sqnorm partials", verbose=False)
    short = parts.clone()
    short[1] = short[1] - g[8192 + 4:8200].pow(2).sum()
    assert caught(lambda: kc.assert_within(short, ref[0], ref[1], "cpu sqnorm, half a chunk of 8 lost", verbose=False))
    for k in ec.CLIP_N:
        vals = ec.rnd(k, seed=61).abs() + 0.01
        rn = ec.clip_refs(vals, 1.0)["norm"]
        norm = torch.sqrt(seq(vals.double())).float()
        kc.assert_within(norm.reshape(1), rn[0].reshape(1), rn[1].reshape(1), "cpu clip norm", verbose=False)
        if k > 1024:          # the stride loop stopping after one trip
            lost = torch.sqrt(vals[:1024].double().sum()).float()
            assert caught(lambda: kc.assert_within(lost.reshape(1), rn[0].reshape(1), rn[1].reshape(1), "cpu clip, one trip", verbose=False))
        cr = ec.clip_coef(norm, 1.0)[0]
        assert float(cr) == float(min(torch.tensor(1.0), torch.tensor(1.0) / (norm + torch.tensor(1e-6))))
        assert float(ec.clip_coef(norm, 0.0)[0]) == 1.0 and float(ec.clip_coef(norm, -1.0)[0]) == 1.0
    # dp_cast_back_kernel over a sentinel destination: a body of 8 elements per thread, then the tail of n & 7
    def cast_back(x, scale, skip_tail=False):
        k = x.numel()
        out = torch.full((k,), kc.SENTINEL[F32], dtype=torch.int32).view(F32)
        body = k >> 3 << 3
        sc = torch.tensor(scale, dtype=F32)
        for c in range(0, body, 8):
            out[c:c + 8] = x[c:c + 8].float() * sc
        if not skip_tail:
            out[body:] = x[body:].float() * sc
        return out

    for k in ec.CAST_BACK_N[:4]:
        x = ec.rnd(k, seed=71).to(BF16)
        for scale in ec.CAST_SCALES:
            ref = ec.cast_back_ref(x, scale)
            ec.same_bits(cast_back(x, scale), ref, "cast_back")
            if k & 7:
                assert caught(lambda: ec.same_bits(cast_back(x, scale, skip_tail=True), ref, "cast_back")), "the tail of n & 7 skipped"
    # copy_many_kernel over a sentinel destination: 16-byte words on the vector path, bytes otherwise
    def copy(src, fault=None):
        nb = src.numel()
        dst = torch.full((nb,), kc.SENTINEL[torch.uint8], dtype=torch.uint8)
        k = (nb >> 4 << 4) if (nb & 15) == 0 or fault == "byte_path_truncated" else nb
        dst[:k] = src[:k]
        return dst

    for src in ec.copy_sources(ec.COPY_BYTES):
        ec.same_bytes(copy(src), src, "copy_many")
        if src.numel() & 15:
            assert caught(lambda: ec.same_bytes(copy(src, "byte_path_truncated"), src, "copy_many")), \
                "copy_many copying nb >> 4 << 4 bytes on the byte path (%d bytes)" % src.numel()
    assert len(ec.COPY_BYTES) == 8 and sum(1 for nb in ec.COPY_BYTES if nb & 15) == 4
    x = ec.cast_inputs(n)
    b = x.to(BF16).view(torch.int16)
    assert int(b[12]) == 0x3F80 and int(b[13]) == 0x3F82 and int(b[9]) == -32768 and int(b[3]) == 0x7F80
    kc.report("cpu flat buffers")


# ------------------------------------------------------------------------------- the references against torch's own
def test_references_equal_torch_float64():
    c = ec.ecase(3, 5, 72, n_type=3, tt="oob", pad=1, p=0.1, acc=True)
    inp = ec.embed_inputs(c)
    lay = ec.embed_layout(c, inp)
    nan0 = lambda t: torch.nan_to_num(t, nan=0.0)
    word, pos, typ = (nan0(inp[k]).double().requires_grad_() for k in ("word", "pos", "typ"))
    gamma, beta = inp["gamma"].double().requires_grad_(), inp["beta"].double().requires_grad_()
    s = word[lay["wi"]] + pos[lay["pi"]] + typ[lay["ti"]]
    y = torch.nn.functional.layer_norm(s, (72,), gamma, beta, EPS_LN) * inp["m"].double()
    rf = ec.fwd_refs(lay, inp["word"], inp["pos"], inp["typ"], None, inp["gamma"], inp["beta"], EPS_LN, inp["m"], F32)
    assert float((rf["y"][0] - y.detach()).abs().max()) < 1e-12
    # the backward reference starts from SAVED xhat / rstd: give it the exact ones (as float64) to compare with autograd
    mean, var = s.mean(-1, keepdim=True), s.var(-1, unbiased=False, keepdim=True)
    rstd = (1.0 / torch.sqrt(var + EPS_LN)).detach()
    xhat = ((s - mean) * rstd).detach()
    y.backward(inp["dy"].double())
    zero = {k: torch.zeros_like(v) for k, v in inp["pre"].items()}
    rb = ec.bwd_refs(lay, inp["dy"], xhat, rstd[:, 0], inp["gamma"], inp["m"], (VOCAB, inp["npos"], 3), 3, -1, True, zero)
    for name, t in (("dword", word.grad), ("dpos", pos.grad), ("dtype", typ.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        assert float((rb[name][0] - t.reshape(rb[name][0].shape)).abs().max()) < 1e-11, name
    # AdamW
    n = 64
    p, g, m, v = ec.adam_inputs(16384 + 8256)
    p, g, m, v = p[:n].double(), g[:n].double(), m[:n].double(), v[:n].double()
    q = p.clone().requires_grad_()
    opt = torch.optim.AdamW([q], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.state[q] = {"step": torch.tensor(6.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g * 0.5
    opt.step()
    ref = ec.adamw_refs(p, g, m, v, 0.5, 1e-2, 0.9, 0.999, 1e-8, 0.01, 7)
    for name, t in (("p", q.detach()), ("m", opt.state[q]["exp_avg"]), ("v", opt.state[q]["exp_avg_sq"])):
        rel = ((ref[name][0] - t).abs() / t.abs().clamp_min(1e-30)).max()
        assert float(rel) < 1e-12, (name, float(rel))
