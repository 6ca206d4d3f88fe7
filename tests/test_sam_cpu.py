"""CPU: the host side of icka_amd.SAM -- the float64 oracle of tests/sam_oracle.py against an independent float64 torch
implementation of the published two-step procedure (Foret et al. 2021; Kwon et al. 2021) on a small nn.Linear, the oracle's
skip rule and bars, the refusals that need no device, and the ctypes mirror of icka_sam_state against the header's struct."""
import os
import types

import numpy as np
import pytest
import torch

import sam_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _published_step(lin, x, y, rho, adaptive):
    """The two-step procedure as the papers state it, per tensor, in float64 torch: gradient at w, the perturbation, the gradient
    at w + e.  Returns (params, first gradients, perturbations, second gradients, losses)."""
    params = [lin.weight, lin.bias]
    loss = torch.nn.functional.mse_loss(lin(x), y)
    grads = torch.autograd.grad(loss, params)
    if adaptive:       # ASAM: e = rho T^2 g / ||T g||, T = |w| element-wise
        norm = torch.sqrt(sum(((p.abs() * g) ** 2).sum() for p, g in zip(params, grads)))
        eps = [rho * p.abs() ** 2 * g / (norm + 1e-12) for p, g in zip(params, grads)]
    else:              # SAM: e = rho g / ||g||
        norm = torch.sqrt(sum((g ** 2).sum() for g in grads))
        eps = [rho * g / (norm + 1e-12) for g in grads]
    with torch.no_grad():
        for p, e in zip(params, eps):
            p.add_(e)
    loss2 = torch.nn.functional.mse_loss(lin(x), y)
    grads2 = torch.autograd.grad(loss2, params)
    with torch.no_grad():
        for p, e in zip(params, eps):
            p.sub_(e)
    return params, grads, eps, grads2, (loss.item(), loss2.item()), norm.item()


@pytest.mark.parametrize("adaptive,rho", [(False, 0.0625), (True, 0.5)], ids=["plain", "adaptive"])
def test_oracle_equals_the_published_two_step_procedure(adaptive, rho):
    torch.manual_seed(3)
    lin = torch.nn.Linear(6, 5).double()
    x, y = torch.randn(16, 6, dtype=torch.float64), torch.randn(16, 5, dtype=torch.float64)
    params, grads, eps, grads2, (l1, l2), norm = _published_step(lin, x, y, rho, adaptive)
    # the arena's layout: each tensor at a multiple of 8 elements, one chunk per tensor, zeros in the alignment padding
    total, offs = 0, []
    for p in params:
        offs.append(total)
        total += (p.numel() + 7) // 8 * 8
    flat, gflat = np.zeros(total), np.zeros(total)
    chunks = []
    for off, p, g in zip(offs, params, grads):
        flat[off:off + p.numel()] = p.detach().numpy().reshape(-1)
        gflat[off:off + p.numel()] = g.numpy().reshape(-1)
        chunks.append((off, (p.numel() + 7) // 8 * 8))
    got = SO.ascend(flat, gflat, chunks, rho, adaptive)       # (these rho are f32 numbers: the oracle's rounding of rho is exact)
    assert not got["skip"]
    assert abs(got["norm"] - norm) <= 1e-14 * norm
    for off, p, e in zip(offs, params, eps):
        want_e = e.detach().numpy().reshape(-1)
        assert np.abs(got["e"][off:off + p.numel()] - want_e).max() <= 1e-14 * np.abs(want_e).max()
        want_p = (p.detach() + e.detach()).numpy().reshape(-1)
        assert np.abs(got["p_new"][off:off + p.numel()] - want_p).max() <= 1e-15 * max(1.0, np.abs(want_p).max())
        assert (got["e"][off + p.numel():off + (p.numel() + 7) // 8 * 8] == 0).all(), "the padding does not move"
    # the perturbation lies on the sphere the papers put it on: ||e|| = rho, ASAM ||e / |w||| = rho
    e, m = got["e"], flat != 0
    radius = np.sqrt(np.sum((e[m] / np.abs(flat[m])) ** 2)) if adaptive else np.sqrt(np.sum(e ** 2))
    assert abs(radius - rho) <= 1e-10 * rho
    # and it climbs: g . e > 0, and the (convex) loss rises by at least that
    assert float(np.dot(gflat, e)) > 0 and l2 - l1 >= float(np.dot(gflat, e)) * (1 - 1e-9)
    assert any(not torch.equal(a, b) for a, b in zip(grads, grads2)), "the second gradient is another gradient"
    # the same perturbation through the oracle's building blocks
    part = SO.partials(flat, gflat, chunks, adaptive)
    assert abs(np.sqrt(part.sum()) - got["norm"]) <= 1e-15 * got["norm"]
    assert got["scale"] == SO.step_scale(rho, got["norm"])
    assert np.array_equal(SO.perturbation(flat, gflat, got["scale"], adaptive)[:30], e[:30])


def test_oracle_skip_rule_bars_and_table():
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal(64).astype(np.float32), (0.02 * rng.standard_normal(64)).astype(np.float32)
    chunks = [(8, 16), (40, 8)]
    for adaptive in (False, True):
        got = SO.ascend(p, g, chunks, 0.05, adaptive)
        inside = SO._mask(64, chunks)
        assert not got["skip"] and (got["e"][~inside] == 0).all() and np.array_equal(got["p_new"][~inside], p[~inside].astype(np.float64))
        assert (got["bar"][~inside] == 0).all() and (got["bar"][inside] > 0).all()
        assert np.isnan(got["backup"][~inside]).all() and np.array_equal(got["backup"][inside], p[inside].astype(np.float64))
        assert got["scale"] == float(np.float32(0.05)) / (got["norm"] + 1e-12), "rho is an f32 launch argument"
        # an element outside the table changes nothing, not even through the norm
        g2 = g.copy()
        g2[0] = 1e30
        assert SO.ascend(p, g2, chunks, 0.05, adaptive)["norm"] == got["norm"]
        for bad in (np.inf, np.nan):
            g3 = g.copy()
            g3[9] = bad
            r = SO.ascend(p, g3, chunks, 0.05, adaptive)
            assert r["skip"] and r["scale"] == 0.0 and np.array_equal(r["p_new"], p.astype(np.float64))
        r = SO.ascend(p, np.zeros_like(g), chunks, 0.05, adaptive)
        assert r["skip"] and r["norm"] == 0.0
    # the depth of the documented tree, and the bars that follow from it
    assert SO.tree_depth(False) == 20 and SO.tree_depth(True) == 21
    assert SO.tree_depth(False, 8) == 13 and SO.tree_depth(False, 8184) == 20 and SO.tree_depth(False, 1025) == 14
    assert SO.norm_bar(False, [(0, 8), (8, 8192)]) == 20 * 2.0 ** -24
    got = SO.ascend(p, g, [(0, 64)], 0.05, True)
    d = SO.tree_depth(True, 64)
    want = 2.0 ** -24 * (3 * np.abs(got["e"]) + np.abs(got["p_new"])) + np.abs(got["e"]) * d * 2.0 ** -24
    assert np.array_equal(got["bar"], want)


def _tiny():
    return torch.nn.Linear(8, 8)


def test_argument_refusals_without_a_device():
    import icka_amd
    from icka_amd import sam as S
    from icka_amd.optim import ArenaAdamW
    m = _tiny()
    opt = ArenaAdamW(m)
    assert not S.registered(m)
    for bad in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError, match="rho"):
            icka_amd.SAM(m, opt, rho=bad)
    with pytest.raises(TypeError, match="ArenaAdamW"):
        icka_amd.SAM(m, torch.optim.AdamW(m.parameters()))
    with pytest.raises(ValueError, match="another model"):
        icka_amd.SAM(_tiny(), opt)
    assert not S.registered(m), "a refused construction registers nothing"
    # a GradReducer on the arena: data parallel is out of scope
    dp = _tiny()
    object.__setattr__(dp, "_icka_arena", types.SimpleNamespace(reducer=object()))
    with pytest.raises(NotImplementedError, match="GradReducer"):
        icka_amd.SAM(dp, ArenaAdamW(dp))
    sam = icka_amd.SAM(m, opt, rho=0.1, adaptive=True)
    assert (sam.rho, sam.adaptive) == (0.1, True) and S.registered(m) and not S.registered(_tiny())
    assert (sam.ascents(), sam.skipped_ascents()) == (0, 0), "before the first ascent there is no device block to read"
    calls = []

    def closure():
        calls.append(1)
        return m(torch.zeros(2, 8)).sum()

    # run while the averaged weights are swapped in; a nested run; the perturbation flag in front of step()
    opt._swapped = True
    with pytest.raises(RuntimeError, match="averaged weights"):
        sam.run(closure)
    opt._swapped = False
    opt._perturbed = True
    with pytest.raises(RuntimeError, match="perturbation"):
        opt.step()
    with pytest.raises(RuntimeError, match="already in place"):
        sam.run(closure)
    opt._perturbed = False
    assert calls == [], "every refusal came before the first pass"
    with pytest.raises(RuntimeError, match="does not nest"):
        sam.run(lambda: sam.run(closure))
    assert calls == [] and not sam._running
    # the model is on the CPU: the first pass runs, the ascent refuses as ArenaAdamW.step() does
    with pytest.raises(RuntimeError, match="no CPU path"):
        sam.run(closure)
    assert calls == [1] and not sam._running and not opt._perturbed


def test_train_step_refuses_accumulation_for_a_model_with_a_registered_sam():
    import icka_amd
    from icka_amd.optim import ArenaAdamW
    m = _tiny()
    opt = ArenaAdamW(m, capturable=True)
    sam = icka_amd.SAM(m, opt)
    with pytest.raises(NotImplementedError, match="accumulate=1"):
        icka_amd.TrainStep(m, lambda x: sam.run(lambda: m(x).sum()), opt, inputs=(torch.zeros(2, 8),), accumulate=2)
    del sam


def test_sam_state_layout_matches_c_struct():
    """sizeof / offsetof of icka_sam_state as the C compiler lays it out == the ctypes mirror."""
    import ctypes
    import subprocess
    import tempfile
    from icka_amd import _lib
    S = _lib.SamState
    fields = [f[0] for f in S._fields_]
    assert fields == ["norm", "scale", "skip", "reserved", "ascents", "skipped"]
    src = '#include <stdio.h>\n#include "icka_hip.h"\nint main(){printf("%zu", sizeof(icka_sam_state));\n' + \
          "".join('printf(" %%zu", __builtin_offsetof(icka_sam_state, %s));\n' % f for f in fields) + \
          'printf(" %d", ICKA_SAM_DRY);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(S) == 32
    assert out[1:1 + len(fields)] == [getattr(S, f).offset for f in fields]
    assert out[-1] == _lib.SAM_DRY
    assert S.ascents.offset % 8 == 0 and S.skipped.offset % 8 == 0
