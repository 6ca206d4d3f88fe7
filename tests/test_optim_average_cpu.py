"""CPU: the host side of ArenaAdamW(average="ema" | "swa") -- the decay rule against the float64 oracle of
tests/optim_average_oracle.py, the oracle's SWA against the arithmetic mean, constructor validation and refusals, and the ctypes
mirror of icka_average_state against the header's struct as gcc lays it out."""
import os

import numpy as np
import pytest
import torch

import optim_average_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = [("swa", 0.999, True), ("ema", 0.999, True), ("ema", 0.9, False)]


@pytest.mark.parametrize("kind,decay,warmup", MODES, ids=["swa", "ema-warmup", "ema-plain"])
def test_average_decay_at_equals_the_oracle(kind, decay, warmup):
    from icka_amd.optim import average_decay_at
    for n in range(51):
        assert average_decay_at(kind, decay, warmup, n) == AO.decay_at(kind, decay, warmup, n), n
    assert average_decay_at(kind, decay, warmup, 0) == 0.0
    if kind == "ema" and warmup:
        assert average_decay_at(kind, decay, warmup, 1) == 2.0 / 11.0
        assert average_decay_at(kind, decay, warmup, 10 ** 6) == decay
    if kind == "swa":
        assert average_decay_at(kind, decay, warmup, 3) == 0.75


def test_average_applies_equals_the_oracle():
    from icka_amd.optim import average_applies
    for start in (0, 1, 2, 5):
        for every in (1, 2, 3):
            got = [t for t in range(1, 20) if average_applies(start, every, t)]
            assert got == [t for t in range(1, 20) if AO.applies(start, every, t)]
            assert got[0] == start + 1 and all(b - a == every for a, b in zip(got, got[1:]))


def test_oracle_swa_is_the_arithmetic_mean():
    rng = np.random.default_rng(0)
    snaps = [rng.standard_normal(257) * s for s in (1e-3, 1.0, 30.0, 1.0, 0.5, 2.0, 7.0)]
    for k in range(1, len(snaps) + 1):
        avg, n, _, used = AO.run("swa", 0.0, False, 0, 1, snaps[:k])
        assert n == k and used == list(range(1, k + 1))
        assert np.abs(avg - np.mean(snaps[:k], axis=0)).max() <= 1e-12
    # start / every: the mean of the snapshots the rule names
    avg, n, _, used = AO.run("swa", 0.0, False, 2, 2, snaps)
    assert used == [3, 5, 7] and n == 3
    assert np.abs(avg - np.mean([snaps[2], snaps[4], snaps[6]], axis=0)).max() <= 1e-12
    # a refused update is neither counted nor averaged
    avg, n, _, used = AO.run("swa", 0.0, False, 0, 1, snaps[:4], applied=[True, False, True, True])
    assert n == 3 and np.abs(avg - np.mean([snaps[0], snaps[2], snaps[3]], axis=0)).max() <= 1e-12


def test_oracle_swap_exchanges():
    p, a = np.arange(8.0), -np.arange(8.0)
    np_, na = AO.swap(p, a)
    assert np.array_equal(np_, a) and np.array_equal(na, p)
    p2, a2 = AO.swap(np_, na)
    assert np.array_equal(p2, p) and np.array_equal(a2, a)


def _tiny():
    return torch.nn.Linear(8, 8)


def test_constructor_validation():
    from icka_amd.optim import ArenaAdamW, average_decay_at
    m = _tiny()
    with pytest.raises(ValueError, match="average="):
        ArenaAdamW(m, average="mean")
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="average_decay"):
            ArenaAdamW(m, average="ema", average_decay=bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError, match="average_start"):
            ArenaAdamW(m, average="swa", average_start=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="average_every"):
            ArenaAdamW(m, average="swa", average_every=bad)
    with pytest.raises(ValueError, match="kind"):
        average_decay_at("mean", 0.9, True, 1)
    with pytest.raises(ValueError):
        average_decay_at("ema", 0.9, True, -1)
    opt = ArenaAdamW(m, average="ema", average_decay=0.0, average_start=3, average_every=2, capturable=True)
    assert (opt.average, opt.average_decay, opt.average_start, opt.average_every) == ("ema", 0.0, 3, 2)
    assert opt.average_count() == 0


def test_off_by_default_allocates_nothing_and_refuses_the_methods():
    from icka_amd.optim import ArenaAdamW
    opt = ArenaAdamW(_tiny())
    assert opt.average is None and opt._avg is None and opt._avg_table is None and opt._avg_state is None
    assert "icka_avg" not in opt.state_dict() and "icka_avg_n" not in opt.state_dict()
    with pytest.raises(RuntimeError, match="average="):
        opt.average_count()
    with pytest.raises(RuntimeError, match="average="):
        opt.averaged_state_dict()
    with pytest.raises(RuntimeError, match="average="):
        with opt.averaged_weights():
            pass


def test_refusals_while_swapped_and_without_a_device():
    """step() and state_dict() / load_state_dict() look at the swapped flag before anything else; the methods that need the
    buffers refuse a model on the CPU as step() does."""
    from icka_amd.optim import ArenaAdamW
    opt = ArenaAdamW(_tiny(), average="swa")
    with pytest.raises(RuntimeError, match="no CPU path"):
        with opt.averaged_weights():
            pass
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.averaged_state_dict()
    sd = opt.state_dict()
    opt._swapped = True
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.load_state_dict(sd)
    opt._swapped = False
    # a checkpoint's average comes with its count and its layout
    with pytest.raises(ValueError, match="come together"):
        opt.load_state_dict(dict(sd, icka_avg=torch.zeros(8)))


def test_a_loaded_average_waits_for_the_arena():
    from icka_amd.optim import ArenaAdamW
    opt = ArenaAdamW(_tiny(), average="swa")
    sd = opt.state_dict()
    sd.update(icka_m=torch.zeros(72), icka_v=torch.zeros(72), icka_layout=[("weight", 0, 64), ("bias", 64, 8)],
              icka_avg=torch.ones(72), icka_avg_n=5, icka_t=9)
    opt.load_state_dict(sd)
    assert opt.average_count() == 5 and opt.steps_taken() == 9
    again = opt.state_dict()
    assert again["icka_avg_n"] == 5 and torch.equal(again["icka_avg"], torch.ones(72))
    # a state without an average restarts it
    opt.load_state_dict({k: v for k, v in sd.items() if k not in ("icka_avg", "icka_avg_n")})
    assert opt.average_count() == 0 and "icka_avg" not in opt.state_dict()


def test_average_state_layout_matches_c_struct():
    """sizeof / offsetof of icka_average_state as the C compiler lays it out == the ctypes mirror."""
    import ctypes
    import subprocess
    import tempfile
    from icka_amd import _lib
    S = _lib.AverageState
    fields = [f[0] for f in S._fields_]
    assert fields == ["n", "decay_now", "apply", "kind", "warmup", "decay", "start", "every"]
    src = '#include <stdio.h>\n#include "icka_hip.h"\nint main(){printf("%zu", sizeof(icka_average_state));\n' + \
          "".join('printf(" %%zu", __builtin_offsetof(icka_average_state, %s));\n' % f for f in fields) + \
          'printf(" %d %d", ICKA_AVERAGE_EMA, ICKA_AVERAGE_SWA);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(S)
    assert out[1:1 + len(fields)] == [getattr(S, f).offset for f in fields]
    assert out[-2:] == [_lib.AVERAGE_EMA, _lib.AVERAGE_SWA]
    assert S.HOST_LO == S.kind.offset and S.n.offset == 0 and ctypes.sizeof(S) % 8 == 0
