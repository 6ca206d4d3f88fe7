"""CPU: the learning-rate factor the capturable ArenaAdamW evaluates on the device (csrc/optim.hip: optim_prepare_kernel), as
restated in Python by ``optim.schedule_factor``, against the reference's scheduler: transformers.get_linear_schedule_with_warmup
(My_cross_attention.py:756-757), which is a LambdaLR -- update number t + 1 runs at base_lr * lambda(t)."""
import pytest
import torch

CASES = [(0, 5), (4, 4), (2, 7)]       # (num_warmup_steps, num_training_steps): no warm-up, warm-up == total, the usual kind
BASE = 3e-5


def _lambda_lr_rates(make, n):
    """Rates of updates 1 .. n under a LambdaLR built by ``make(optimizer)``: the rate in force when optimizer.step() runs."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("warmup,total", CASES)
def test_factor_equals_get_linear_schedule_with_warmup(warmup, total):
    from transformers import get_linear_schedule_with_warmup
    from icka_amd.optim import schedule_factor
    n = total + 4                      # t = 0 .. total + 3
    ref = _lambda_lr_rates(lambda o: get_linear_schedule_with_warmup(o, warmup, total), n)
    mine = [BASE * schedule_factor("linear", warmup, total, t) for t in range(n)]
    assert mine == ref, (mine, ref)
    assert all(schedule_factor("constant", warmup, total, t) == 1.0 for t in range(n))


@pytest.mark.parametrize("warmup,total", CASES)
def test_factor_equals_the_hand_written_lambda_of_the_recipe_test(warmup, total):
    """tests/test_recipe_gpu.py writes the same schedule by hand (its ``total + 1`` is this ``total``)."""
    from icka_amd.optim import schedule_factor
    n = total + 4
    hand = lambda s: float(s) / max(1, warmup) if s < warmup else max(0.0, float(total - s) / max(1, total - warmup))  # noqa: E731
    ref = _lambda_lr_rates(lambda o: torch.optim.lr_scheduler.LambdaLR(o, hand), n)
    assert [BASE * schedule_factor("linear", warmup, total, t) for t in range(n)] == ref


def test_the_rates_of_warmup_2_total_7():
    from icka_amd.optim import schedule_factor
    got = [BASE * schedule_factor("linear", 2, 7, t) for t in range(10)]
    want = [0, 1.5e-5, 3e-5, 2.4e-5, 1.8e-5, 1.2e-5, 6e-6, 0, 0, 0]
    assert got == pytest.approx(want, rel=1e-12, abs=0)


def test_schedule_argument_is_validated():
    from icka_amd.optim import _parse_schedule, schedule_factor
    assert _parse_schedule(None) == _parse_schedule("constant") == ("constant", 0, 0)
    assert _parse_schedule(("linear", 2, 7)) == ("linear", 2, 7)
    for bad in ("cosine", ("linear", 2), ("linear", -1, 3), 5):
        with pytest.raises(ValueError):
            _parse_schedule(bad)
    with pytest.raises(ValueError):
        schedule_factor("cosine", 0, 1, 0)
