"""Float64 NumPy restatement of the averaged weights of ArenaAdamW(average="ema" | "swa") (icka_amd/optim.py;
csrc/optim.hip: optim_average_prepare_kernel, optim_average_kernel, optim_swap_kernel): the decay rule, the update, the
start / every selection and the swap.  Nothing here imports icka_amd."""
import numpy as np


def decay_at(kind, decay, warmup, n):
    """The decay of averaged update number n + 1."""
    assert kind in ("ema", "swa") and n >= 0
    if n == 0:
        return 0.0
    if kind == "swa":
        return n / (n + 1.0)
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def applies(start, every, t):
    """Whether update number t (1-based) is averaged."""
    return t > start and (t - start - 1) % every == 0


def update(avg, p, d):
    """avg + (1 - d) * (p - avg) in float64."""
    avg, p = np.asarray(avg, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return avg + (1.0 - d) * (p - avg)


def run(kind, decay, warmup, start, every, snapshots, avg0=None, n0=0, applied=None):
    """The average after the updates whose parameters are ``snapshots`` (snapshot k = the parameters after update k + 1).
    ``applied``: optional per-update flags, False = that update was refused (not applied, not counted, t does not advance).
    Returns (average in float64, n, the per-element rounding bound of an f32 implementation, the update numbers averaged).

    The bound: an f32 implementation rounds 1 - d, p - avg, the product and the sum: four roundings of at most 2^-24
    relative each, every one on a value of magnitude at most |p| + |avg|, so update k adds at most
    4 * 2^-24 * (|p_k| + |avg_{k-1}|) and (the factor d <= 1 on the carried error) the errors add up."""
    avg = None if avg0 is None else np.asarray(avg0, dtype=np.float64).copy()
    n, t, bound, used = int(n0), 0, None, []
    for k, p in enumerate(snapshots):
        if applied is not None and not applied[k]:
            continue
        t += 1
        p = np.asarray(p, dtype=np.float64)
        if bound is None:
            bound = np.zeros_like(p)
        if not applies(start, every, t):
            continue
        d = decay_at(kind, decay, warmup, n)
        prev = np.zeros_like(p) if avg is None else avg
        bound = bound + 4.0 * 2.0 ** -24 * (np.abs(p) + np.abs(prev))
        avg = p.copy() if (avg is None or d == 0.0) else update(avg, p, d)
        n += 1
        used.append(t)
    return avg, n, bound, used


def swap(p, avg):
    """What icka_optim_swap leaves: (new p, new avg, bf16 bits are the caller's to derive from new p)."""
    return np.array(avg, copy=True), np.array(p, copy=True)
