"""Float64 NumPy restatement of the sharpness-aware ascent (icka_amd/sam.py; csrc/sam.hip: sam_sqnorm_adaptive_kernel,
sam_prepare_kernel, sam_ascend_kernel, sam_restore_kernel): norm, step scale, both forms of the perturbation e, the perturbed
weights, and the bars an f32 implementation is held to.  Nothing here imports icka_amd.

    plain:     n = sqrt(sum g^2)           s = rho / (n + 1e-12)    e = s g          p' = p + e
    adaptive:  n = sqrt(sum (|p| g)^2)     s = rho / (n + 1e-12)    e = p^2 g s      p' = p + e

over the elements the chunk table names ((first element, count) pairs), everything else untouched.  ``rho`` reaches the kernel as
an f32 launch argument, so the oracle rounds it to f32 first; all else is float64 on the f32 inputs.

The norm's bar (relative): 2^-24 times the DEPTH of the summation tree of one chunk -- the number of f32 roundings on the longest
path from an element to the chunk's partial sum.  Every term is non-negative, so a sum whose every path carries at most d
roundings is off by at most (1 + 2^-24)^d - 1 ~ d 2^-24 relative, whatever the order.  The path, for a chunk of at most 8192
elements walked by 256 threads four elements at a time (optim_sqnorm_kernel's loop, which the adaptive kernel repeats):
    adaptive only: a = |p| g                                  1
    the square                                                1
    the sum of the four squares of one 16-byte load           3
    the thread's running sum, ceil(count / 1024) iterations   8 for a full chunk
    the wave's sum (four DPP steps, two steps over the rows)  6
    the block's four waves, (r0 + r1) + (r2 + r3)             2
= 20 (plain) / 21 (adaptive) for a full chunk; a fused multiply-add only removes roundings.  The partials are then summed in
double (2^-53 per step: nothing beside 2^-24), the square root halves the relative error and the cast to f32 adds one 2^-24, so
the norm itself is within (d / 2 + 1) 2^-24 and the step scale -- one more f32 cast -- within (d / 2 + 2) 2^-24, both inside
d 2^-24 for every d >= 4.

The per-element bar of p': one 2^-24 |value| term per f32 rounding the header documents, plus |e| times the norm's bar (the
relative error of the scale, which multiplies e):
    plain,    two roundings:   e = scale * g -> 2^-24 |e|;   p' = p + e -> 2^-24 |p'|
    adaptive, four roundings:  t = p * p, u = t * g, e = u * scale -> each an error of 2^-24 relative on a factor of e, so
                               2^-24 |e| each;   p' = p + e -> 2^-24 |p'|
    bar = 2^-24 (k |e| + |p'|) + |e| d 2^-24,   k = 1 (plain) or 3 (adaptive)
The backup, the restored weights, the 16-bit shadows and everything outside the table have no bar: they are bitwise."""
import numpy as np

U = 2.0 ** -24
CHUNK = 8192


def tree_depth(adaptive, count=CHUNK):
    """f32 roundings on the longest path from an element of a chunk of ``count`` elements to its partial sum."""
    assert 0 < count <= CHUNK
    return (1 if adaptive else 0) + 1 + 3 + -(-count // 1024) + 6 + 2


def norm_bar(adaptive, chunks):
    """Relative bar of the norm (and of the step scale) over a table of (first element, count) chunks."""
    return U * max(tree_depth(adaptive, n) for _, n in chunks)


def _mask(total, chunks):
    m = np.zeros(total, dtype=bool)
    for lo, n in chunks:
        m[lo:lo + n] = True
    return m


def partials(p, g, chunks, adaptive):
    """Per-chunk sums of (t g)^2 in float64."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    out = []
    for lo, n in chunks:
        a = g[lo:lo + n] * (np.abs(p[lo:lo + n]) if adaptive else 1.0)
        out.append(float(np.sum(a * a)))
    return np.array(out)


def step_scale(rho, norm):
    return float(np.float32(rho)) / (float(norm) + 1e-12)


def perturbation(p, g, scale, adaptive):
    """e for every element, in float64."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return (p * p * g * scale) if adaptive else (scale * g)


def ascend(p, g, chunks, rho, adaptive):
    """What icka_sam_sqnorm + icka_sam_prepare + icka_sam_ascend leave, in float64: a dict of ``skip`` (the ascent is refused:
    the sum is zero or not finite), ``norm``, ``scale``, ``e`` and ``p_new`` (full length; e = 0 and p_new = p outside the table
    and for a refused ascent), ``backup`` (p inside the table, NaN outside: not written), ``norm_bar`` (relative) and ``bar``
    (per element of p_new)."""
    p64, g64 = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m = _mask(p64.shape[0], chunks)
    with np.errstate(all="ignore"):
        total = float(np.sum(partials(p64, g64, chunks, adaptive)))
    nb = norm_bar(adaptive, chunks)
    out = {"norm_bar": nb, "backup": np.where(m, p64, np.nan)}
    if not np.isfinite(total) or total == 0.0:
        out.update(skip=True, norm=float(np.sqrt(total)) if total >= 0 else float("nan"), scale=0.0, e=np.zeros_like(p64),
                   p_new=p64.copy(), bar=np.zeros_like(p64))
        return out
    norm = float(np.sqrt(total))
    scale = step_scale(rho, norm)
    e = np.where(m, perturbation(p64, g64, scale, adaptive), 0.0)
    p_new = p64 + e
    k = 3.0 if adaptive else 1.0
    bar = np.where(m, U * (k * np.abs(e) + np.abs(p_new)) + np.abs(e) * nb, 0.0)
    out.update(skip=False, norm=norm, scale=scale, e=e, p_new=p_new, bar=bar)
    return out
