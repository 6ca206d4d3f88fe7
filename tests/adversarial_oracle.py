"""Float64 restatement of the adversarial-training definitions of include/icka_hip.h ("adversarial training"): the ascent step
of icka_adv_ascend and the uniform start of icka_adv_init_uniform; no test functions.  Shared by tests/adversarial_check.py,
tests/test_adversarial_cpu.py and the GPU tests."""
import numpy as np
import torch

F64 = torch.float64
SLAB_ROWS = 8                 # token rows per block of icka_adv_ascend (the header's reduction tree)


def icka_hash(s0, s1, idx):
    """csrc/common.h: icka_hash, on numpy uint32 arrays"""
    with np.errstate(over="ignore"):
        x = (np.asarray(idx).astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(s0)).astype(np.uint32)
        x = x ^ (x >> np.uint32(16))
        x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
        x = x ^ (x >> np.uint32(15))
        x = (x * np.uint32(0x846ca68b) + np.uint32(s1)).astype(np.uint32)
        x = x ^ (x >> np.uint32(16))
    return x


def uniform_r(n, seed, counter=0):
    """r of the flat element indices 0 .. n-1: (float)(hash >> 8) * 2^-23 - 1, exact in f32 and so in float64"""
    sd = (int(seed) + int(counter)) & 0xFFFFFFFFFFFFFFFF
    h = icka_hash(sd & 0xFFFFFFFF, sd >> 32, np.arange(n, dtype=np.uint64).astype(np.uint32))
    return (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def valid_of(mask):
    return mask != 0


def uniform_start64(mask, H, epsilon, seed, counter=0):
    """delta0 [B, S, H] float64: r * epsilon / sqrt(n_b * H) at valid positions, 0 elsewhere"""
    B, S = mask.shape
    v = valid_of(mask)
    n_b = v.sum(1).to(F64)
    r = torch.from_numpy(uniform_r(B * S * H, seed, counter)).reshape(B, S, H)
    sc = torch.where(n_b > 0, epsilon / torch.sqrt((n_b * H).clamp_min(1.0)), torch.zeros_like(n_b))
    return torch.where(v[:, :, None], r * sc[:, None, None], torch.zeros_like(r))


def uniform_start_f32(mask, H, epsilon, seed, counter=0):
    """The same in the kernel's f32 arithmetic -- one correctly rounded square root of the exact product n_b * H, one
    correctly rounded division, one product per element -- for a bitwise comparison."""
    B, S = mask.shape
    v = valid_of(mask).numpy()
    n_b = v.sum(1).astype(np.float32)
    r = uniform_r(B * S * H, seed, counter).astype(np.float32).reshape(B, S, H)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.float32(epsilon) / np.sqrt(n_b * np.float32(H), dtype=np.float32)
    out = np.where(v[:, :, None], r * sc.astype(np.float32)[:, None, None], np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(out)


def sumsq(x, valid):
    """per-sample sum of squares over the valid positions, float64 [B] (a non-finite element of a valid row -> inf / NaN)"""
    x = x.to(F64)
    sq = torch.where(valid[:, :, None], x * x, torch.zeros_like(x))
    return sq.sum((1, 2))


def ascend64(delta, grad, mask, alpha, epsilon):
    """One ascent step.  -> dict: delta [B, S, H] float64, norms [B, 2] float64 (n_g, ||delta_b|| after the step), stepped [B]
    (n_g neither 0 nor non-finite), n_u [B] (the norm before the projection), shrunk [B]."""
    v = valid_of(mask)
    d, g = delta.to(F64), grad.to(F64)
    n_g = torch.sqrt(sumsq(g, v))
    stepped = torch.isfinite(n_g) & (n_g > 0)
    sc = torch.where(stepped, alpha / torch.where(stepped, n_g, torch.ones_like(n_g)), torch.zeros_like(n_g))
    gz = torch.where(stepped[:, None, None], g, torch.zeros_like(g))          # (a sample that stays never reads g into delta)
    u = torch.where(v[:, :, None], d + sc[:, None, None] * gz, torch.zeros_like(d))
    n_u = torch.sqrt(sumsq(u, v))
    shrunk = stepped & (n_u > epsilon)
    f = torch.where(shrunk, epsilon / torch.where(shrunk, n_u, torch.ones_like(n_u)), torch.ones_like(n_u))
    out = u * f[:, None, None]
    n_after = torch.where(shrunk, torch.full_like(n_u, epsilon), n_u)
    return dict(delta=out, norms=torch.stack([n_g, n_after], 1), stepped=stepped, n_u=n_u, shrunk=shrunk, u=u)
