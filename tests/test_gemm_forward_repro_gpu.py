"""GPU: a forward GEMM with a handful of rows gives the same bits on every call.

The general GEMM path may split K over blockIdx.y and add the partial tiles with f32 atomics, whose order is not fixed.  That
is meant for skinny WEIGHT GRADIENTS (TN).  A forward (NT / NN) GEMM of a few rows with f32 output -- [batch, 1024] x
[1024, 1024] at an evaluation batch of 2 or 3 -- used to meet the same condition: its output then moved by one ulp from call
to call, and the dev loss of a replayed capture differed from the eager one (test_crf_decode_graph_gpu)."""
import pytest
import torch

from icka_amd import kernels as K

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("op", ["nt", "nn"])
@pytest.mark.parametrize("rows,n,k", [(3, 1024, 1024), (2, 1024, 1024), (32, 768, 2048), (256, 128, 4096)])
def test_forward_gemm_of_few_rows_is_bitwise_reproducible(op, rows, n, k):
    g = torch.Generator(device="cuda").manual_seed(rows * 7 + n + k)
    x = torch.randn(rows, k, generator=g, device="cuda", dtype=F32).to(BF16)
    w = torch.randn(n, k, generator=g, device="cuda", dtype=F32).to(BF16)
    if op == "nn":
        w = w.t().contiguous()                                    # [k, n]
    code = K.GEMM_NT if op == "nt" else K.GEMM_NN
    first = K.gemm(code, x, w, torch.empty(rows, n, device="cuda", dtype=F32)).clone()
    ref = x.float() @ (w.float().t() if op == "nt" else w.float())
    # f32 accumulation of k bf16 products, outputs of size ~sqrt(k)
    assert (first - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-3
    for _ in range(12):
        again = K.gemm(code, x, w, torch.empty(rows, n, device="cuda", dtype=F32))
        assert torch.equal(first, again)
