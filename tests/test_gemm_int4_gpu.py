"""int4 (group-128) weight-only quantisation: the quantiser's guarantees (CPU), mi_gemm_int4w_packed against an fp64
product of the dequantised matrix, the entry points' contract, and the engine with quantization="int4"."""
import pytest
import torch

from model_configs import MID, TINY, make_model_dir
from test_kernels_gpu import assert_bf16_close

DEV = "cuda:0"


def test_quantiser_scale_has_four_bits_and_dequantisation_is_exact_in_bf16():
    from nanovllm import ops

    g = torch.Generator().manual_seed(1)
    w = torch.randn(32, 1024, generator=g) * 0.02
    w = (w.view(32, 8, 128) * 2.0 ** torch.randint(-6, 7, (32, 8, 1), generator=g)).view(32, 1024)
    w[3, 256:384] = 0  # an all-zero group
    w = w.bfloat16()
    q, s = ops.quantize_int4(w)
    assert q.dtype == torch.uint8 and s.dtype == torch.bfloat16 and 1 <= int(q.min()) and int(q.max()) <= 15
    assert not bool((s.view(torch.int16) & 0xF).any())  # four-bit significand
    absmax, s64 = w.double().view(32, 8, 128).abs().amax(-1), s.double()
    nz = absmax > 0
    assert bool((s64[~nz] == 1).all()) and bool((s64 >= absmax / 7)[nz].all()) and bool((absmax / 7 > s64 / 1.125)[nz].all())
    deq = ops.dequantize_int4(q, s)
    assert bool(((w.double() - deq.double()).abs().view(32, 8, 128) <= s64[..., None] / 2).all())
    exact = (q.double() - 8).view(32, 8, 128) * s64[..., None]
    assert torch.equal(deq.double(), exact.view(32, 1024))  # (q - 8) * s needs no rounding in bf16


def test_entry_points_check_shapes_on_the_host_and_config_takes_int4():
    from nanovllm import _C
    from nanovllm.config import Config

    p = 0x1000  # checked, never dereferenced: both calls return before any launch
    assert _C.lib.mi_gemm_int4w_packed(p, p, p, p, 1, 16, 192, 0, None) == -2  # K is no multiple of the group
    assert _C.lib.mi_gemm_int4w_packed(p, p, None, p, 1, 16, 128, 0, None) == -1  # null scale
    model = make_model_dir(TINY)
    assert Config(model, quantization="int4").quantization == "int4"
    with pytest.raises(AssertionError):
        Config(model, quantization="int3")


SHAPES = (
    [(256, k, m) for k in (128,     # one group, one wave
                           256,     # two waves
                           896,     # seven groups: an odd wave count
                           1024,    # eight waves of one group: the widest single-group form at 33+ rows
                           3072)    # 12 / 8 / 4 waves x 2 / 3 / 6 groups: the double-buffered loop, each peeled tail
     for m in (1, 17, 64, 100)]     # one to four column tiles; 100: a second chunk of 64 rows, partly filled
    + [(16, k, m) for k in (128, 3072) for m in (1, 100)]      # a single row tile
    + [(32768, 1024, m) for m in (17, 64)])  # two row tiles per workgroup (<= 32 rows); >= 2048 workgroups: four waves


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,M", SHAPES)
def test_gemm_int4_weights(N, K, M):
    """All sixteen nibbles, four-bit scales varying by row and group (dequantised std ~0.02), x = randn: the kernel
    against bf16(fp64 product of the dequantised matrix) - no allowance for the format, the dequantised weights are
    exact.  Bound of test_gemm_fp8_weights (same fp32 sum over K, one rounding).  A torch fp32 emulation of the
    kernel's order (each wave's K-slice in 32-deep steps, then the waves in order) on the CPU differs from the fp64
    reference by one ulp on 0 .. 3.9e-5 of the outputs of these shapes (max_frac 0.02 is a cap)."""
    from nanovllm import ops

    g = torch.Generator().manual_seed(N + K + M)
    x = torch.randn(M, K, generator=g).bfloat16()
    q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    scale = ((8 + torch.randint(0, 8, (N, K // 128), generator=g)) / 8 * 2.0 ** (torch.randint(0, 2, (N, K // 128), generator=g) - 9)).bfloat16()
    want = (x.double() @ ops.dequantize_int4(q, scale).double().T).bfloat16()
    wp = ops.pack_weight_int4((q.to(DEV), scale.to(DEV)))
    xd = x.to(DEV)
    assert_bf16_close(ops.gemm_packed(xd, wp).cpu(), want, max_ulp=1, max_frac=0.02, atol=K * 2.0 ** -22)
    for ks in (2, 4):
        if K % (128 * ks) == 0:
            parts = ops.gemm_packed_splitk(xd, wp, ks).cpu()
            assert_bf16_close(parts.sum(0).bfloat16(), want, max_ulp=1, max_frac=0.02, atol=K * 2.0 ** -22)
    if N == 256:
        act = ops.gemm_packed(xd, wp, silu_mul=True).cpu()
        gate, up = want[:, : N // 2].float(), want[:, N // 2:].float()
        ref = (torch.nn.functional.silu(gate).bfloat16().float() * up).bfloat16()
        assert_bf16_close(act, ref, max_ulp=2, max_frac=0.05, atol=32 * K * 2.0 ** -22)


@pytest.mark.gpu
def test_engine_int4_weights_match_oracle_on_dequantised_weights(monkeypatch):
    """MID widths, hipGraph decode: the decode GEMMs stream the nibbles, the prefill runs the bf16 tile GEMM on the
    dequantised parameters, the oracle gets the same dequantised projections (head and embedding stay bf16).  The
    error sources are the bf16 engine's (activation roundings); measured worst |logit - oracle| 2.55e-2 - twice that
    is not below the fp8 case's 6e-2, which therefore stays the bound."""
    import test_engine_gpu as eng
    from nanovllm import ops

    make_oracle = eng._oracle_for

    def oracle_on_dequantised(llm, cfg, seed):
        oracle = make_oracle(llm, cfg, seed)
        for name, w in oracle.w.items():
            if w.dim() == 2 and "proj" in name:
                oracle.w[name] = ops.dequantize_int4(*ops.quantize_int4(w)).to(w.dtype)
        return oracle

    monkeypatch.setattr(eng, "_oracle_for", oracle_on_dequantised)
    worst = eng._engine_vs_oracle(MID, [5, 16, 17, 63, 130, 31], enforce_eager=False, seed=11, tol=6e-2, quantization="int4")
    print(f"int4 engine: worst |logit - oracle| = {worst:.3e}")
