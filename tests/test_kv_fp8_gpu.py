"""Opt-in fp8 (e4m3) KV cache: store, decode attention, expansion for prefill, and the engine on top of them
(csrc/paged_attn_fp8kv.hip).  The quantisation rule is fixed (include/mi355_nanovllm.h), so content checks are exact and
the attention bound is the bf16 kernels' own: attention over the dequantised rows."""
import pytest
import torch

from model_configs import TINY, TINY_LLAMA_HD64, make_model_dir

pytestmark = pytest.mark.gpu
D = 128


def kv_rule(x):
    """The rule on the CPU: per row of 128, scale = 2^max(floor(log2 amax) - 7, -120) (1 for a zero row),
    q = RNE_e4m3fn(x / scale).  Returns (e4m3 bytes, scales, dequantised rows in x's dtype)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    e = torch.where(amax > 0, (torch.frexp(amax)[1] - 8).clamp(min=-120), torch.zeros_like(amax, dtype=torch.int32))
    scale = torch.ldexp(torch.ones_like(amax), e)
    q = torch.ldexp(xf, -e[..., None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale, (q.float() * scale[..., None]).to(x.dtype)


def rows(n, hkv, seed):
    """[n, hkv, 128] bf16 rows whose magnitudes differ by 2^-6 .. 2^3 between tokens and heads."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.ldexp(torch.ones(n, hkv, 1), torch.randint(-6, 4, (n, hkv, 1), generator=g))
    return (torch.randn(n, hkv, D, generator=g) * mag).to(torch.bfloat16)


def fp8_caches(nblk, hkv, bs):
    from nanovllm import ops

    return torch.zeros((2, *ops.kv_cache_shape_fp8(nblk, hkv, bs)), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("block_size", [16, 256])
@pytest.mark.parametrize("pairs", [False, True])
def test_store_is_bit_exact(pairs, block_size):
    from nanovllm import ops

    hkv, n, nblk = 2, 40, 5
    k, v = rows(n, hkv, 1), rows(n, hkv, 2)
    k[3] = 0  # an all-zero row: scale 1, bytes 0
    slots = torch.randperm(nblk * block_size, generator=torch.Generator().manual_seed(3))[:n].int()
    slots[7] = -1  # skipped
    cache = fp8_caches(nblk, hkv, block_size)
    cache[:, :, :, :, :2048] = 0x5A  # what was there before
    arg = torch.stack([slots // block_size, slots % block_size], 1) if pairs else slots
    arg = torch.where(slots[:, None] < 0, -1, arg) if pairs else arg
    ops.kv_store_fp8(k.cuda(), v.cuda(), cache[0], cache[1], arg.int().contiguous().cuda(), hkv, block_size)
    every = torch.arange(nblk * block_size, dtype=torch.int32)
    written = torch.zeros(nblk * block_size, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    for is_v, x in ((False, k), (True, v)):
        q, s = ops.kv_cache_gather_fp8(cache[int(is_v)], is_v, every.cuda(), hkv, block_size)
        q, s = q.cpu().view(-1, hkv, D), s.cpu()
        wq, ws, _ = kv_rule(x)
        keep = slots >= 0
        assert torch.equal(q[slots[keep].long()], wq[keep]) and torch.equal(s[slots[keep].long()], ws[keep])
        assert (q[~written] == 0x5A).all() and (s[~written] == 0).all()  # slots not written stay as they were


LENS = [1, 15, 16, 17, 33, 257, 700]  # single-tile tail, chunk boundary, run boundaries, every wave busy


@pytest.mark.parametrize("block_size", [16, 256])
@pytest.mark.parametrize("hq,hkv", [(16, 8), (16, 2)])
@pytest.mark.parametrize("lens", [LENS, LENS * 3, [700]], ids=["batch7", "batch21_unsplit", "batch1_split"])
def test_decode_attention_matches_fp64_over_the_dequantised_cache(lens, hq, hkv, block_size):
    from nanovllm import ops

    g, scale = hq // hkv, D ** -0.5
    nb = [-(-n // block_size) for n in lens]
    nblk = sum(nb) + 3
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(5)).int()
    tables = torch.full((len(lens), max(nb)), -1, dtype=torch.int32)
    cache = fp8_caches(nblk, hkv, block_size)
    q = rows(len(lens), hq, 6)
    want, used = [], 0
    for i, n in enumerate(lens):
        tables[i, : nb[i]] = perm[used: used + nb[i]]
        used += nb[i]
        k, v = rows(n, hkv, 10 + i), rows(n, hkv, 40 + i)
        pos = torch.arange(n)
        slots = (tables[i][pos // block_size] * block_size + pos % block_size).int()
        ops.kv_store_fp8(k.cuda(), v.cuda(), cache[0], cache[1], slots.cuda(), hkv, block_size)
        kd, vd = (kv_rule(x)[2].double().repeat_interleave(g, 1) for x in (k, v))  # [n, hq, D]
        p = torch.softmax(torch.einsum("hd,nhd->hn", q[i].double(), kd) * scale, -1)
        want.append(torch.einsum("hn,nhd->hd", p, vd))
    want = torch.stack(want).reshape(len(lens), hq * D)
    ctx = torch.tensor(lens, dtype=torch.int32).cuda()
    out = ops.paged_attn_decode_fp8kv(q.cuda(), cache[0], cache[1], tables.cuda(), ctx, hq, hkv, block_size, scale)
    err = (out.double().cpu() - want).abs() - 2.0 ** -8 * out.double().cpu().abs()
    print(f"worst |out - ref| - 2^-8 |out| = {err.max().item():.3e} (allowed 1e-4)")
    assert err.max().item() <= 1e-4
    # paging invariance: an identity table over a permuted copy of the cache gives the same bits
    order = perm[:used].long().cuda()
    ident = torch.full_like(tables, -1)
    ident[tables >= 0] = torch.arange(used, dtype=torch.int32)
    out2 = ops.paged_attn_decode_fp8kv(q.cuda(), cache[0][order].contiguous(), cache[1][order].contiguous(),
                                       ident.cuda(), ctx, hq, hkv, block_size, scale)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("block_size", [16, 48])
def test_expand_fills_the_bf16_scratch_with_the_dequantised_rows(block_size):
    from nanovllm import ops

    hkv, nblk, lens = 2, 7, [2 * block_size, block_size + 5]  # the second sequence ends in a partial block
    tables = torch.tensor([[5, 1], [3, 6]], dtype=torch.int32)
    cache = fp8_caches(nblk, hkv, block_size)
    scratch = torch.full((2, *ops.kv_cache_shape(nblk, hkv, block_size)), 7.0, dtype=torch.bfloat16, device="cuda")
    kv, slots = [], []
    for i, n in enumerate(lens):
        pos = torch.arange(n)
        slots.append((tables[i][pos // block_size] * block_size + pos % block_size).int())
        kv.append((rows(n, hkv, 20 + i), rows(n, hkv, 30 + i)))
        ops.kv_store_fp8(kv[i][0].cuda(), kv[i][1].cuda(), cache[0], cache[1], slots[i].cuda(), hkv, block_size)
    ops.kv_fp8_expand(cache[0], cache[1], scratch[0], scratch[1], tables.cuda(),
                      torch.tensor(lens, dtype=torch.int32).cuda(), hkv, block_size)
    for i in range(len(lens)):
        for is_v in (False, True):
            got = ops.kv_cache_gather(scratch[int(is_v)], is_v, slots[i].cuda(), hkv, block_size).cpu()
            assert torch.equal(got.view(-1, hkv, D), kv_rule(kv[i][int(is_v)])[2])
    assert (scratch[:, [0, 2, 4]] == 7.0).all()  # blocks no table references are left alone


def run_engine_against_oracle(kv_cache_dtype, enforce_eager, patch):
    """Greedy run of the tiny 2-layer Qwen3 against the oracle fed the same schedule; the second request hits the
    prefix cache and the decode steps cross a block boundary.  Returns the worst |logit| deviation (|logit| <= 4)."""
    from nanovllm import LLM, SamplingParams
    from nanovllm.engine import batch_meta
    from test_engine_gpu import _oracle_for

    tol = 4e-2
    llm = LLM(make_model_dir(TINY), kvcache_block_size=16, max_num_seqs=8, max_num_batched_tokens=1024,
              max_model_len=512, num_kvcache_blocks=40, enforce_eager=enforce_eager, warmup=False, synthetic_seed=7,
              kv_cache_dtype=kv_cache_dtype)
    try:
        if patch is not None:
            from oracle import layers as oracle_layers

            plain = oracle_layers.kv_scatter
            patch.setattr(oracle_layers, "kv_scatter",
                          lambda k, v, *a: plain(kv_rule(k)[2], kv_rule(v)[2], *a))
        oracle = _oracle_for(llm, TINY, 7)
        gen = torch.Generator().manual_seed(3)
        first = torch.randint(0, TINY["vocab_size"], (29,), generator=gen).tolist()
        second = first[:16] + torch.randint(0, TINY["vocab_size"], (13,), generator=gen).tolist()
        worst, cached = 0.0, 0
        for prompt in (first, second):
            llm.add_request(prompt, SamplingParams(max_tokens=6, ignore_eos=True, greedy=True))
            while not llm.is_finished():
                seqs, is_prefill = llm.scheduler.schedule()
                if is_prefill:
                    m = batch_meta.prefill_meta(seqs, 16)
                    cached += sum(s.num_cached_tokens for s in seqs)
                    want = oracle.prefill(torch.from_numpy(m.input_ids), torch.from_numpy(m.positions),
                                          torch.from_numpy(m.cu_seqlens_q), torch.from_numpy(m.slot_mapping),
                                          torch.from_numpy(m.block_tables), fp32_logits=True)
                else:
                    m = batch_meta.decode_meta(seqs)
                    want = oracle.decode(torch.from_numpy(m.input_ids), torch.from_numpy(m.positions),
                                         torch.from_numpy(m.slot_mapping), torch.from_numpy(m.context_lens),
                                         torch.from_numpy(m.block_tables), fp32_logits=True)
                toks = llm.model_runner.call("run", seqs, is_prefill)
                got = llm.model_runner.last_logits[: len(seqs)].float().cpu()
                worst = max(worst, (got - want).abs().max().item())
                top2 = want.topk(2, dim=-1).values
                for row, (a, b) in enumerate(zip(toks, want.argmax(-1).tolist())):
                    if float(top2[row, 0] - top2[row, 1]) > 2 * tol:
                        assert a == b, (row, a, b)
                llm.scheduler.postprocess(seqs, want.argmax(-1).tolist())
        assert cached == 16, cached
        return worst
    finally:
        llm.exit()


@pytest.mark.parametrize("enforce_eager", [True, False])
def test_engine_with_fp8_cache_matches_the_oracle_on_quantised_rows(monkeypatch, enforce_eager):
    worst = run_engine_against_oracle("fp8", enforce_eager, monkeypatch)
    print(f"worst logit deviation {worst:.3e} (allowed 4e-2)")
    assert worst <= 4e-2, worst


def test_fp8_cache_refuses_what_it_is_not_built_for():
    from nanovllm.config import Config

    with pytest.raises(NotImplementedError, match="head_dim 64"):
        Config(make_model_dir(TINY_LLAMA_HD64), kv_cache_dtype="fp8")
    with pytest.raises(NotImplementedError, match="tensor_parallel_size"):
        Config(make_model_dir(dict(TINY, num_attention_heads=4, num_key_value_heads=2)), kv_cache_dtype="fp8",
               tensor_parallel_size=2)
