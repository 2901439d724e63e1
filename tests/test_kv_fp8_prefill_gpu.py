"""Prefill over the fp8 KV cache without the bf16 scratch (csrc/prefill_fp8kv.hip): the attention kernel that reads the
e4m3 tiles against fp64 attention over the dequantised rows, its fused-Q form and the fused K / V store against the
launches they replace (bit for bit), and the engine against its own MI355_FP8_PREFILL=expand form."""
import functools

import pytest
import torch

from model_configs import TINY, make_model_dir
from test_kv_fp8_gpu import D, kv_rule, rows

pytestmark = pytest.mark.gpu
EPS = 1e-6
Q_LENS = [1, 7, 16, 33, 129, 260]   # single key, partial tile, tile and chunk boundaries, several query blocks per pair
KV_LENS = [1, 7, 16, 33, 193, 260]  # the fifth sequence has a 64-token cached prefix


def filled_caches(nblk, hkv, bs):
    """[2, nblk, hkv, bs / 16, 2112] with every tile holding data bytes 0x5A and scales 1.0: a masking slip shows."""
    from nanovllm import ops

    tile = torch.cat([torch.full((2048,), 0x5A, dtype=torch.uint8), torch.ones(16).view(torch.uint8)])
    return tile.expand(2, *ops.kv_cache_shape_fp8(nblk, hkv, bs)).contiguous().cuda()


def rope_table(n):
    ang = torch.rand(n, D // 2, generator=torch.Generator().manual_seed(7)) * 6.2832
    return torch.cat([ang.cos(), ang.sin()], 1).cuda()


@functools.lru_cache(maxsize=None)
def attention_case(hq, hkv):
    """q / k / v rows of every sequence and fp64 causal attention over the dequantised rows, with V and with |V|."""
    g, out = hq // hkv, []
    for i, (nq, nk) in enumerate(zip(Q_LENS, KV_LENS)):
        q, k, v = rows(nq, hq, 60 + i), rows(nk, hkv, 10 + i), rows(nk, hkv, 40 + i)
        kd, vd = (kv_rule(x)[2].double().repeat_interleave(g, 1) for x in (k, v))
        s = torch.einsum("qhd,nhd->hqn", q.double(), kd) * D ** -0.5
        seen = torch.arange(nk)[None, :] <= torch.arange(nq)[:, None] + (nk - nq)
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), -1)
        out.append((q, k, v, torch.einsum("hqn,nhd->qhd", p, vd), torch.einsum("hqn,nhd->qhd", p, vd.abs())))
    return out


@pytest.mark.parametrize("block_size", [16, 48, 256])
@pytest.mark.parametrize("hq,hkv", [(16, 8), (8, 8), (16, 1), (4, 1)])
def test_prefill_attention_matches_fp64_over_the_dequantised_rows(hq, hkv, block_size):
    from nanovllm import ops

    bs, case = block_size, attention_case(hq, hkv)
    nb = [-(-n // bs) for n in KV_LENS]
    nblk = sum(nb) + 3
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(5)).int()
    tables = torch.full((len(KV_LENS), max(nb)), -1, dtype=torch.int32)
    cache, used = filled_caches(nblk, hkv, bs), 0
    for i, (_, k, v, _, _) in enumerate(case):
        tables[i, : nb[i]] = perm[used: used + nb[i]]
        used += nb[i]
        pos = torch.arange(KV_LENS[i])
        slots = (tables[i][pos // bs] * bs + pos % bs).int()
        ops.kv_store_fp8(k.cuda(), v.cuda(), cache[0], cache[1], slots.cuda(), hkv, bs)
    q = torch.cat([c[0] for c in case]).cuda()
    want, want_absv = (torch.cat([c[j] for c in case]).reshape(-1, hq * D) for j in (3, 4))
    cu = torch.tensor([0] + Q_LENS).cumsum(0).int().cuda()
    kvl = torch.tensor(KV_LENS, dtype=torch.int32).cuda()
    out = ops.paged_attn_prefill_fp8kv(q, cache[0], cache[1], tables.cuda(), cu, kvl, max(Q_LENS), hq, hkv, bs, D ** -0.5)
    # tests/test_kernels_gpu.py::_prefill_bound with P as one bf16 per key
    used_up = (out.double().cpu() - want).abs() / (want.abs() * 2 ** -8 + want_absv * 2 ** -8 + 1e-4)
    print(f"worst |out - ref| / bound = {used_up.max().item():.3f} (allowed 1)")
    assert used_up.max().item() <= 1
    # paging invariance: an identity table over a permuted copy of the cache gives the same bits
    order = perm[:used].long().cuda()
    ident = torch.full_like(tables, -1)
    ident[tables >= 0] = torch.arange(used, dtype=torch.int32)
    out2 = ops.paged_attn_prefill_fp8kv(q, cache[0][order].contiguous(), cache[1][order].contiguous(), ident.cuda(), cu,
                                        kvl, max(Q_LENS), hq, hkv, bs, D ** -0.5)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "norm"])
@pytest.mark.parametrize("hq,hkv", [(4, 2), (16, 1)])
def test_fused_q_equals_prepared_q(hq, hkv, norm):
    from nanovllm import ops

    bs, q_lens, kv_lens = 16, [70, 45], [70, 85]  # the second sequence sits behind 40 cached tokens
    T, nblk = sum(q_lens), 12
    qkv = rows(T, hq + 2 * hkv, 6).view(T, -1).cuda()
    gen = torch.Generator().manual_seed(8)
    qw, kw = ((1 + 0.2 * torch.randn(D, generator=gen)).bfloat16().cuda() for _ in range(2)) if norm else (None, None)
    positions = torch.cat([torch.arange(70), 40 + torch.arange(45)]).cuda()
    cos_sin = rope_table(128)
    cache = filled_caches(nblk, hkv, bs)
    tables = torch.tensor([[3, 9, 0, 7, 5, -1], [11, 1, 8, 2, 6, 4]], dtype=torch.int32)
    for i, n in enumerate(kv_lens):
        pos = torch.arange(n)
        ops.kv_store_fp8(rows(n, hkv, 20 + i).cuda(), rows(n, hkv, 30 + i).cuda(), cache[0], cache[1],
                         (tables[i][pos // bs] * bs + pos % bs).int().cuda(), hkv, bs)
    throwaway = torch.zeros((2, *ops.kv_cache_shape(nblk, hkv, bs)), dtype=torch.bfloat16, device="cuda")
    q = ops.qknorm_rope_store(qkv, qw, kw, EPS, positions, cos_sin, throwaway[0], throwaway[1],
                              torch.arange(T, dtype=torch.int32).cuda(), hq, hkv, bs)
    args = (cache[0], cache[1], tables.cuda(), torch.tensor([0, 70, 115], dtype=torch.int32).cuda(),
            torch.tensor(kv_lens, dtype=torch.int32).cuda(), max(q_lens), hq, hkv, bs, D ** -0.5)
    want = ops.paged_attn_prefill_fp8kv(q, *args)
    out = ops.paged_attn_prefill_fp8kv_fused(qkv, qw, EPS, positions, cos_sin, *args)
    assert want.abs().max() > 0 and torch.equal(out, want)


@pytest.mark.parametrize("block_size", [16, 48])
@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "norm"])
def test_fused_store_equals_its_launch_sequence(norm, block_size):
    from nanovllm import ops

    hq, hkv, bs, T, nblk = 4, 2, block_size, 100, 12
    # runs of slots: block-aligned (whole tiles), starting mid-tile, a ragged tail, and two skipped tokens
    slots = torch.cat([2 * bs + torch.arange(48), 7 * bs + 5 + torch.arange(30), 5 * bs + torch.arange(22)]).int()
    slots[[50, 97]] = -1
    qkv = rows(T, hq + 2 * hkv, 9)
    qkv[3, [hq, hq + hkv]] = 0  # an all-zero K row and V row: scale 1, bytes 0
    qkv = qkv.view(T, -1).cuda()
    kw = (1 + 0.2 * torch.randn(D, generator=torch.Generator().manual_seed(4))).bfloat16().cuda() if norm else None
    positions, cos_sin = (torch.arange(T) * 3 % 128).cuda(), rope_table(128)
    want, got = filled_caches(nblk, hkv, bs), filled_caches(nblk, hkv, bs)
    q3, k3, v3 = (x.view(T, -1, D) for x in qkv.split([hq * D, hkv * D, hkv * D], dim=-1))
    k_rot = ops.rope(positions, q3, ops.rmsnorm(k3, kw, EPS) if norm else k3, cos_sin, hq, hkv)[1]
    ops.kv_store_fp8(k_rot, v3, want[0], want[1], slots.cuda(), hkv, bs)
    ops.qknorm_rope_store_fp8(qkv, kw, EPS, positions, cos_sin, got[0], got[1], slots.cuda(), hq, hkv, bs)
    every = torch.arange(nblk * bs, dtype=torch.int32).cuda()
    written = torch.zeros(nblk * bs, dtype=torch.bool)
    written[slots[slots >= 0].long()] = True
    for is_v in (False, True):
        b_want, s_want = ops.kv_cache_gather_fp8(want[int(is_v)], is_v, every, hkv, bs)
        b_got, s_got = ops.kv_cache_gather_fp8(got[int(is_v)], is_v, every, hkv, bs)
        assert torch.equal(b_got, b_want) and torch.equal(s_got, s_want)
        assert (b_got.cpu()[~written] == 0x5A).all() and (s_got.cpu()[~written] == 1).all()  # untouched slots
        assert (b_got.cpu()[written] != 0x5A).any()
    assert torch.equal(got, want)


def greedy_run(enforce_eager, forced=None):
    """Two prompts - 150 tokens (the module-by-module forward), then 70 new tokens behind 32 cached ones (the streaming
    forward); every step's logits.  `forced`: the tokens to continue with (the other run's), so that both runs see
    the same sequences."""
    from nanovllm import LLM, SamplingParams

    llm = LLM(make_model_dir(TINY), kvcache_block_size=16, max_num_seqs=8, max_num_batched_tokens=1024, max_model_len=512,
              num_kvcache_blocks=40, enforce_eager=enforce_eager, warmup=False, synthetic_seed=7, kv_cache_dtype="fp8")
    try:
        scratch = llm.model_runner.kv_scratch
        gen = torch.Generator().manual_seed(3)
        first = torch.randint(0, TINY["vocab_size"], (150,), generator=gen).tolist()
        second = first[:32] + torch.randint(0, TINY["vocab_size"], (70,), generator=gen).tolist()
        steps, cached = [], 0
        for prompt in (first, second):
            llm.add_request(prompt, SamplingParams(max_tokens=6, ignore_eos=True, greedy=True))
            while not llm.is_finished():
                seqs, is_prefill = llm.scheduler.schedule()
                cached += sum(s.num_cached_tokens for s in seqs) if is_prefill else 0
                toks = llm.model_runner.call("run", seqs, is_prefill)
                steps.append((toks, llm.model_runner.last_logits[: len(seqs)].float().cpu()))
                llm.scheduler.postprocess(seqs, forced[len(steps) - 1][0] if forced else toks)
        assert cached == 32, cached
        return scratch, steps
    finally:
        llm.exit()


@pytest.mark.parametrize("enforce_eager", [True, False])
def test_engine_prefill_attends_the_fp8_cache_without_a_scratch(monkeypatch, enforce_eager):
    monkeypatch.setenv("MI355_FP8_PREFILL", "expand")
    scratch, expand = greedy_run(enforce_eager)
    assert scratch is not None
    monkeypatch.delenv("MI355_FP8_PREFILL")
    scratch, direct = greedy_run(enforce_eager, forced=expand)
    assert scratch is None and len(direct) == len(expand)
    for (toks, _), (want_toks, logits) in zip(direct, expand):
        top2 = logits.topk(2, dim=-1).values
        for row, (a, b) in enumerate(zip(toks, want_toks)):
            if float(top2[row, 0] - top2[row, 1]) > 2 * 4e-2:  # twice the engine bound of test_kv_fp8_gpu.py
                assert a == b, (row, a, b)
