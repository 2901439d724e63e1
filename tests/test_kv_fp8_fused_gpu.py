"""The fused fp8-KV decode step (mi_paged_attn_decode_fp8kv_fused): q/k-norm + RoPE + quantising store + attention in
one launch against the launch sequence it replaces (bit for bit) and against fp64 attention over the dequantised cache."""
import ctypes

import pytest
import torch

from test_kv_fp8_gpu import D, LENS, fp8_caches, kv_rule, rows

EPS = 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("block_size", [16, 256])
@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "norm"])
@pytest.mark.parametrize("hq,hkv", [(2, 2), (16, 8), (16, 2), (16, 1)])
@pytest.mark.parametrize("lens", [LENS, LENS * 3, [700]], ids=["batch7", "batch21_unsplit", "batch1_split"])
def test_fused_step_equals_its_launch_sequence_and_fp64_attention(lens, hq, hkv, norm, block_size):
    from nanovllm import ops

    g, scale, n_seq, bs = hq // hkv, D ** -0.5, len(lens), block_size
    ctx = torch.tensor(lens + [0], dtype=torch.int32)  # the last row is graph padding: no context, slot (-1, -1)
    nb = [-(-n // bs) for n in lens]
    nblk = sum(nb) + 3
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(5)).int()
    tables = torch.full((n_seq + 1, max(nb)), -1, dtype=torch.int32)
    cache = fp8_caches(nblk, hkv, bs)
    flat, used = [], 0  # flat slots of every position of every sequence
    for i, n in enumerate(lens):
        tables[i, : nb[i]] = perm[used: used + nb[i]]
        used += nb[i]
        pos = torch.arange(n)
        flat.append((tables[i][pos // bs] * bs + pos % bs).int())
        if n > 1:  # the context before this step
            ops.kv_store_fp8(rows(n - 1, hkv, 10 + i).cuda(), rows(n - 1, hkv, 40 + i).cuda(), cache[0], cache[1],
                             flat[i][:-1].cuda(), hkv, bs)
    last = torch.stack([f[-1] for f in flat])
    slots = torch.cat([torch.stack([last // bs, last % bs], 1), torch.tensor([[-1, -1]])]).int().cuda()
    qkv = rows(n_seq + 1, hq + 2 * hkv, 6)
    qkv[n_seq // 2, [hq, hq + hkv]] = 0  # an all-zero K row and V row (kv head 0 of one sequence): scale 1, bytes 0
    qkv = qkv.view(n_seq + 1, -1).cuda()
    gen = torch.Generator().manual_seed(7)
    qw, kw = ((1 + 0.2 * torch.randn(D, generator=gen)).bfloat16().cuda() for _ in range(2)) if norm else (None, None)
    ang = torch.rand(max(lens), D // 2, generator=gen) * 6.2832
    cos_sin = torch.cat([ang.cos(), ang.sin()], 1).cuda()
    positions = (ctx.long() - 1).clamp(min=0).cuda()
    tables, ctx = tables.cuda(), ctx.cuda()

    # 1. the launches it replaces: norm + RoPE (through a scratch bf16 cache), quantising store, attention
    scratch = torch.zeros((2, *ops.kv_cache_shape(nblk, hkv, bs)), dtype=torch.bfloat16, device="cuda")
    q = ops.qknorm_rope_store(qkv, qw, kw, EPS, positions, cos_sin, scratch[0], scratch[1], slots, hq, hkv, bs)
    k_new = ops.kv_cache_gather(scratch[0], False, last.cuda(), hkv, bs).view(n_seq, hkv, D)
    v_new = qkv[:n_seq, (hq + hkv) * D:].view(n_seq, hkv, D)
    want_cache = cache.clone()
    ops.kv_store_fp8(k_new, v_new, want_cache[0], want_cache[1], slots[:n_seq].contiguous(), hkv, bs)
    want = ops.paged_attn_decode_fp8kv(q, want_cache[0], want_cache[1], tables, ctx, hq, hkv, bs, scale)
    out = ops.paged_attn_decode_fp8kv_fused(qkv, qw, kw, EPS, positions, cos_sin, slots, cache[0], cache[1], tables, ctx,
                                            hq, hkv, bs, scale)
    assert torch.equal(out, want)
    assert torch.equal(cache, want_cache)  # data and scales; nothing else moved (the padding row stored nothing)
    assert (out[n_seq] == 0).all()

    # 2. fp64 attention over the dequantised cache as the fused launch left it
    every = torch.cat(flat).cuda()
    deq = []
    for is_v in (False, True):
        b8, s = ops.kv_cache_gather_fp8(cache[int(is_v)], is_v, every, hkv, bs)
        b8, s = b8.cpu().view(-1, hkv, D), s.cpu()
        deq.append(b8.view(torch.float8_e4m3fn).double() * s[..., None].double())
        wq, ws, _ = kv_rule((v_new if is_v else k_new).cpu())  # the new rows follow the rule
        at = torch.tensor(lens).cumsum(0) - 1
        assert torch.equal(b8[at], wq) and torch.equal(s[at], ws)
    ref, o = [], 0
    for n in lens:
        kd, vd = (x[o: o + n].repeat_interleave(g, 1) for x in deq)
        p = torch.softmax(torch.einsum("hd,nhd->hn", q[len(ref)].view(hq, D).double().cpu(), kd) * scale, -1)
        ref.append(torch.einsum("hn,nhd->hd", p, vd).reshape(-1))
        o += n
    got = out[:n_seq].double().cpu()
    err = (got - torch.stack(ref)).abs() - 2.0 ** -8 * got.abs()
    print(f"worst |out - ref| - 2^-8 |out| = {err.max().item():.3e} (allowed 1e-4)")
    assert err.max().item() <= 1e-4


def test_fused_entry_point_is_exported_and_checks_its_arguments():
    from nanovllm import _C

    assert "mi_paged_attn_decode_fp8kv_fused" in _C.EXPORTED_SYMBOLS
    p, eps, sc = 1 << 20, ctypes.c_float(EPS), ctypes.c_float(0.1)  # a 16-byte aligned address that is never followed

    def call(qkv=p, q_w=p, k_w=p, pos=p, cs=p, slots=p, kc=p, out=p, hq=16, hkv=8, head_dim=128):
        return _C.lib.mi_paged_attn_decode_fp8kv_fused(qkv, 4096, q_w, k_w, eps, pos, cs, slots, kc, p, p, 4, p, out, p,
                                                       1 << 30, 0, hq, hkv, head_dim, 16, sc, None)

    assert call() == 0  # batch 0: checked, nothing launched
    for null in ("qkv", "pos", "cs", "slots", "kc", "out"):
        assert call(**{null: None}) == -1, null  # MI_EINVAL
    assert call(k_w=None) == -1 and call(q_w=None) == -1 and call(q_w=None, k_w=None) == 0  # both or neither
    assert call(head_dim=64) == -2 and call(hq=14, hkv=2) == -2  # MI_EUNSUPPORTED
