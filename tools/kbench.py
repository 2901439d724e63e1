#!/usr/bin/env python3
"""Kernel micro-benchmarks on one MI355X (HIP events on the launch stream).

Reports each hot kernel's duration and its fraction of the 8 TB/s HBM roofline
at the BASELINE shapes (Qwen3-0.6B, bs=32, ctx=1024, block 16).  Buffers are
cycled over 28 "layers" so nothing is served from the 256 MiB Infinity Cache.
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nano-vllm-ascend_amd"))
from nanovllm import _C, ops  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def timeit(fn, n_layers, iters=5, warm=2, reps=None):
    """Capture `n_layers` back-to-back launches into a hipGraph (removes the ~10 us
    python/ctypes launch cost) and time `iters` replays with HIP events."""
    reps = reps or max(1, 28 // n_layers)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for l in range(n_layers):
            fn(l)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            for l in range(n_layers):
                fn(l)
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / (iters * n_layers * reps)


def prefill_attention():
    """One prefill step of the bench: 16 prompts x 1024 tokens, Qwen3-0.6B heads (causal, through the paged cache)."""
    n, T, bs, hq, hkv, L = 16, int(os.environ.get("CTX", 1024)), 16, 16, 8, 4
    nb = (T + bs - 1) // bs
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = [torch.randn(ops.kv_cache_shape(n * nb, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    vc = [torch.randn(ops.kv_cache_shape(n * nb, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    tables = torch.randperm(n * nb, generator=g).to(torch.int32).view(n, nb).to(DEV)
    q = torch.randn(n * T, hq * 128, device=DEV).bfloat16()
    out = torch.empty_like(q)
    cu = (torch.arange(n + 1, dtype=torch.int32) * T).to(DEV)
    kvl = torch.full((n,), T, dtype=torch.int32, device=DEV)
    t = timeit(lambda l: ops.paged_attn_prefill(q, kc[l], vc[l], tables, cu, kvl, T, hq, hkv, bs, 128 ** -0.5, out=out), L)
    flops = n * hq * (T * (T + 1) / 2) * 128 * 2 * 2  # causal QK^T + PV, useful flops (the hi/lo P split is not counted)
    print(f"paged_attn_prefill 16x{T}: {t * 1e6:9.1f} us   {flops / t / 1e12:7.1f} TFLOP/s useful "
          f"({flops / t / 2.5e15:.3f} of 2.5 PFLOP/s bf16)")


def prefill_attention_order():
    """The fused-Q prefill attention (q-norm + RoPE in the Q-operand load) in every variant of its _ex entry point,
    alternating rounds (KBENCH_ONLY=prefill_order)."""
    n, T, bs, hq, hkv, L = 16, int(os.environ.get("CTX", 1024)), 16, 16, 8, 4
    nb = (T + bs - 1) // bs
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = [torch.randn(ops.kv_cache_shape(n * nb, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    vc = [torch.randn(ops.kv_cache_shape(n * nb, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    tables = torch.randperm(n * nb, generator=g).to(torch.int32).view(n, nb).to(DEV)
    qkv = torch.randn(n * T, (hq + 2 * hkv) * 128, device=DEV).bfloat16()
    qw = torch.ones(128, device=DEV).bfloat16()
    pos = torch.arange(T, dtype=torch.int64).repeat(n).to(DEV)
    inv = 1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128))
    fr = torch.arange(T).float()[:, None] * inv[None]
    cos_sin = torch.cat([fr.cos(), fr.sin()], -1).to(DEV)
    out = torch.empty(n * T, hq * 128, device=DEV).bfloat16()
    cu = (torch.arange(n + 1, dtype=torch.int32) * T).to(DEV)
    kvl = torch.full((n,), T, dtype=torch.int32, device=DEV)
    # variant bits of mi_paged_attn_prefill_fused_ex (include/mi355_nanovllm.h)
    variants = (("default (round 6: sum-checked softmax, scalar request addressing)", 0),
                ("round-5 softmax: chunk maximum before the exponentials (32)", 32),
                ("round-5 request addressing: 64-bit VALU pointers + global_load_lds (64)", 64),
                ("the round-5 kernel as a whole (96)", 96),
                ("P as bf16 hi + lo (4)", 4),
                ("round-3 V reads: ds_read2st64_b64 (8)", 8),
                ("round-3 request path: table read + divisions per chunk (16)", 16),
                ("both round-3 forms, P bf16 (24)", 24),
                ("the round-3 kernel as a whole: P hi + lo (28)", 28),
                ("requests ahead of the Q preparation (1)", 1),
                ("one barrier per two chunks, ring of four (2)", 2))
    res = {name: [] for name, _ in variants}
    for rnd in range(int(os.environ.get("ROUNDS", 4))):
        for name, v in variants:
            t = timeit(lambda l: ops.paged_attn_prefill_fused(qkv, qw, 1e-6, pos, cos_sin, kc[l], vc[l], tables, cu, kvl, T,
                                                              hq, hkv, bs, 128 ** -0.5, out=out, variant=v), L)
            res[name].append(round(t * 1e6, 1))
    flops = n * hq * (T * (T + 1) / 2) * 128 * 2 * 2
    print(f"fused-Q prefill attention 16x{T}, us per launch, alternating rounds ({flops / 1e9:.1f} GFLOP useful per launch):")
    for k, v in res.items():
        best = min(v)
        print(f"  {k}: {v}   best {flops / best / 1e6:.0f} TFLOP/s")


def plain_attention():
    """The reference README's small-model head geometries (KBENCH_ONLY=plain): decode bs 32 x ctx 1024 (HBM bytes = K + V
    rows of every context token) and prefill 16 x 1024 tokens, on the plain-layout family (csrc/attn_plain.hip, the
    round-3 path) and on the fragment-native MFMA kernels over 2 KiB tiles / groups of 7 (round 4)."""
    B, T, bs, L = 32, 1024, 16, 4
    nb = (T + bs - 1) // bs
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, hq, hkv, d in (("Qwen2-0.5B 14/2 x 64", 14, 2, 64), ("Llama-3.2-1B 32/8 x 64", 32, 8, 64),
                             ("Qwen2.5-7B 28/4 x 128", 28, 4, 128)):
        tables = torch.randperm(B * nb, generator=g).to(torch.int32).view(B, nb).to(DEV)
        q = torch.randn(B, hq * d, device=DEV).bfloat16()
        out = torch.empty_like(q)
        ctx = torch.full((B,), T, dtype=torch.int32, device=DEV)
        n = 16
        qp = torch.randn(n * T, hq * d, device=DEV).bfloat16()
        op = torch.empty_like(qp)
        cu = (torch.arange(n + 1, dtype=torch.int32) * T).to(DEV)
        kvl = torch.full((n,), T, dtype=torch.int32, device=DEV)
        byt = B * 2 * T * hkv * d * 2
        flops = n * hq * (T * (T + 1) / 2) * d * 2 * 2
        for family in ("plain layout", "fragment-native"):
            shape = ops.kv_cache_shape_plain(B * nb, hkv, bs, d) if family == "plain layout" else ops.kv_cache_shape(B * nb, hkv, bs, d)
            kc = [torch.randn(shape, device=DEV).bfloat16() for _ in range(L)]
            vc = [torch.randn(shape, device=DEV).bfloat16() for _ in range(L)]
            if family == "plain layout":
                t = timeit(lambda l: ops.paged_attn_decode_plain(q, kc[l], vc[l], tables, ctx, hq, hkv, bs, d ** -0.5, out=out), L)
                tp = timeit(lambda l: ops.paged_attn_prefill_plain(qp, kc[l], vc[l], tables[:n], cu, kvl, T, hq, hkv, bs,
                                                                   d ** -0.5, out=op), L)
            else:
                ws = ops.attn_workspace(DEV, B, hq)
                t = timeit(lambda l: ops.paged_attn_decode(q, kc[l], vc[l], tables, ctx, hq, hkv, bs, d ** -0.5, out=out,
                                                           workspace=ws), L)
                tp = timeit(lambda l: ops.paged_attn_prefill(qp, kc[l], vc[l], tables[:n], cu, kvl, T, hq, hkv, bs, d ** -0.5,
                                                             out=op), L)
            print(f"{name} [{family:15s}]: decode bs {B} ctx {T} {t * 1e6:7.1f} us = {byt / t / 1e9:6.0f} GB/s "
                  f"({byt / t / PEAK:.2f} of 8 TB/s); prefill 16x{T} {tp * 1e6:8.1f} us = {flops / tp / 1e12:5.1f} TFLOP/s useful",
                  flush=True)


def fp8_kv_attention():
    """The fp8-KV decode attention launch beside the bf16 one: bs 32, 8 kv heads x 2, ctx 1049 (the middle of the timed
    bench window), distinct caches per layer, interleaved rounds; and the launches the fp8 path runs in front of it
    (q-norm, k-norm, RoPE, quantising store) where the bf16 path has its fused step prologue."""
    B, c, bs, hq, hkv, L = 32, int(os.environ.get("CTX", 1049)), 16, 16, 8, 28
    nb = (c + bs - 1) // bs
    nblk = B * nb
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = [torch.randn(ops.kv_cache_shape(nblk, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    vc = [torch.randn(ops.kv_cache_shape(nblk, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    # finite e4m3 bytes everywhere (0x7f / 0xff are NaN) and scale 1: timing needs no meaningful values
    k8 = [torch.randint(0, 0x70, ops.kv_cache_shape_fp8(nblk, hkv, bs), dtype=torch.uint8, device=DEV) for _ in range(L)]
    v8 = [torch.randint(0, 0x70, ops.kv_cache_shape_fp8(nblk, hkv, bs), dtype=torch.uint8, device=DEV) for _ in range(L)]
    for t8 in k8 + v8:
        t8[..., 2048:].view(torch.float32).fill_(1.0)
    perm = torch.randperm(nblk, generator=g).to(torch.int32).view(B, nb).to(DEV)
    ctxl = torch.full((B,), c, dtype=torch.int32, device=DEV)
    q = torch.randn(B, hq * 128, device=DEV).bfloat16()
    out = torch.empty(B, hq * 128, dtype=torch.bfloat16, device=DEV)
    ws = ops.attn_workspace(DEV, B, hq)
    qkv = torch.randn(B, (hq + 2 * hkv) * 128, device=DEV).bfloat16()
    q_, k_, v_ = (t.view(B, -1, 128) for t in qkv.split([hq * 128, hkv * 128, hkv * 128], dim=-1))
    w128 = torch.ones(128, device=DEV).bfloat16()
    rope_t = torch.randn(4096, 128, device=DEV)
    pos = torch.full((B,), c - 1, dtype=torch.int64, device=DEV)
    sl = torch.stack([perm[:, (c - 1) // bs], torch.full((B,), (c - 1) % bs, dtype=torch.int32, device=DEV)], 1).contiguous()
    byt16 = B * 2 * c * hkv * 128 * 2
    byt8 = B * 2 * c * hkv * (128 + 4)

    def front(l):
        qr, kr = ops.rope(pos, ops.rmsnorm(q_, w128, 1e-6), ops.rmsnorm(k_, w128, 1e-6), rope_t, hq, hkv)
        ops.kv_store_fp8(kr, v_, k8[l], v8[l], sl, hkv, bs)
        return qr

    for rnd in range(3):
        t = timeit(lambda l: ops.paged_attn_decode(q, kc[l], vc[l], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
        print(f"#{rnd} paged_attn_decode        bf16 KV ctx={c}: {t * 1e6:7.2f} us  {byt16 / 1e6:6.1f} MB  {byt16 / t / PEAK:5.3f} of 8 TB/s")
        t = timeit(lambda l: ops.paged_attn_decode_fp8kv(q, k8[l], v8[l], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
        print(f"#{rnd} paged_attn_decode_fp8kv  fp8 KV  ctx={c}: {t * 1e6:7.2f} us  {byt8 / 1e6:6.1f} MB  {byt8 / t / PEAK:5.3f} of 8 TB/s")
        t = timeit(lambda l: ops.paged_attn_decode_fused(qkv, w128, w128, 1e-6, pos, rope_t, sl, kc[l], vc[l], perm, ctxl, hq, hkv,
                                                         bs, 128 ** -0.5, out=out, workspace=ws), L)
        print(f"#{rnd} bf16 fused step (norm + RoPE + store + attention, one launch): {t * 1e6:7.2f} us")
        t = timeit(front, L)
        print(f"#{rnd} fp8 front launches (q-norm, k-norm, RoPE, quantising store):   {t * 1e6:7.2f} us")
        t = timeit(lambda l: ops.paged_attn_decode_fp8kv(front(l), k8[l], v8[l], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out,
                                                         workspace=ws), L)
        print(f"#{rnd} fp8 step (front launches + attention, five launches):          {t * 1e6:7.2f} us")
        t = timeit(lambda l: ops.paged_attn_decode_fp8kv_fused(qkv, w128, w128, 1e-6, pos, rope_t, sl, k8[l], v8[l], perm, ctxl,
                                                               hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
        print(f"#{rnd} fp8 fused step (norm + RoPE + quantising store + attention, one launch): {t * 1e6:7.2f} us")


def fp8_kv_prefill():
    """The attention side of an fp8-KV prefill layer, six launches over the expansion scratch (q-norm, k-norm, RoPE,
    quantising store, expand, bf16 attention: MI355_FP8_PREFILL=expand) against the two that read the e4m3 tiles
    (fused store, fused-Q attention): the bench's prefill step and a prefix-hit step, alternating rounds, plus the
    pieces on their own (KBENCH_ONLY=fp8kv, or fp8kv_prefill for this part alone)."""
    n, bs, hq, hkv, L = 16, 16, 16, 8, 4
    w128 = torch.ones(128, device=DEV).bfloat16()
    for name, T, ctx in (("prefill step, 16 x 1024 tokens", 1024, 1024), ("prefix hit, 16 x 64 new behind 4032 cached", 64, 4096)):
        nb = ctx // bs
        g = torch.Generator(device="cpu").manual_seed(0)
        k8 = [torch.randint(0, 0x70, ops.kv_cache_shape_fp8(n * nb, hkv, bs), dtype=torch.uint8, device=DEV) for _ in range(L)]
        v8 = [torch.randint(0, 0x70, ops.kv_cache_shape_fp8(n * nb, hkv, bs), dtype=torch.uint8, device=DEV) for _ in range(L)]
        for t8 in k8 + v8:
            t8[..., 2048:].view(torch.float32).fill_(1.0)
        ks, vs = (torch.zeros(ops.kv_cache_shape(n * nb, hkv, bs), dtype=torch.bfloat16, device=DEV) for _ in range(2))
        tables = torch.randperm(n * nb, generator=g).to(torch.int32).view(n, nb)
        pos1 = torch.arange(ctx - T, ctx)
        slots = (tables[:, pos1 // bs] * bs + pos1 % bs).reshape(-1).int().to(DEV)
        pos, tables = pos1.repeat(n).to(DEV), tables.to(DEV)
        qkv = torch.randn(n * T, (hq + 2 * hkv) * 128, device=DEV).bfloat16()
        q_, k_, v_ = (t.view(n * T, -1, 128) for t in qkv.split([hq * 128, hkv * 128, hkv * 128], dim=-1))
        fr = torch.arange(ctx).float()[:, None] / (1e6 ** (torch.arange(0, 128, 2).float() / 128))[None]
        cos_sin = torch.cat([fr.cos(), fr.sin()], -1).to(DEV)
        out = torch.empty(n * T, hq * 128, dtype=torch.bfloat16, device=DEV)
        cu = (torch.arange(n + 1, dtype=torch.int32) * T).to(DEV)
        kvl = torch.full((n,), ctx, dtype=torch.int32, device=DEV)
        sc = 128 ** -0.5

        def six(l):
            qr, kr = ops.rope(pos, ops.rmsnorm(q_, w128, 1e-6), ops.rmsnorm(k_, w128, 1e-6), cos_sin, hq, hkv)
            ops.kv_store_fp8(kr, v_, k8[l], v8[l], slots, hkv, bs)
            ops.kv_fp8_expand(k8[l], v8[l], ks, vs, tables, kvl, hkv, bs)
            ops.paged_attn_prefill(qr, ks, vs, tables, cu, kvl, T, hq, hkv, bs, sc, out=out)

        def two(l):
            ops.qknorm_rope_store_fp8(qkv, w128, 1e-6, pos, cos_sin, k8[l], v8[l], slots, hq, hkv, bs)
            ops.paged_attn_prefill_fp8kv_fused(qkv, w128, 1e-6, pos, cos_sin, k8[l], v8[l], tables, cu, kvl, T, hq, hkv, bs, sc,
                                               out=out)

        qr = ops.rope(pos, ops.rmsnorm(q_, w128, 1e-6), ops.rmsnorm(k_, w128, 1e-6), cos_sin, hq, hkv)[0]
        forms = (("six launches over the scratch", six), ("two launches over the e4m3 tiles", two),
                 ("  expand alone", lambda l: ops.kv_fp8_expand(k8[l], v8[l], ks, vs, tables, kvl, hkv, bs)),
                 ("  bf16 attention over the scratch alone",
                  lambda l: ops.paged_attn_prefill(qr, ks, vs, tables, cu, kvl, T, hq, hkv, bs, sc, out=out)),
                 ("  fp8kv attention alone (prepared q)",
                  lambda l: ops.paged_attn_prefill_fp8kv(qr, k8[l], v8[l], tables, cu, kvl, T, hq, hkv, bs, sc, out=out)),
                 ("  fused fp8 store alone", lambda l: ops.qknorm_rope_store_fp8(qkv, w128, 1e-6, pos, cos_sin, k8[l], v8[l],
                                                                              slots, hq, hkv, bs)))
        res = {k: [] for k, _ in forms}
        for rnd in range(int(os.environ.get("ROUNDS", 4))):
            for k, fn in forms:
                res[k].append(round(timeit(fn, L) * 1e6, 1))
        print(f"fp8-KV prefill, {name} (hq {hq} / hkv {hkv}, block {bs}); us per layer, alternating rounds:")
        for k, v in res.items():
            print(f"  {k}: {v}   median {sorted(v)[len(v) // 2]}", flush=True)
        del k8, v8, ks, vs


def head_and_sampler():
    """The head GEMM (151936 x 1024, 32 rows) alone, with the pick epilogue, and the standalone sampler."""
    M, N, K = 32, 151936, 1024
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) * 0.05).bfloat16()
    wp = ops.pack_weight(w)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    toks = torch.empty(M, dtype=torch.int64, device=DEV)
    rng = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    cand = torch.empty(N // 16 * M * 2, dtype=torch.int32, device=DEV)
    res = {}
    byt = N * K * 2
    for name, temps in (("greedy", torch.zeros(M, device=DEV)), ("sampled", torch.full((M,), 0.8, device=DEV))):
        t = timeit(lambda l: ops.gemm_packed_pick(x, wp, temps, rng, toks, logits=y, candidates=cand), 1, reps=4)
        res[f"head GEMM + pick ({name})"] = {"us": t * 1e6, "frac": byt / t / PEAK}
        t = timeit(lambda l: ops.sample(y, temps, 1, 2, out=toks), 1, reps=4)
        res[f"standalone sampler ({name})"] = {"us": t * 1e6}
    t = timeit(lambda l: ops.gemm_packed(x, wp, out=y), 1, reps=4)
    res["head GEMM"] = {"us": t * 1e6, "frac": byt / t / PEAK}
    print(json.dumps(res, indent=1))


def moe_block():
    """The sparse block of a decode step at Qwen3-30B-A3B widths (hidden 2048, 128 experts x 768, top-8), bs 32
    (TP 1: every expert whole) and as one rank of TP 4 (192 of every expert's 768).  Bytes = the weights of the
    experts that were hit (each streamed once by each grouped GEMM)."""
    H, E, topk, T = 2048, 128, 8, 32
    res = {}
    for tp in (1, 4):
        inter = 768 // tp
        L = 4  # rotate over several layers' weights (TP 1: 1.2 GB per layer, beyond any cache anyway)
        gu = [ops.pack_expert_weights((torch.randn(E, 2 * inter, H, device=DEV) * 0.02).bfloat16()) for _ in range(L)]
        dn = [ops.pack_expert_weights((torch.randn(E, H, inter, device=DEV) * 0.02).bfloat16()) for _ in range(L)]
        x = torch.randn(T, H, device=DEV).bfloat16()
        logits = torch.randn(T, E, device=DEV).bfloat16()
        _, ids, _ = ops.moe_forward(x, logits, gu[0], dn[0], topk)
        hit = int(torch.unique(ids).numel())
        byt = hit * 3 * inter * H * 2
        t = timeit(lambda l: ops.moe_forward(x, logits, gu[l], dn[l], topk), L, reps=3)
        res[f"moe block tp{tp} (route+sort+gate_up+down+combine), {hit}/128 experts hit"] = {
            "us": t * 1e6, "MB": byt / 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
    print(json.dumps(res, indent=1))


def chain_32b_shard():
    """The six non-attention launches of a decode layer on ONE RANK of Qwen3-32B at TP 8 (hidden 5120, 8 q / 1 kv
    heads, intermediate 3200 per rank; all-reduce seams not included), bs 32, over 4 rotating layers."""
    H, hq, hkv, inter, B, L = 5120, 8, 1, 25600 // 8, 32, 4
    mk = lambda n, k: ops.pack_weight((torch.randn(n, k, device=DEV) * 0.02).bfloat16())  # noqa: E731
    qkv = [mk((hq + 2 * hkv) * 128, H) for _ in range(L)]
    o = [mk(H, hq * 128) for _ in range(L)]  # row-parallel projections: complete bf16 rows per rank (TP path);
    gu = [mk(2 * inter, H) for _ in range(L)]  # N = 5120 has enough row tiles for the packed kernel (layers/linear.py)
    dn = [mk(H, inter) for _ in range(L)]
    wn = torch.ones(H, device=DEV).bfloat16()
    x = torch.randn(B, H, device=DEV).bfloat16()
    attn_out = torch.randn(B, hq * 128, device=DEV).bfloat16()
    res_ = torch.randn(B, H, device=DEV).bfloat16()

    def layer(l):
        xn, r = ops.add_rmsnorm(x, res_, wn, 1e-6)
        ops.gemm_packed(xn, qkv[l])
        y = ops.gemm_packed(attn_out, o[l])
        xn, r = ops.add_rmsnorm(y, r, wn, 1e-6)
        a = ops.gemm_packed(xn, gu[l], silu_mul=True)
        ops.gemm_packed(a, dn[l])

    byt = ((hq + 2 * hkv) * 128 * H + H * hq * 128 + 2 * inter * H + H * inter) * 2
    t = timeit(layer, L, reps=3)
    print(json.dumps({"Qwen3-32B TP8 rank shard, 6 launches per layer": {
        "us": t * 1e6, "MB": byt / 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}}, indent=1))


def chain_32b_one_gpu():
    """The six non-attention launches of a decode layer of the UNSHARDED Qwen3-32B (hidden 5120, 64 q / 8 kv heads,
    intermediate 25600) on one GPU, bs 32, over 2 rotating layers: the row-parallel projections as complete rows +
    add_rmsnorm, and as split-K 4 partials + add_rmsnorm_splitk (models/qwen3.py::_ksplit for long K)."""
    H, hq, hkv, inter, B, L = 5120, 64, 8, 25600, 32, 2
    mk = lambda n, k: ops.pack_weight((torch.randn(n, k, device=DEV) * 0.02).bfloat16())  # noqa: E731
    qkv = [mk((hq + 2 * hkv) * 128, H) for _ in range(L)]
    o = [mk(H, hq * 128) for _ in range(L)]
    gu = [mk(2 * inter, H) for _ in range(L)]
    dn = [mk(H, inter) for _ in range(L)]
    wn = torch.ones(H, device=DEV).bfloat16()
    x = torch.randn(B, H, device=DEV).bfloat16()
    attn_out = torch.randn(B, hq * 128, device=DEV).bfloat16()
    res_ = torch.randn(B, H, device=DEV).bfloat16()
    parts0 = torch.randn(4, B, H, device=DEV) * 0.1

    def rows(l):
        xn, r = ops.add_rmsnorm(x, res_, wn, 1e-6)
        ops.gemm_packed(xn, qkv[l])
        y = ops.gemm_packed(attn_out, o[l])
        xn, r = ops.add_rmsnorm(y, r, wn, 1e-6)
        a = ops.gemm_packed(xn, gu[l], silu_mul=True)
        ops.gemm_packed(a, dn[l])

    def splitk(l):
        xn, r = ops.add_rmsnorm_splitk(parts0, res_, wn, 1e-6)
        ops.gemm_packed(xn, qkv[l])
        p = ops.gemm_packed_splitk(attn_out, o[l], 4)
        xn, r = ops.add_rmsnorm_splitk(p, r, wn, 1e-6)
        a = ops.gemm_packed(xn, gu[l], silu_mul=True)
        ops.gemm_packed_splitk(a, dn[l], 4)

    byt = ((hq + 2 * hkv) * 128 * H + H * hq * 128 + 2 * inter * H + H * inter) * 2
    out = {}
    for name, fn in (("complete rows + add_rmsnorm", rows), ("split-K 4 + add_rmsnorm_splitk", splitk)):
        t = min(timeit(fn, L, reps=3) for _ in range(3))
        out[name] = {"us": t * 1e6, "MB": byt / 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
    t = min(timeit(lambda l: ops.add_rmsnorm(x, res_, wn, 1e-6), 1, reps=28) for _ in range(3))
    out["add_rmsnorm 32 x 5120 alone"] = {"us": t * 1e6}
    t = min(timeit(lambda l: ops.add_rmsnorm_splitk(parts0, res_, wn, 1e-6), 1, reps=28) for _ in range(3))
    out["add_rmsnorm_splitk 4 x 32 x 5120 alone"] = {"us": t * 1e6}
    print(json.dumps({"Qwen3-32B on one GPU, 6 launches per layer": out}, indent=1))


def gemms_32b_shard():
    """Each projection of a Qwen3-32B TP 8 rank (and of the unsharded 32B layer) alone, bs 32: packed / split-K /
    complete-row variants, 4 rotating weight copies."""
    B, L = 32, 4
    res = {}
    shapes = {"qkv tp8 1280x5120": (1280, 5120, False), "o tp8 5120x1024": (5120, 1024, False),
              "gate_up tp8 6400x5120": (6400, 5120, True), "down tp8 5120x3200": (5120, 3200, False),
              "qkv tp1 10240x5120": (10240, 5120, False), "o tp1 5120x8192": (5120, 8192, False),
              "gate_up tp1 51200x5120": (51200, 5120, True), "down tp1 5120x25600": (5120, 25600, False)}
    for name, (N, K, silu) in shapes.items():
        ws = [(torch.randn(N, K, device=DEV) * 0.02).bfloat16() for _ in range(L)]
        wp = [ops.pack_weight(w) for w in ws]
        x = torch.randn(B, K, device=DEV).bfloat16()
        byt = N * K * 2
        r = {}
        t = timeit(lambda l: ops.gemm_packed(x, wp[l], silu_mul=silu), L, reps=4)
        r["packed_us"] = t * 1e6
        r["packed_frac"] = byt / t / PEAK
        if not silu:
            for ks in (2, 4, 8):
                if K % (ks * 256) == 0:
                    t = timeit(lambda l: ops.gemm_packed_splitk(x, wp[l], ks), L, reps=4)
                    r[f"splitk{ks}_us"] = t * 1e6
            w4 = [ops.pack_weight_rows4(w) for w in ws]
            t = timeit(lambda l: ops.gemm_rows4(x, w4[l]), L, reps=4)
            r["rows4_us"] = t * 1e6
        res[name] = r
        del ws, wp
    print(json.dumps(res, indent=1))


def main():
    if os.environ.get("KBENCH_ONLY") == "32b_gemms":
        return gemms_32b_shard()
    if os.environ.get("KBENCH_ONLY") == "moe":
        return moe_block()
    if os.environ.get("KBENCH_ONLY") == "32b":
        return chain_32b_shard()
    if os.environ.get("KBENCH_ONLY") == "32b_tp1":
        return chain_32b_one_gpu()
    if os.environ.get("KBENCH_ONLY") == "plain":
        return plain_attention()
    if os.environ.get("KBENCH_ONLY") == "prefill_order":
        return prefill_attention_order()
    if os.environ.get("KBENCH_ONLY") == "prefill":
        return prefill_attention()
    if os.environ.get("KBENCH_ONLY") == "fp8kv_prefill":
        return fp8_kv_prefill()
    if os.environ.get("KBENCH_ONLY") == "fp8kv":
        fp8_kv_attention()
        return fp8_kv_prefill()
    if os.environ.get("KBENCH_ONLY") == "head":
        return head_and_sampler()
    B, ctx, bs, hq, hkv, L = 32, int(os.environ.get("CTX", 1024)), 16, 16, 8, 28
    res = {}
    nb_seq = (ctx + bs - 1) // bs
    nblk = B * max(nb_seq, (1170 + bs - 1) // bs)  # every table below draws DISTINCT blocks (no cache-assisted re-reads)
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = [torch.randn(ops.kv_cache_shape(nblk, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    vc = [torch.randn(ops.kv_cache_shape(nblk, hkv, bs), device=DEV).bfloat16() for _ in range(L)]
    perm = torch.randperm(nblk, generator=g)[: B * nb_seq].to(torch.int32).view(B, nb_seq).to(DEV)
    ctxl = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    q = torch.randn(B, hq * 128, device=DEV).bfloat16()
    out = torch.empty(B, hq * 128, dtype=torch.bfloat16, device=DEV)
    ws = ops.attn_workspace(DEV, B, hq)
    t = timeit(lambda l: ops.paged_attn_decode(q, kc[l], vc[l], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
    byt = B * 2 * ctx * hkv * 128 * 2
    res["paged_attn_decode(+merge)"] = {"us": t * 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
    # the same layer's cache every launch: 134 MB of K/V stay in the 256 MiB Infinity Cache
    t = timeit(lambda l: ops.paged_attn_decode(q, kc[0], vc[0], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), 1)
    res["paged_attn_decode L3-resident"] = {"us": t * 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
    for c2 in (1040, 1100, 1170):  # ragged / growing contexts as in the timed bench window
        ctx2 = torch.full((B,), c2, dtype=torch.int32, device=DEV)
        nb2 = (c2 + bs - 1) // bs
        perm2 = torch.randperm(nblk, generator=g)[: B * nb2].to(torch.int32).view(B, nb2).to(DEV)
        t = timeit(lambda l: ops.paged_attn_decode(q, kc[l], vc[l], perm2, ctx2, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
        byt2 = B * 2 * c2 * hkv * 128 * 2
        res[f"paged_attn_decode ctx={c2}"] = {"us": t * 1e6, "GB/s": byt2 / t / 1e9, "frac": byt2 / t / PEAK}

    # geometry A/B (tuning knob; a captured graph keeps its choice) and the fused step
    _C.set_tuning(_C.TUNE_ATTN_PIPE, 0)
    t = timeit(lambda l: ops.paged_attn_decode(q, kc[l], vc[l], perm, ctxl, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
    res["paged_attn_decode 16 waves (r01)"] = {"us": t * 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
    _C.set_tuning(_C.TUNE_ATTN_PIPE, 1)
    qkv_ = torch.randn(B, (hq + 2 * hkv) * 128, device=DEV).bfloat16()
    w128 = torch.ones(128, device=DEV).bfloat16()
    rope_t = torch.randn(4096, 128, device=DEV)
    for c2 in (ctx, 1100):
        ctx2 = torch.full((B,), c2, dtype=torch.int32, device=DEV)
        nb2 = (c2 + bs - 1) // bs
        perm2 = torch.randperm(nblk, generator=g)[: B * nb2].to(torch.int32).view(B, nb2).to(DEV)
        pos2 = torch.full((B,), c2 - 1, dtype=torch.int64, device=DEV)
        sl2 = torch.stack([perm2[:, (c2 - 1) // bs], torch.full((B,), (c2 - 1) % bs, dtype=torch.int32, device=DEV)], 1).contiguous()
        byt2 = B * 2 * c2 * hkv * 128 * 2
        qo_ = torch.empty(B, hq * 128, dtype=torch.bfloat16, device=DEV)
        t = timeit(lambda l: (ops.qknorm_rope_store(qkv_, w128, w128, 1e-6, pos2, rope_t, kc[l], vc[l], sl2, hq, hkv, bs, q_out=qo_),
                              ops.paged_attn_decode(qo_, kc[l], vc[l], perm2, ctx2, hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws)), L)
        res[f"rope_store + attn ctx={c2}"] = {"us": t * 1e6, "GB/s": byt2 / t / 1e9, "frac": byt2 / t / PEAK}
        t = timeit(lambda l: ops.paged_attn_decode_fused(qkv_, w128, w128, 1e-6, pos2, rope_t, sl2, kc[l], vc[l], perm2, ctx2,
                                                         hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
        res[f"attn fused step ctx={c2}"] = {"us": t * 1e6, "GB/s": byt2 / t / 1e9, "frac": byt2 / t / PEAK}

    # block ids read through the scalar cache per chunk (default) vs a wave's run resolved once, interleaved rounds
    c2 = 1100
    ctx2 = torch.full((B,), c2, dtype=torch.int32, device=DEV)
    nb2 = (c2 + bs - 1) // bs
    perm2 = torch.randperm(nblk, generator=g)[: B * nb2].to(torch.int32).view(B, nb2).to(DEV)
    pos2 = torch.full((B,), c2 - 1, dtype=torch.int64, device=DEV)
    sl2 = torch.stack([perm2[:, (c2 - 1) // bs], torch.full((B,), (c2 - 1) % bs, dtype=torch.int32, device=DEV)], 1).contiguous()
    byt2 = B * 2 * c2 * hkv * 128 * 2
    for rnd in range(3):
        for mode in ("0", "1"):
            _C.set_tuning(_C.TUNE_ATTN_RESOLVE, int(mode))
            t = timeit(lambda l: ops.paged_attn_decode_fused(qkv_, w128, w128, 1e-6, pos2, rope_t, sl2, kc[l], vc[l], perm2, ctx2,
                                                             hq, hkv, bs, 128 ** -0.5, out=out, workspace=ws), L)
            res[f"fused step ctx=1100 {'run resolved   ' if mode == '1' else 'table per chunk'} #{rnd}"] = {
                "us": t * 1e6, "GB/s": byt2 / t / 1e9, "frac": byt2 / t / PEAK}
    _C.set_tuning(_C.TUNE_ATTN_RESOLVE, 0)

    if os.environ.get("KBENCH_ONLY") == "attn":
        for k, v in res.items():
            print(f"{k:32s} " + "  ".join(f"{a}={b:9.2f}" for a, b in v.items()))
        return

    def gemm(name, N, K, M=32):
        ws_ = [(torch.randn(N, K, device=DEV) * 0.02).bfloat16() for _ in range(L if N < 100000 else 3)]
        x = torch.randn(M, K, device=DEV).bfloat16()
        y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        n = len(ws_)
        t = timeit(lambda l: ops.gemm_skinny(x, ws_[l], out=y), n)
        byt = N * K * 2
        res[name] = {"us": t * 1e6, "GB/s": byt / t / 1e9, "frac": byt / t / PEAK}
        # torch (hipBLASLt) comparison column
        t2 = timeit(lambda l: torch.nn.functional.linear(x, ws_[l]), n)
        res[name]["torch_us"] = t2 * 1e6
        wp_ = [ops.pack_weight(w_) for w_ in ws_]
        t3 = timeit(lambda l: ops.gemm_packed(x, wp_[l], out=y), n)
        res[name]["packed_us"] = t3 * 1e6
        if N <= 2048:  # row-parallel projections: split-K over workgroups + fused consumer
            r = torch.randn(M, N, device=DEV).bfloat16()
            nw = torch.ones(N, device=DEV).bfloat16()
            for ks in (2, 4, 8):
                if K % (32 * ks * 4):
                    continue
                parts = torch.empty(ks, M, N, dtype=torch.float32, device=DEV)
                t4 = timeit(lambda l: ops.gemm_packed_splitk(x, wp_[l], ks, out=parts), n)
                res[name][f"splitk{ks}_us"] = t4 * 1e6
            t5 = timeit(lambda l: (ops.gemm_packed_splitk(x, wp_[l], 4, out=parts[:4] if parts.shape[0] >= 4 else parts),
                                   ops.add_rmsnorm_splitk(parts[:4], r, nw, 1e-6, out=r, residual_out=r)), n)
            res[name]["splitk4+addnorm_us"] = t5 * 1e6
            t6 = timeit(lambda l: (ops.gemm_packed(x, wp_[l], out=y), ops.add_rmsnorm(y, r, nw, 1e-6, out=y, residual_out=r)), n)
            res[name]["packed+addnorm_us"] = t6 * 1e6
        if N <= 2048:  # complete rows from N/4 workgroups, and the pair (projection, consumer GEMM with norm prologue)
            w4_ = [ops.pack_weight_rows4(w_) for w_ in ws_]
            yr = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            t9 = timeit(lambda l: ops.gemm_rows4(x, w4_[l], out=yr), n)
            res[name]["rows4_us"] = t9 * 1e6
        if N == 6144:
            so_ = torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV)
            t7 = timeit(lambda l: ops.gemm_packed(x, wp_[l], out=so_, silu_mul=True), n)
            res[name]["packed_silu_fused_us"] = t7 * 1e6
            t8 = timeit(lambda l: (ops.gemm_packed(x, wp_[l], out=y), ops.silu_mul(y, out=so_)), n)
            res[name]["packed+silu_us"] = t8 * 1e6

    gemm("qkv 4096x1024", 4096, 1024)
    gemm("o 1024x2048", 1024, 2048)
    gemm("gate_up 6144x1024", 6144, 1024)
    gemm("down 1024x3072", 1024, 3072)
    gemm("lm_head 151936x1024", 151936, 1024)

    x = torch.randn(B, 1024, device=DEV).bfloat16()
    r = torch.randn(B, 1024, device=DEV).bfloat16()
    w = torch.ones(1024, device=DEV).bfloat16()
    t = timeit(lambda l: ops.add_rmsnorm(x, r, w, 1e-6, out=x, residual_out=r), 1, iters=20, reps=50)
    res["add_rmsnorm 32x1024"] = {"us": t * 1e6}
    gu = torch.randn(B, 6144, device=DEV).bfloat16()
    so = torch.empty(B, 3072, dtype=torch.bfloat16, device=DEV)
    t = timeit(lambda l: ops.silu_mul(gu, out=so), 1, iters=20, reps=50)
    res["silu_mul 32x6144"] = {"us": t * 1e6}
    qkv = torch.randn(B, 4096, device=DEV).bfloat16()
    pos = torch.full((B,), ctx - 1, dtype=torch.int64, device=DEV)
    table = torch.randn(4096, 128, device=DEV)
    slots = torch.stack([perm[:, -1], torch.full((B,), (ctx - 1) % bs, dtype=torch.int32, device=DEV)], 1).contiguous()
    qo = torch.empty(B, 2048, dtype=torch.bfloat16, device=DEV)
    t = timeit(lambda l: ops.qknorm_rope_store(qkv, w[:128], w[:128], 1e-6, pos, table, kc[l], vc[l], slots, hq, hkv, bs, q_out=qo), L)
    res["qknorm_rope_store"] = {"us": t * 1e6}
    logits = torch.randn(B, 151936, device=DEV).bfloat16()
    t = timeit(lambda l: ops.argmax(logits), 1, iters=20, reps=10)
    res["argmax 32x151936"] = {"us": t * 1e6}
    # empty-launch floor through ctypes (host-bound)
    t0 = time.perf_counter()
    for _ in range(2000):
        ops.silu_mul(gu, out=so)
    torch.cuda.synchronize()
    res["host launch via ctypes"] = {"us": (time.perf_counter() - t0) / 2000 * 1e6}
    for k, v in res.items():
        print(f"{k:32s} " + "  ".join(f"{a}={b:9.2f}" if isinstance(b, float) else f"{a}={b}" for a, b in v.items()))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/kbench.json", "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
