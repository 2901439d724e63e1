"""The fp8-KV decode kernel (csrc/paged_attn_fp8kv.hip) past three chunks per wave: the double-buffered steady-state loop
of paged_attn_decode_fp8kv_kernel, its two exits, a patch of the step's token inside and behind that loop, the group
size 4 and block size 48 instantiations - and the quantisation rule at its edges through all three stores.

The kernel deals 32-key chunks to 8 * splits waves; only a wave with four or more chunks enters the loop.  work_split()
restates that deal on the host, test_the_cases_reach_the_steady_state_loop holds the contexts below to it (so that a
change of the deal fails there instead of quietly un-covering the loop), and every GPU test pads its batch with empty
rows (context 0, as hipGraph padding) until the launch has the number of splits its contexts were chosen for."""
import functools
import math

import pytest
import torch

from test_kv_fp8_gpu import D, LENS, fp8_caches, kv_rule, rows

EPS = 1e-6
# splits == 1: (k, single-tile last chunk) for k = 3 .. 8 and (k + 1, full) ...
UNSPLIT = [769, 1025, 1281, 1537, 1793, 2049]
# ... and the same runs with the step's token in the other tile of its chunk
UNSPLIT = UNSPLIT + [n + 16 for n in UNSPLIT[1:]]
TWO_WAY = [1537, 1553, 2049, 2065]  # splits == 2: 4 and 5 chunks through the fp32 partials and the merge kernel
SETS = {"unsplit": (UNSPLIT, 1), "two_way": (TWO_WAY, 2)}
Q_MILD = -6  # the second draw of test 3: q * 2^Q_MILD (see reference())
V_SEED = 70  # seeds of test 3's V rows (with 40, test_kv_fp8_gpu.py's, one all-small tile of 16 rows leaves a margin of 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the work split on the host
# ---------------------------------------------------------------------------------------------------------------------
def decode_splits(batch, hkv):
    """decode_splits8 of csrc/paged_attn_fp8kv.hip"""
    return min(max(4096 // max(batch * hkv * 16, 1), 1), 16)


def work_split(batch, hkv, ctx):
    """The kernel's deal for one (sequence, kv head): (splits, [(chunks, last chunk is a single tile)] per wave,
    (chunks of the wave, buffer, tile of its chunk) of the tile that holds token ctx - 1).  The buffers alternate
    A, B, A, ... along a wave's run on every path of the kernel."""
    splits = decode_splits(batch, hkv)
    n_tiles = (ctx + 15) >> 4
    dq, dr = divmod((n_tiles + 1) >> 1, 8 * splits)
    deal = lambda r: r * dq + min(r, dr)  # noqa: E731
    waves, new, new_tile = [], None, (ctx - 1) >> 4
    for vw in range(8 * splits):
        c0, c1 = deal(vw), deal(vw + 1)
        t1 = min(n_tiles, 2 * c1)
        waves.append((c1 - c0, c1 > c0 and 2 * (c1 - 1) + 1 >= t1))
        if ctx > 0 and c0 <= new_tile >> 1 < c1:
            new = (c1 - c0, "AB"[((new_tile >> 1) - c0) & 1], new_tile & 1)
    return splits, waves, new


def padded_batch(n_rows, hkv, splits):
    """The smallest batch >= n_rows whose launch has `splits` splits; the rows behind n_rows are empty."""
    batch = max(n_rows, 128 // hkv + 1 if splits == 1 else -(-86 // hkv))
    assert decode_splits(batch, hkv) == splits, (batch, hkv, splits)
    return batch


def test_the_cases_reach_the_steady_state_loop():
    for hkv in (1, 2, 4, 8):
        for n_rows in (len(UNSPLIT), 2 * len(UNSPLIT)):
            runs, placed = set(), set()
            for ctx in UNSPLIT:
                splits, waves, new = work_split(padded_batch(n_rows, hkv, 1), hkv, ctx)
                assert splits == 1
                runs |= set(waves)
                placed.add(new)
            assert {(k, s) for k in range(3, 9) for s in (False, True)} <= runs, sorted(runs)
            # the step's token in buffer A and in buffer B, as first and as second tile, on waves that ran the loop
            assert {(b, t) for k, b, t in placed if k >= 4} == {(b, t) for b in "AB" for t in (0, 1)}, sorted(placed)
        for n_rows in (len(TWO_WAY), 2 * len(TWO_WAY)):
            runs, placed = set(), set()
            for ctx in TWO_WAY:
                splits, waves, new = work_split(padded_batch(n_rows, hkv, 2), hkv, ctx)
                assert splits == 2 and len(waves) == 16
                runs |= set(waves)
                placed.add(new)
            assert {(4, False), (4, True), (5, False)} <= runs, sorted(runs)
            assert any(k >= 4 for k, _, _ in placed), sorted(placed)
    # the gap this file closes: what test_kv_fp8_gpu.py and test_kv_fp8_fused_gpu.py launch never enters the loop
    runs, placed = set(), set()
    for lens in (LENS, LENS * 3, [700]):
        for hkv in (1, 2, 8):
            for batch in (len(lens), len(lens) + 1):  # the fused test adds one padding row
                for ctx in lens:
                    _, waves, new = work_split(batch, hkv, ctx)
                    runs |= set(waves)
                    placed.add(new)
    assert {k for k, _ in runs} == {0, 1, 2, 3} and all(k <= 1 for k, single in runs if single), sorted(runs)
    assert placed == {(1, "A", 0), (1, "A", 1), (2, "B", 1)}, sorted(placed)


# ---------------------------------------------------------------------------------------------------------------------
# shared: paging
# ---------------------------------------------------------------------------------------------------------------------
def paging(lens, bs, n_rows):
    """Permuted block tables [n_rows, .] (rows behind len(lens) hold -1), the flat slot of every position of every
    sequence, and what the identity-table twin needs."""
    nb = [-(-n // bs) for n in lens]
    nblk = sum(nb) + 3
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(5)).int()
    tables = torch.full((n_rows, max(nb)), -1, dtype=torch.int32)
    flat, used = [], 0
    for i, n in enumerate(lens):
        tables[i, : nb[i]] = perm[used: used + nb[i]]
        used += nb[i]
        pos = torch.arange(n)
        flat.append((tables[i][pos // bs] * bs + pos % bs).int())
    return tables, flat, nblk, perm[:used].long()


def identity_twin(tables, order):
    """Tables over cache[order]: the same sequences at blocks 0, 1, 2, ..."""
    ident = torch.full_like(tables, -1)
    ident[tables >= 0] = torch.arange(len(order), dtype=torch.int32)
    return ident


# ---------------------------------------------------------------------------------------------------------------------
# 2. every key counted exactly once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block_size", [16, 48, 256])
@pytest.mark.parametrize("hq,hkv", [(16, 4), (8, 8)])
@pytest.mark.parametrize("which", list(SETS))
def test_every_key_is_counted_exactly_once(which, hq, hkv, block_size):
    """q = 0: every score is 0 and every visible key weighs 1 / ctx.  V of token t is one-hot 1.0 (exact in e4m3) at
    dim (t / 16) % 128, so out[d] = (number of context tokens whose tile maps to d) / ctx: sums of ones are exact, the
    unsplit path divides them correctly rounded, the merge path multiplies by a rounded reciprocal - one bf16 ulp
    covers both.  A token dropped, attended twice or masked wrongly moves an element by 1/16 of itself or more."""
    from nanovllm import ops

    lens, splits = SETS[which]
    bs, n_seq = block_size, len(lens)
    batch = padded_batch(n_seq, hkv, splits)
    tables, flat, nblk, order = paging(lens, bs, batch)
    cache = fp8_caches(nblk, hkv, bs)
    want = torch.zeros(batch, D, dtype=torch.float64)
    for i, n in enumerate(lens):
        v = torch.zeros(n, hkv, D, dtype=torch.bfloat16)
        v[torch.arange(n), :, (torch.arange(n) // 16) % D] = 1.0
        ops.kv_store_fp8(rows(n, hkv, 10 + i).cuda(), v.cuda(), cache[0], cache[1], flat[i].cuda(), hkv, bs)
        want[i] = torch.bincount((torch.arange(n) // 16) % D, minlength=D).double() / n
    ctx = torch.tensor(lens + [0] * (batch - n_seq), dtype=torch.int32).cuda()
    q = torch.zeros(batch, hq * D, dtype=torch.bfloat16, device="cuda")
    out = ops.paged_attn_decode_fp8kv(q, cache[0], cache[1], tables.cuda(), ctx, hq, hkv, bs, D ** -0.5)
    got = out.double().cpu().view(batch, hq, D)
    ulp = torch.where(want > 0, torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 8), torch.zeros_like(want))
    off = ((got - want[:, None]).abs() / ulp[:, None].clamp(min=2.0 ** -140)).max().item()
    print(f"worst |out - count / ctx| = {off:.3f} bf16 ulp (allowed 1)")
    assert ((got - want[:, None]).abs() <= ulp[:, None]).all()
    assert (got[n_seq:] == 0).all()  # the padding rows
    out2 = ops.paged_attn_decode_fp8kv(q, cache[0][order.cuda()].contiguous(), cache[1][order.cuda()].contiguous(),
                                       identity_twin(tables, order).cuda(), ctx, hq, hkv, bs, D ** -0.5)
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fp64 attention over the dequantised rows
# ---------------------------------------------------------------------------------------------------------------------
def fp64_attention(q, kd, vd, g):
    """q [hq, D], kd / vd [n, hkv, D] fp64 -> (out [hq, D], p [hq, n])"""
    p = torch.softmax(torch.einsum("hd,nhd->hn", q.double(), kd.repeat_interleave(g, 1)) * D ** -0.5, -1)
    return torch.einsum("hn,nhd->hd", p, vd.repeat_interleave(g, 1)), p


def tile_margin(out, p, vd, g):
    """For every query head: min over the 16-key tiles of max over the output elements of
    |out without the tile - out| / (4 * allowed(out)), allowed = 1e-4 + 2^-8 |out|.  From the fp64 probabilities alone:
    without tile T the output is (out - S_T) / (1 - P_T), S_T = sum_T p v, P_T = sum_T p."""
    hq, n = p.shape
    n_tiles = -(-n // 16)
    pp = torch.zeros(hq, n_tiles * 16, dtype=torch.float64)
    pp[:, :n] = p
    vv = torch.zeros(n_tiles * 16, hq, D, dtype=torch.float64)
    vv[:n] = vd.repeat_interleave(g, 1)
    s_t = torch.einsum("htk,tkhd->htd", pp.view(hq, n_tiles, 16), vv.view(n_tiles, 16, hq, D))
    p_t = pp.view(hq, n_tiles, 16).sum(-1)[..., None]
    moved = ((out[:, None] - s_t) / (1 - p_t) - out[:, None]).abs()
    return (moved / (4 * (1e-4 + 2.0 ** -8 * out.abs()))[:, None]).amax(-1).amin(-1)  # [hq]


@functools.lru_cache(maxsize=None)
def reference(which, hq, hkv):
    """Per sequence (k, v) and, for both draws of q, fp64 attention over the dequantised rows; the margins of the
    milder draw.  q of the first draw is `rows` itself (many heads nearly one-hot: the largest scores, the rescaling
    path), the second is the same q times 2^Q_MILD, which spreads every head's weight over its whole context."""
    lens, g = SETS[which][0], hq // hkv
    q = rows(len(lens), hq, 6)
    q_mild = (q.float() * 2.0 ** Q_MILD).to(torch.bfloat16)  # (exact)
    kv, want, want_mild, margin = [], [], [], []
    for i, n in enumerate(lens):
        k, v = rows(n, hkv, 10 + i), rows(n, hkv, V_SEED + i)
        # the final tile holds ONE token at these contexts: no spread of the weight lets an ordinary row there move
        # the output by more than the bound, so its V row gets the largest magnitude of `rows`
        tail = 16 * ((n - 1) // 16)
        v[tail:] = (torch.randn(n - tail, hkv, D, generator=torch.Generator().manual_seed(1000 + i)) * 8).to(v.dtype)
        kd, vd = kv_rule(k)[2].double(), kv_rule(v)[2].double()
        kv.append((k, v))
        want.append(fp64_attention(q[i], kd, vd, g)[0])
        o, p = fp64_attention(q_mild[i], kd, vd, g)
        want_mild.append(o)
        margin.append(tile_margin(o, p, vd, g).view(hkv, g).amax(-1))  # the best query head of every kv head
    return kv, torch.cat([q, q_mild]), torch.stack(want + want_mild).view(2 * len(lens), hq * D), torch.stack(margin)


GEOMETRIES = [(4, 4), (16, 8), (16, 4), (16, 2), (16, 1)]  # G = 1, 2, 4, 8, 16


@pytest.mark.parametrize("hq,hkv", GEOMETRIES)
@pytest.mark.parametrize("which", list(SETS))
def test_the_milder_draw_would_show_any_mis_attended_tile(which, hq, hkv):
    """The condition that makes test_long_decode_matches_fp64... sensitive, from the reference alone: for every
    sequence and kv head there is a query head for which leaving ANY single 16-key tile out of the attention moves some
    output element by more than 4 times what the bound allows that element.  With q * 2^-6 the smallest margin over all
    cases is 1.90 (times the 4), between 1.8 and 2.6 from q * 2^-5 to q * 2^-8; with q itself it is 0 (heads that see
    one key only)."""
    margin = reference(which, hq, hkv)[3]
    print(f"smallest margin {margin.min().item():.2f} (needed > 1)")
    assert margin.min().item() > 1


@pytest.mark.gpu
@pytest.mark.parametrize("block_size", [16, 48, 256])
@pytest.mark.parametrize("hq,hkv", GEOMETRIES)
@pytest.mark.parametrize("which", list(SETS))
def test_long_decode_matches_fp64_over_the_dequantised_cache(which, hq, hkv, block_size):
    """test_kv_fp8_gpu.py's decode test at the contexts that run the loop, its bound unchanged (an fp32 model of the
    kernel's arithmetic stays below 1e-6 of it at these contexts: the bound does not grow with the context).  Every
    sequence is attended twice in the one launch, with q and with the milder q, through the same blocks."""
    from nanovllm import ops

    lens, splits = SETS[which]
    bs, n_seq, scale = block_size, len(lens), D ** -0.5
    kv, q, want, _ = reference(which, hq, hkv)
    batch = padded_batch(2 * n_seq, hkv, splits)
    tables, flat, nblk, order = paging(lens, bs, batch)
    tables[n_seq: 2 * n_seq] = tables[:n_seq]
    cache = fp8_caches(nblk, hkv, bs)
    ops.kv_store_fp8(torch.cat([k for k, _ in kv]).cuda(), torch.cat([v for _, v in kv]).cuda(), cache[0], cache[1],
                     torch.cat(flat).cuda(), hkv, bs)
    ctx = torch.tensor(lens * 2 + [0] * (batch - 2 * n_seq), dtype=torch.int32).cuda()
    q_all = torch.zeros(batch, hq * D, dtype=torch.bfloat16)
    q_all[: 2 * n_seq] = q.view(2 * n_seq, -1)
    out = ops.paged_attn_decode_fp8kv(q_all.cuda(), cache[0], cache[1], tables.cuda(), ctx, hq, hkv, bs, scale)
    got = out.double().cpu()
    err = (got[: 2 * n_seq] - want).abs() - 2.0 ** -8 * got[: 2 * n_seq].abs()
    print(f"worst |out - ref| - 2^-8 |out| = {err[:n_seq].max().item():.3e}, milder q {err[n_seq:].max().item():.3e} "
          f"(allowed 1e-4)")
    assert err.max().item() <= 1e-4
    assert (got[2 * n_seq:] == 0).all()  # the padding rows
    # paging invariance: an identity table over a permuted copy of the cache gives the same bits
    ident = identity_twin(tables[:n_seq], order)
    ident = torch.cat([ident, ident, torch.full_like(tables[2 * n_seq:], -1)])
    out2 = ops.paged_attn_decode_fp8kv(q_all.cuda(), cache[0][order.cuda()].contiguous(),
                                       cache[1][order.cuda()].contiguous(), ident.cuda(), ctx, hq, hkv, bs, scale)
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the fused step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block_size", [16, 48])
@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "norm"])
@pytest.mark.parametrize("hq,hkv", [(16, 4), (16, 1)])
@pytest.mark.parametrize("which", list(SETS))
def test_long_fused_step_equals_its_launch_sequence_and_fp64_attention(which, hq, hkv, norm, block_size):
    """test_kv_fp8_fused_gpu.py's test where the step's token is patched into a buffer inside or behind the loop."""
    from nanovllm import ops

    lens, splits = SETS[which]
    g, scale, n_seq, bs = hq // hkv, D ** -0.5, len(lens), block_size
    batch = padded_batch(n_seq, hkv, splits)  # the rows behind n_seq are graph padding: no context, slot (-1, -1)
    ctx = torch.tensor(lens + [0] * (batch - n_seq), dtype=torch.int32)
    tables, flat, nblk, _ = paging(lens, bs, batch)
    cache = fp8_caches(nblk, hkv, bs)
    for i, n in enumerate(lens):  # the context before this step
        ops.kv_store_fp8(rows(n - 1, hkv, 10 + i).cuda(), rows(n - 1, hkv, 40 + i).cuda(), cache[0], cache[1],
                         flat[i][:-1].cuda(), hkv, bs)
    last = torch.stack([f[-1] for f in flat])
    slots = torch.full((batch, 2), -1, dtype=torch.int32)
    slots[:n_seq] = torch.stack([last // bs, last % bs], 1)
    slots = slots.cuda()
    qkv = rows(batch, hq + 2 * hkv, 6)
    qkv[:n_seq, :hq] = (qkv[:n_seq, :hq].float() * 2.0 ** Q_MILD).to(torch.bfloat16)
    qkv = qkv.view(batch, -1).cuda()
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
    assert torch.equal(cache, want_cache)  # data and scales; nothing else moved (the padding rows stored nothing)
    assert (out[n_seq:] == 0).all()

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
    for i, n in enumerate(lens):
        ref.append(fp64_attention(q[i].view(hq, D).cpu(), deq[0][o: o + n], deq[1][o: o + n], g)[0].reshape(-1))
        o += n
    got = out[:n_seq].double().cpu()
    err = (got - torch.stack(ref)).abs() - 2.0 ** -8 * got.abs()
    print(f"worst |out - ref| - 2^-8 |out| = {err.max().item():.3e} (allowed 1e-4)")
    assert err.max().item() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 5. the quantisation rule at its edges
# ---------------------------------------------------------------------------------------------------------------------
def e4m3_byte(x):
    """RNE_e4m3fn of a double by integers: sign, 4 exponent bits (bias 7), 3 mantissa bits; subnormals are multiples of
    2^-9 below 2^-6.  (Python's round() of an exactly representable quotient is round-half-to-even.)"""
    sign = 0x80 if math.copysign(1.0, x) < 0 else 0
    a = abs(x)
    if a == 0:
        return sign
    e = max(math.frexp(a)[1] - 1, -6)  # floor(log2 a), the subnormals share the smallest normal exponent
    n = round(math.ldexp(a, 3 - e))    # units of 2^(e - 3): 8 .. 16 for normals, 0 .. 8 for subnormals
    if n == 16:
        n, e = 8, e + 1
    assert e <= 8, x  # the rule keeps every value below 448
    return sign | n if n < 8 else sign | (e + 7) << 3 | (n - 8)


def rule_by_integers(row):
    """include/mi355_nanovllm.h's rule for one row of doubles: (bytes, scale)"""
    amax = max(abs(x) for x in row)
    e = max(math.frexp(amax)[1] - 1 - 7, -120) if amax > 0 else 0
    return [e4m3_byte(math.ldexp(x, -e)) for x in row], math.ldexp(1.0, e)


@functools.lru_cache(maxsize=None)
def edge_rows():
    """bf16 rows [n, 128] whose e4m3 image is known by construction (scaled values s, row = s * 2^e), with their bytes
    and scales by rule_by_integers.  Inf and NaN are outside the rule and are left out."""
    u = 2.0 ** -9  # the e4m3 subnormal unit
    ties = [136, 152, 168, 184, 200, 216, 232, 248, 17, 19, 34, 38, 4.25, 4.75, 1.0625, 1.1875]  # halfway in their binade
    near = [135, 137, 151, 153, 247, 249, 16.5, 17.5, 33, 35, 1.03125, 1.09375]  # a quarter step off the ties
    sub = [u, 2 * u, 3 * u, 7 * u, 8 * u, 0.5 * u, 1.5 * u, 2.5 * u, 3.5 * u, 6.5 * u, 7.5 * u,  # values and ties
           0.25 * u, 0.125 * u, 0.4375 * u, 0.5625 * u, 1.25 * u, 1.75 * u, 7.25 * u, 7.75 * u, 8.5 * u, 9 * u]
    both = lambda xs: [s * x for x in xs for s in (1, -1)]  # noqa: E731
    spec = [(k, [128.0, -64.0] + both(ties[8:]) + both(near[6:])) for k in (-100, -9, 0, 3, 110)]  # amax = 2^(k + 7)
    spec += [(k, both(ties) + both(near) + both(sub)) for k in (-7, 20)]
    spec += [(k, [255.0, -255.0, 254, 253, 129, 127.5] + both(ties[:8])) for k in (-30, 0, 120)]  # 255 -> 256; 120: 0x7f7f
    spec += [(k, [192.0] + both(sub) + [0.0, -0.0]) for k in (-60, -7, 0, 40)]
    spec += [(0, [0.0, -0.0]), (0, [-0.0])]  # zero rows: scale 1, the sign survives
    spec += [(-113, [128.0, 1.5 * 128] + both(ties)),  # the last exponent above the clamp
             (-120, [2.0 ** -6, -(2.0 ** -6)] + both(sub[:12])),  # amax = 2^-126 under the clamp; bf16 subnormals behind it
             (-120, [96.0, 64, 100, -50, 25] + both(sub[:12])),   # amax = 1.5 * 2^-114: clamped
             (-133, both([float(i) for i in (1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 40, 56, 63, 64, 65, 100, 120, 127)]))]
    x = torch.tensor([[math.ldexp(vals[i % len(vals)], k) for i in range(D)] for k, vals in spec], dtype=torch.float64)
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.double(), x) and torch.isfinite(xb.float()).all()  # every value is a bf16 value
    assert torch.equal(torch.signbit(xb.float()), torch.signbit(x))
    want = [rule_by_integers(r) for r in x.tolist()]
    return (xb, torch.tensor([w[0] for w in want], dtype=torch.uint8), torch.tensor([w[1] for w in want], dtype=torch.float32))


def test_kv_rule_follows_the_header_at_the_edges():
    """kv_rule (torch's frexp, ldexp and float8 cast) against the integer description, so that the GPU tests below do not
    rest on torch's handling of ties, subnormals and signed zeros."""
    assert [e4m3_byte(x) for x in (0.0, -0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 240.0, 248.0, 256.0, -448.0, 2.0 ** -10,
                                   1.5 * 2.0 ** -10)] == [0, 0x80, 1, 8, 0x38, 0x77, 0x78, 0x78, 0xFE, 0, 1]
    every = torch.arange(256, dtype=torch.uint8)  # the encoder inverts the decoder on all finite codes
    vals = every.view(torch.float8_e4m3fn).double()
    assert [e4m3_byte(v) for v in vals.tolist() if not math.isnan(v)] == [b for b in range(256) if b & 0x7F != 0x7F]
    x, want_q, want_s = edge_rows()
    assert 0x80 in want_q and 0x78 in want_q and 0xF8 in want_q
    assert want_s.min().item() == 2.0 ** -120 and want_s.max().item() == 2.0 ** 120
    q, s, deq = kv_rule(x)
    assert torch.equal(s, want_s)
    assert torch.equal(q, want_q)
    # value * scale is exact - but for values of 248 * 2^120 and more, which round up to 256 * 2^120 = 2^128: the one
    # place where the dequantised row is not finite (bf16's largest value is 255 * 2^120)
    over = x.double().abs() >= 248 * 2.0 ** 120
    assert over.any() and torch.equal(torch.isinf(deq), over)
    assert torch.equal(deq.double()[~over], (q.view(torch.float8_e4m3fn).double() * s.double()[:, None])[~over])


def gathered(cache, is_v, slots, hkv, bs):
    from nanovllm import ops

    b8, s = ops.kv_cache_gather_fp8(cache[int(is_v)], is_v, slots.cuda(), hkv, bs)
    return b8.cpu().view(-1, hkv, D), s.cpu()


def first_difference(got, want):
    bad = (got != want).nonzero()
    return f"{len(bad)} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}"


@pytest.mark.gpu
@pytest.mark.parametrize("block_size", [16, 48])
def test_the_three_stores_follow_the_rule_at_its_edges(block_size):
    """The edge rows as K and V through kv_store_fp8, as V through the prefill-sized fused store and as V of the step's
    token through the fused decode step (neither transforms V): bytes and scales equal kv_rule's, exactly."""
    from nanovllm import ops

    x, _, _ = edge_rows()
    hq, hkv, bs, n = 4, 2, block_size, len(x)
    kv = torch.stack([x, x.flip(0)], 1)  # [n, hkv, D]: every row under both kv heads
    want_q, want_s, _ = kv_rule(kv)
    nblk = -(-n // bs) + 2
    slots = torch.randperm(nblk * bs, generator=torch.Generator().manual_seed(3))[:n].int()

    cache = fp8_caches(nblk, hkv, bs)
    ops.kv_store_fp8(kv.cuda(), kv.flip(1).contiguous().cuda(), cache[0], cache[1], slots.cuda(), hkv, bs)
    for is_v, (wq, ws) in ((False, (want_q, want_s)), (True, (want_q.flip(1), want_s.flip(1)))):
        b8, s = gathered(cache, is_v, slots, hkv, bs)
        assert torch.equal(s, ws), "kv_store_fp8 scales: " + first_difference(s, ws)
        assert torch.equal(b8, wq), "kv_store_fp8 bytes: " + first_difference(b8, wq)

    qkv = rows(n, hq + 2 * hkv, 9)
    qkv[:, hq + hkv:] = kv
    qkv = qkv.view(n, -1).cuda()
    ang = torch.rand(64, D // 2, generator=torch.Generator().manual_seed(7)) * 6.2832
    cos_sin = torch.cat([ang.cos(), ang.sin()], 1).cuda()
    cache = fp8_caches(nblk, hkv, bs)
    ops.qknorm_rope_store_fp8(qkv, None, EPS, torch.arange(n).cuda() % 64, cos_sin, cache[0], cache[1], slots.cuda(),
                              hq, hkv, bs)
    b8, s = gathered(cache, True, slots, hkv, bs)
    assert torch.equal(s, want_s), "qknorm_rope_store_fp8 scales: " + first_difference(s, want_s)
    assert torch.equal(b8, want_q), "qknorm_rope_store_fp8 bytes: " + first_difference(b8, want_q)

    # the fused decode step: sequence i has i % 40 + 1 tokens (an all-zero context in front of the step's token)
    lens = [i % 40 + 1 for i in range(n)]
    tables, flat, nblk, _ = paging(lens, bs, n)
    last = torch.stack([f[-1] for f in flat])
    cache = fp8_caches(nblk, hkv, bs)
    ctx = torch.tensor(lens, dtype=torch.int32)
    ops.paged_attn_decode_fp8kv_fused(qkv, None, None, EPS, (ctx.long() - 1).cuda(), cos_sin,
                                      torch.stack([last // bs, last % bs], 1).int().cuda(), cache[0], cache[1],
                                      tables.cuda(), ctx.cuda(), hq, hkv, bs, D ** -0.5)
    b8, s = gathered(cache, True, last, hkv, bs)
    assert torch.equal(s, want_s), "fused decode step scales: " + first_difference(s, want_s)
    assert torch.equal(b8, want_q), "fused decode step bytes: " + first_difference(b8, want_q)
