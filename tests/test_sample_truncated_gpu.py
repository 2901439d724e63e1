"""Top-k / top-p sampling: mi_sample_truncated against the fp64 definition of its kept set, and the engine paths to it."""
import types

import pytest
import torch

from model_configs import MID, make_model_dir
from nanovllm import LLM, SamplingParams, ops
from nanovllm.engine.llm_engine import LLMEngine

# (top_k, top_p, temperature) of the six rows of every kernel case; "V" stands for the vocabulary size
ROWS = ((0, 1.0, 1.0), (50, 1.0, 0.7), (0, 0.9, 1.0), (20, 0.8, 0.6), ("V", 1.0, 1.3), (5, 1.0, 0.0))
# generator seeds for which every top-p threshold clears the margin asserted in kept_set (checked when written)
CASES = {(1003, "randn"): 5, (1003, "grid"): 1, (4096, "randn"): 7, (4096, "grid"): 1, (151936, "randn"): 92,
         (151936, "grid"): 1, (155661, "randn"): 13, (155661, "grid"): 1}


def make_logits(vocab, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return (torch.randn(len(ROWS), vocab, generator=gen) * 3).bfloat16()
    # ~40 distinct values, heavy ties: negatives, both zeros, neighbours in the low byte of one high byte (1.0 = 0x3F80,
    # 0x3F81, 0x3F82; 2.0 = 0x4000, 0x4001; -1.0 = 0xBF80, 0xBF81), and a few -inf; high values are rarer
    grid = torch.tensor([-8.0, -6.0, -4.5, -3.0, -2.0, -1.0078125, -1.0, -0.5, -0.25, -0.0, 0.0, 0.125, 0.25, 0.5, 0.75,
                         1.0, 1.0078125, 1.015625, 1.5, 1.75, 2.0, 2.015625, 2.5, 3.0, 3.5, 4.0, 4.03125, 4.5, 5.0, 5.5,
                         6.0, 6.5, 7.0, 7.0625, 7.5, 8.0, 8.0625, 8.5, 9.0, 9.5]).bfloat16()
    weights = torch.linspace(3.0, 0.0, grid.numel()).exp()
    idx = torch.multinomial(weights, len(ROWS) * vocab, replacement=True, generator=gen).view(len(ROWS), vocab)
    logits = grid[idx]
    holes = torch.randint(0, vocab, (len(ROWS), 5), generator=gen)
    logits.scatter_(1, holes, float("-inf"))
    return logits


def kept_set(row, k, p, t):
    """One row's kept columns in float64, by the header's definition; asserts the margin around the top-p threshold."""
    l = row.double()
    keep = torch.ones_like(l, dtype=torch.bool)
    if 0 < k < l.numel():
        keep = l >= torch.topk(l, k).values[-1]
    if p < 1.0:
        w = torch.where(keep, ((l - l.max()) / t).exp(), torch.zeros_like(l))
        vals, inv = torch.unique(l[keep], return_inverse=True)  # ascending
        mass = torch.zeros_like(vals).index_add_(0, inv, w[keep])
        from_top = mass.flip(0).cumsum(0).flip(0)  # mass of {l >= vals[i]}
        total = w.sum()
        i = int((from_top >= p * total).nonzero().max())
        near = [from_top[i]] + ([from_top[i + 1]] if i + 1 < vals.numel() else [])
        assert all(abs(float(m - p * total)) >= 1e-3 * float(total) for m in near), "pick another generator seed"
        keep &= l >= vals[i]
    return keep


def on_device(logits, stride=None):
    """On the device with a row stride of whole 16-byte loads; the columns behind vocab would win every pick."""
    rows, vocab = logits.shape
    wide = torch.full((rows, stride or -(-vocab // 8) * 8), 100.0, dtype=torch.bfloat16, device="cuda")
    wide[:, :vocab] = logits.cuda()
    return wide[:, :vocab]


def check_case(logits_cpu, stride=None):
    logits_dev = on_device(logits_cpu, stride)
    rows = [(logits_cpu.shape[1] if k == "V" else k, p, t) for k, p, t in ROWS]
    masked = logits_cpu.clone()
    for r, (k, p, t) in enumerate(rows):
        if t > 0:
            masked[r, ~kept_set(logits_cpu[r], k, p, t)] = float("-inf")
    dev = "cuda"
    masked = on_device(masked, stride)
    top_k = torch.tensor([k for k, _, _ in rows], dtype=torch.int32, device=dev)
    top_p = torch.tensor([p for _, p, _ in rows], dtype=torch.float32, device=dev)
    temps = torch.tensor([t for _, _, t in rows], dtype=torch.float32, device=dev)
    greedy = ops.argmax(logits_dev).tolist()
    for seed, step in ((1234, 1), (2 ** 63 + 5, 987654321)):
        want = ops.sample(masked, temps, seed, step).tolist()
        full = ops.sample(logits_dev, temps, seed, step).tolist()
        out = torch.full((len(rows),), -7, dtype=torch.int64, device=dev)
        got = ops.sample_truncated(logits_dev, temps, top_k, top_p, seed, step, out=out).tolist()
        again = ops.sample_truncated(logits_dev, temps, top_k, top_p, seed, step, out=torch.zeros_like(out)).tolist()
        rng = torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed, step], dtype=torch.int64, device=dev)
        by_rng = ops.sample_truncated(logits_dev, temps, top_k, top_p, 0, 0, out=torch.zeros_like(out), rng=rng).tolist()
        assert got[0] == -7 and got[1:5] == want[1:5]  # truncation off: the row is not written
        assert got[4] == full[4] and got[5] == greedy[5]  # top_k = vocab, top_p = 1: the untruncated sampler
        assert again[1:] == got[1:] and by_rng[1:] == got[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("vocab,kind,stride", [(*c, None) for c in CASES] + [(1003, "grid", 1024)])
def test_kernel_picks_the_sampler_token_of_the_fp64_kept_set(vocab, kind, stride):
    """Tails of 3 and 5 columns, under one register pass, the real row, a row read from memory, a stride > vocab."""
    check_case(make_logits(vocab, kind, CASES[(vocab, kind)]), stride)


PROMPTS = [p.tolist() for p in torch.randint(0, 4096, (64,), generator=torch.Generator().manual_seed(0)).split((5, 33, 17, 9))]


def engine(lookahead):
    return LLM(make_model_dir(MID), kvcache_block_size=16, max_num_seqs=4, max_num_batched_tokens=256, max_model_len=128,
               num_kvcache_blocks=40, warmup=False, sampling_seed=1234, decode_lookahead=lookahead, synthetic_seed=1)


def generate(lookahead, sps):
    llm = engine(lookahead)
    try:
        return [o["token_ids"] for o in llm.generate(PROMPTS, sps, use_tqdm=False)]
    finally:
        llm.exit()


@pytest.fixture(scope="module")
def greedy_tokens():
    """The greedy streams, stepped synchronously; no sampled row has a tie at its maximum (top_k = 1 would keep both)."""
    llm = engine(False)
    try:
        seqs = [llm.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True, greedy=True)) for p in PROMPTS]
        while not llm.is_finished():
            step, is_prefill = llm.scheduler.schedule()
            toks = llm.model_runner.call("run", step, is_prefill)
            top2 = llm.model_runner.last_logits[: len(step)].float().topk(2, dim=-1).values
            assert bool((top2[:, 0] > top2[:, 1]).all())
            llm.scheduler.postprocess(step, toks)
        return [s.completion_token_ids for s in seqs]
    finally:
        llm.exit()


@pytest.mark.gpu
@pytest.mark.parametrize("lookahead", [False, True])
def test_top_k_1_generates_the_greedy_tokens(greedy_tokens, lookahead):
    """Prefill pick, decode graph pick and the lookahead chain: every token comes from the truncating launch."""
    sp = SamplingParams(temperature=1.0, top_k=1, max_tokens=8, ignore_eos=True)
    assert generate(lookahead, [sp] * len(PROMPTS)) == greedy_tokens


@pytest.mark.gpu
@pytest.mark.parametrize("lookahead", [False, True])
def test_truncating_neighbours_leave_the_other_rows_alone(lookahead):
    plain = SamplingParams(temperature=0.8, max_tokens=8, ignore_eos=True)
    trunc = SamplingParams(temperature=0.8, top_k=8, top_p=0.9, max_tokens=8, ignore_eos=True)
    base = generate(lookahead, [plain] * 4)
    mixed = generate(lookahead, [trunc, plain, trunc, plain])
    assert mixed[1] == base[1] and mixed[3] == base[3]
    assert mixed[0] != base[0] and mixed[2] != base[2]  # (4096 near-uniform columns: eight draws do not all fall in 8)


def test_sampling_params_validate_top_k_and_top_p():
    assert (SamplingParams().top_k, SamplingParams().top_p, SamplingParams(top_k=-1).top_k) == (0, 1.0, 0)  # -1: vLLM's "off"
    for bad in (dict(top_k=-2), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1)):
        with pytest.raises(AssertionError):
            SamplingParams(**bad)


def test_tensor_parallel_engine_refuses_a_truncating_request():
    eng = object.__new__(LLMEngine)  # (no device: add_request up to the refusal)
    eng.config, eng.scheduler = types.SimpleNamespace(tensor_parallel_size=2), types.SimpleNamespace(max_model_len=64)
    eng.block_size, eng.tokenizer = 16, None
    for sp in (SamplingParams(top_k=20), SamplingParams(top_p=0.8)):
        with pytest.raises(NotImplementedError, match="tensor_parallel_size"):
            eng.add_request([1, 2, 3], sp)
