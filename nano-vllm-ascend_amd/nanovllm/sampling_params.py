"""Per-request sampling knobs (reference: nanovllm/sampling_params.py:5-11)."""
from dataclasses import dataclass


@dataclass
class SamplingParams:
    temperature: float = 1.0
    max_tokens: int = 64
    ignore_eos: bool = False
    # Extension over the reference (which only has multinomial sampling and rejects
    # temperature -> 0): deterministic argmax decoding, needed for parity runs
    # (BASELINE config 1 "greedy decode").  Default keeps the reference behaviour.
    greedy: bool = False
    # Truncated sampling (mi_sample_truncated, include/mi355_nanovllm.h): keep the top_k most likely tokens (0 or -1:
    # off; ties at the threshold are kept), then the smallest set of them whose probability reaches top_p (1.0: off).
    # One GPU only: a tensor-parallel engine refuses such a request.
    top_k: int = 0
    top_p: float = 1.0

    def __post_init__(self):
        assert self.temperature > 1e-10, "greedy sampling is not permitted (pass greedy=True for argmax)"
        if self.top_k == -1:
            self.top_k = 0
        assert self.top_k >= 0, "top_k is a count of tokens (0 or -1: off)"
        assert 0.0 < self.top_p <= 1.0, "top_p is a probability in (0, 1]"
