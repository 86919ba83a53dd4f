"""CPU yardstick for the score recorder (csrc/sampling.hip: score_record_kernel / lmx_op_score_row; generate(output_scores=True)): what HF's generate() keeps in
`scores` for one step, and float64 log-probabilities over it.

  raw row in its stored dtype -> float32 -> HF's logits processors (tests/logit_rules_ref.py:hf_process) -> for a sampled request the three warpers in
  sample()'s order (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper), restated here in the same fp32 operations -> float64 log_softmax.

tests/test_scores_host.py holds the restatement to transformers' own classes and to torch.log_softmax."""
import torch

from logit_rules_ref import hf_process


def warp(row_f32, temperature, top_k=0, top_p=1.0):
    """TemperatureLogitsWarper (a true fp32 division), TopKLogitsWarper (`scores < k-th largest` leave), TopPLogitsWarper (ascending sort; ids whose inclusive
    cumulative probability is <= 1 - top_p leave, the most likely one always stays).  row_f32: [V] fp32 CPU."""
    s = row_f32 / torch.tensor(float(temperature), dtype=torch.float32)
    if top_k and top_k > 0:
        k = min(int(top_k), s.numel())
        s = s.masked_fill(s < torch.topk(s, k)[0][-1], float("-inf"))
    if top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(s, descending=False)
        remove = sorted_logits.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[-1:] = False
        s = s.masked_fill(torch.zeros_like(remove).scatter(0, sorted_idx, remove), float("-inf"))
    return s


def processed_row(row_stored, V, hist=(), n_out=0, rules=None, sampling=None):
    """HF's `scores` entry for the step: [V] fp32.  row_stored: the raw row (any float dtype, >= V elements); rules: hf_process's keywords or None;
    sampling: (temperature, top_k, top_p) or None for a greedy request."""
    s = row_stored[:V].float().cpu()
    if rules:
        s = hf_process(s, list(hist), n_out, **rules)
    if sampling is not None:
        s = warp(s, *sampling)
    return s


def log_softmax64(row_f32):
    """(log-sum-exp, log_softmax) of the row in float64; NaN where no entry is finite, as torch.log_softmax gives."""
    d = row_f32.double()
    return torch.logsumexp(d, dim=-1), torch.log_softmax(d, dim=-1)


def boundary_clear(row_f32_processed, sampling, eps=1e-4):
    """The precondition under which a device survivor set must EQUAL the reference's: no id sits at a warper's boundary.  top-k: the k-th largest value is
    not shared with the (k+1)-th (a tie class would straddle the cut);  top-p: in float64, the inclusive ascending cumulative probability of the last id that
    leaves and of the first that stays are both further than eps from 1 - top_p (fp32 cumulative sums on the host and 31-bit fixed-point masses on the
    device differ by ~V * 2^-31 ~ 1.5e-5 at V = 32000), and the two ids' values differ."""
    temperature, top_k, top_p = sampling
    s = (row_f32_processed / torch.tensor(float(temperature), dtype=torch.float32)).double()
    V = s.numel()
    if top_k and 0 < top_k < V:
        top = torch.topk(s, int(top_k) + 1)[0]
        if not bool(top[-2] > top[-1]):
            return False
        s = s.masked_fill(s < top[-2], float("-inf"))
    if top_p < 1.0:
        v, _ = torch.sort(s, descending=False)
        c = v.softmax(dim=-1).cumsum(dim=-1)
        cut = 1.0 - top_p
        n_remove = int((c[:-1] <= cut).sum())          # the last one always stays
        if n_remove > 0 and (abs(float(c[n_remove - 1]) - cut) <= eps or not bool(v[n_remove - 1] < v[n_remove])):
            return False
        if n_remove < V - 1 and abs(float(c[n_remove]) - cut) <= eps:
            return False
    return True
