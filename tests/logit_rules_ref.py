"""CPU references for the device-side logits processors (csrc/sampling.hip, lmx_seq_set_logit_rules): transformers' own processors, and a restatement of
the rules' definition that also covers histories with ids outside [0, V) (the image marker -200, ids past the vocabulary), on which HF raises or wraps."""
import torch


def hf_process(row_f32, hist, n_out, penalty=1.0, ngram=0, min_new=0, eos=(), suppress=()):
    """The row after HF's processors in _get_logits_processor's order.  row_f32: [V] fp32 CPU; hist: list of ids in [0, V), the last n_out generated."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    ids = torch.tensor([list(hist)], dtype=torch.long)
    s = row_f32[None].clone()
    if penalty != 1.0 and len(hist):
        s = RepetitionPenaltyLogitsProcessor(float(penalty))(ids, s)
    if ngram > 0:
        s = NoRepeatNGramLogitsProcessor(int(ngram))(ids, s)
    if min_new > 0 and len(eos):
        s = MinNewTokensLengthLogitsProcessor(len(hist) - n_out, int(min_new), list(eos), device="cpu")(ids, s)
    if len(suppress):
        s = SuppressTokensLogitsProcessor(list(suppress), device="cpu")(ids, s)
    return s[0]


def restate(row_f32, hist, n_out, penalty=1.0, ngram=0, min_new=0, eos=(), suppress=()):
    """The rules as the header states them; ids outside [0, V) take no part."""
    V, h, s = row_f32.numel(), list(hist), row_f32.clone()
    seen = sorted({t for t in h if 0 <= t < V}) if penalty != 1.0 else []
    if seen:
        s[seen] = torch.where(s[seen] < 0, s[seen] * penalty, s[seen] / penalty)
    ban = set(suppress) | (set(eos) if n_out < min_new else set())
    if ngram >= 1 and len(h) + 1 >= ngram:
        ban |= {h[j + ngram - 1] for j in range(len(h) - ngram + 1) if h[j:j + ngram - 1] == h[len(h) - ngram + 1:]}
    s[[t for t in ban if 0 <= t < V]] = float("-inf")
    return s
