"""The restatement of the logits-processor rules that the GPU tests use for histories HF cannot take (ids outside [0, V)) agrees with transformers' own
processors wherever both apply: 200 random in-range cases, bit for bit."""
import random

import torch

from logit_rules_ref import hf_process, restate


def test_restatement_matches_hf_processors_on_in_range_histories():
    rng = random.Random(7)
    g = torch.Generator().manual_seed(7)
    for case in range(200):
        V = rng.choice([5, 37, 200])
        n_hist = rng.choice([0, 1, 2, 3, 7, 40])
        hist = [rng.randrange(min(V, 6) if case % 2 else V) for _ in range(n_hist)]          # small alphabets make n-grams repeat
        n_out = rng.randint(0, n_hist)
        kw = dict(penalty=rng.choice([1.0, 1.3, 0.8]), ngram=rng.choice([0, 1, 2, 3]), min_new=rng.choice([0, n_out, n_out + 1]),
                  eos=rng.sample(range(V), rng.randint(0, 4)), suppress=rng.sample(range(V), rng.choice([0, 1, 5])))
        row = torch.randn(V, generator=g) * 3
        want, got = hf_process(row, hist, n_out, **kw), restate(row, hist, n_out, **kw)
        assert torch.equal(torch.isinf(want), torch.isinf(got)), (case, V, hist, kw)
        fin = torch.isfinite(want)
        assert torch.equal(want[fin], got[fin]), (case, V, hist, kw)
