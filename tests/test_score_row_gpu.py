"""The score recorder on a caller-supplied row (csrc/sampling.hip: score_row_body, through ops.score_row / lmx_op_score_row) against tests/scores_ref.py: the
processed fp32 row HF's generate() would keep in `scores` — after the logits processors, and for a sampled request after temperature / top-k / top-p — bit for
bit, and its log-sum-exp and the token's log-probability against float64 within the bound the project holds its fp32 log-sum-exp to
(tests/test_beam_gpu.py: 2e-5 + 1e-5 |ref|).  Every row sits in a buffer of pitch ld > V whose tail is NaN: reading it would poison every figure."""
import pytest
import torch

from scores_ref import boundary_clear, log_softmax64, processed_row

pytestmark = pytest.mark.gpu

VOCABS = [257, 1027, 32000, 32776]      # fewer ids than threads | no multiple of 8 or 1024 | the model's | past the register-cached sampler's range (32768)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
RULES = dict(penalty=1.3, ngram=2, suppress=[7])
SAMPLED = [(0.7, 0, 0.9), (0.7, 50, 0.9)]      # (temperature, top_k, top_p)
MODES = [("greedy", None, None), ("greedy-ruled", RULES, None), ("sampled-k0", None, SAMPLED[0]), ("sampled-k50", None, SAMPLED[1]),
         ("sampled-ruled", RULES, SAMPLED[1])]
U32 = 2654435769


def _history(V):
    g = torch.Generator().manual_seed(V + 1)
    alphabet = torch.randperm(V, generator=g)[:12].tolist()
    idx = torch.randint(0, 12, (40,), generator=g).tolist()
    return [alphabet[i] for i in idx]


def _row(kind, V, dt, hist, seed):
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(V, generator=g) * 8.0
    for t in set(hist):
        row[t] += 12.0                      # the history's ids are the likely ones: the rules change the row where it matters
    if kind == "dominant":
        row[V // 3] = 200.0                 # log-prob of the pick ~ 0
    if kind == "holes":
        row[torch.randperm(V, generator=g)[: V // 10]] = float("-inf")
    return row.to(dt)


def _case_row(kind, V, dt, hist, rules, sampling):
    """The first seed whose row has no id at a warper boundary (scores_ref.boundary_clear): there the device's survivor set must equal HF's exactly."""
    for seed in range(1000 * V, 1000 * V + 64):
        row = _row(kind, V, dt, hist, seed)
        if sampling is None or boundary_clear(processed_row(row, V, hist, 3, rules), sampling):
            return row
    raise AssertionError("no seed with a clear warper boundary")


def _score(buf, V, hist, rules, sampling, token):
    from llava_mi355x import ops
    kw = dict(rules or {})
    if sampling is not None:
        kw.update(temperature=sampling[0], top_k=sampling[1], top_p=sampling[2], u32=U32)
    row, lse, lp, redraw = ops.score_row(buf, V, history=hist, n_out=min(3, len(hist)), token=token, **kw)      # the references use n_out = 3 on a 40-id history
    return row.cpu(), lse, lp, redraw


def _close(got, ref):
    return abs(got - ref) <= 2e-5 + 1e-5 * abs(ref)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("V", VOCABS)
def test_row_lse_and_logprob(cuda, V, dt):
    hist = _history(V)
    ld = V + 24
    for kind in ("normal", "dominant", "holes"):
        for name, rules, sampling in MODES:
            row = _case_row(kind, V, dt, hist, rules, sampling)
            greedy_row = processed_row(row, V, hist, 3, rules)
            if sampling is not None:
                assert boundary_clear(greedy_row, sampling), (kind, name)         # the precondition of an exact survivor set
            want = processed_row(row, V, hist, 3, rules, sampling)
            lse64, lsm64 = log_softmax64(want)
            buf = torch.full((ld,), float("nan"), dtype=dt)
            buf[:V] = row
            buf = buf.to(cuda)
            before = buf.clone()
            token = -1 if sampling is not None else int(torch.argmax(want))
            got, lse, lp, redraw = _score(buf, V, hist, rules, sampling, token)
            tag = (kind, name, V, dt)
            assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), tag            # the logits row stays raw, byte for byte
            assert torch.equal(torch.isinf(got) & (got < 0), torch.isinf(want) & (want < 0)), (tag, int((torch.isinf(got) != torch.isinf(want)).sum()))
            fin = torch.isfinite(want)
            assert not bool(torch.isnan(got).any()) and torch.equal(got[fin], want[fin]), (tag, (got[fin] != want[fin]).nonzero()[:8])
            if sampling is not None:
                assert 0 <= redraw < V and bool(torch.isfinite(got[redraw])), (tag, redraw)     # the id re-drawn under the same number survived
                token = redraw
            else:
                assert redraw == -1
            print(tag, "lse", lse, float(lse64), "logprob", lp, float(lsm64[token]), "finite", int(fin.sum()))
            assert _close(lse, float(lse64)), (tag, lse, float(lse64))
            assert _close(lp, float(lsm64[token])), (tag, lp, float(lsm64[token]))
            if kind == "dominant" and rules is None:
                assert abs(lp) < 1e-3, (tag, lp)
            if rules is not None:
                assert not torch.equal(greedy_row, row[:V].float()), tag                          # the rules are not vacuous
            # another token of the same row: the log-prob is the row's entry minus the same lse
            other = int(torch.argmin(torch.where(fin, want, torch.full_like(want, float("inf")))))
            got2, lse2, lp2, _ = _score(buf, V, hist, rules, sampling, other)
            # ... and a second call gives identical bits
            assert torch.equal(got2.view(torch.int32), got.view(torch.int32)), tag
            assert torch.tensor(lse2).view(torch.int32).item() == torch.tensor(lse).view(torch.int32).item(), tag
            assert _close(lp2, float(lsm64[other])), (tag, lp2, float(lsm64[other]))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
def test_row_without_a_finite_entry_gives_nan(cuda, dt):
    import math
    V = 257
    buf = torch.full((V + 7,), float("-inf"), dtype=dt)
    buf[V:] = float("nan")
    buf = buf.to(cuda)
    got, lse, lp, _ = _score(buf, V, [], None, None, 5)
    assert bool((torch.isinf(got) & (got < 0)).all()) and math.isnan(lse) and math.isnan(lp)
    got, lse, lp, _ = _score(buf, V, [], None, SAMPLED[0], 5)
    assert bool((torch.isinf(got) & (got < 0)).all()) and math.isnan(lse) and math.isnan(lp)
    # every id banned by the rules: the same
    row = torch.randn(V).to(dt)
    got, lse, lp, _ = _score(row.to(cuda), V, list(range(V)), dict(ngram=1), None, 5)
    assert bool((torch.isinf(got) & (got < 0)).all()) and math.isnan(lse) and math.isnan(lp)


def test_bad_arguments_are_refused(cuda):
    from llava_mi355x import _C, ops
    buf = torch.zeros(64, device=cuda)
    with pytest.raises(_C.LmxError):
        ops.score_row(buf, 64, token=64)                    # token outside [0, V)
    with pytest.raises(_C.LmxError):
        ops.score_row(buf, 64, token=-1)                    # "the re-drawn id" of a greedy row
    with pytest.raises(_C.LmxError):
        ops.score_row(buf, 65, token=0)                     # V beyond the buffer
