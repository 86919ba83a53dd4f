"""The yardstick of the score tests (tests/scores_ref.py) held to transformers' own classes: the restated warpers give the bits of TemperatureLogitsWarper ->
TopKLogitsWarper -> TopPLogitsWarper, the processed row is hf_process + those, and the float64 log-softmax agrees with torch.log_softmax.  No GPU."""
import pytest
import torch

from scores_ref import boundary_clear, log_softmax64, processed_row, warp

SAMPLING = [(0.7, 0, 0.9), (0.7, 50, 0.9), (1.0, 0, 1.0), (1.3, 5, 1.0), (0.2, 0, 0.5), (2.0, 40, 0.99)]


def _rows(V):
    g = torch.Generator().manual_seed(V)
    normal = torch.randn(V, generator=g) * 8.0
    dominant = normal.clone()
    dominant[V // 3] = 200.0
    holes = normal.clone()
    holes[torch.randperm(V, generator=g)[: V // 10]] = float("-inf")
    return {"normal": normal, "dominant": dominant, "holes": holes}


def _hf_warp(row, T, top_k, top_p):
    lp = pytest.importorskip("transformers.generation.logits_process")
    ids = torch.zeros((1, 1), dtype=torch.long)
    s = lp.TemperatureLogitsWarper(float(T))(ids, row[None].clone())
    if top_k:
        s = lp.TopKLogitsWarper(int(top_k))(ids, s)
    if top_p < 1.0:
        s = lp.TopPLogitsWarper(float(top_p))(ids, s)
    return s[0]


@pytest.mark.parametrize("V", [257, 1027, 32000])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_warpers_equal_transformers(V, dt):
    for name, row in _rows(V).items():
        row = row.to(dt).float()
        for T, k, p in SAMPLING:
            got, want = warp(row, T, k, p), _hf_warp(row, T, k, p)
            assert torch.equal(torch.isinf(got), torch.isinf(want)), (name, T, k, p)
            fin = torch.isfinite(want)
            assert torch.equal(got[fin], want[fin]), (name, T, k, p)
            assert bool(torch.isfinite(got[int(torch.argmax(row))]))          # the most likely id always stays


def test_processed_row_is_processors_then_warpers():
    from logit_rules_ref import hf_process
    pytest.importorskip("transformers")
    V = 1027
    row = _rows(V)["normal"].to(torch.bfloat16)
    hist = [5, 9, 5, 9, 700, 5]
    rules = dict(penalty=1.3, ngram=2, suppress=[11])
    greedy = processed_row(row, V, hist, 2, rules)
    assert torch.equal(greedy, hf_process(row.float(), hist, 2, **rules))
    assert not torch.equal(greedy, row.float()) and greedy[11] == float("-inf") and greedy[9] == float("-inf")
    sampled = processed_row(row, V, hist, 2, rules, (0.7, 50, 0.9))
    want = _hf_warp(greedy, 0.7, 50, 0.9)
    assert torch.equal(torch.isinf(sampled), torch.isinf(want)) and torch.equal(sampled[torch.isfinite(want)], want[torch.isfinite(want)])
    assert processed_row(torch.cat([row, torch.full((13,), float("nan"), dtype=row.dtype)]), V).numel() == V          # a pitch > V is cut off


def test_log_softmax64_against_torch():
    for name, row in _rows(1027).items():
        s = warp(row, 0.7, 50, 0.9)
        lse, lsm = log_softmax64(s)
        want = torch.log_softmax(s.double(), dim=-1)
        assert torch.equal(lsm, want), name
        fin = torch.isfinite(s)
        assert torch.allclose(s.double()[fin] - lse, want[fin], rtol=0, atol=1e-12), name
        assert abs(float(torch.exp(lsm[fin]).sum()) - 1.0) < 1e-12
        # fp32 torch agrees with the float64 figures within the bound the GPU tests use
        f32 = torch.log_softmax(s, dim=-1)
        assert bool(((f32[fin].double() - want[fin]).abs() <= 2e-5 + 1e-5 * want[fin].abs()).all()), name
    lse, lsm = log_softmax64(torch.full((37,), float("-inf")))
    assert bool(torch.isnan(lse)) or float(lse) == float("-inf")
    assert bool(torch.isnan(lsm).all())


def test_boundary_precondition_detects_ties():
    row = torch.tensor([0.0, 1.0, 2.0, 3.0, 3.0, -1.0])
    assert not boundary_clear(row, (1.0, 1, 1.0))           # the top-1 cut runs through the tie 3.0 / 3.0
    assert boundary_clear(row, (1.0, 2, 1.0))
    assert boundary_clear(torch.tensor([0.0, 5.0, 10.0]), (1.0, 0, 0.9))
    two = torch.tensor([0.0, 0.0])                          # cumulative probability 0.5 exactly at 1 - top_p
    assert not boundary_clear(two, (1.0, 0, 0.5))
