"""The ruled pick (csrc/sampling.hip: the rules-carrying instantiations, through lmx_op_pick_rules) against transformers' own logits processors applied on
the CPU to the row upcast to fp32: the processed row bit for bit, the greedy pick = argmax of it (first index wins), a draw = the sampler's semantics
(tests/test_sampling_gpu.py) on it; the row in memory stays raw.  Histories HF cannot take (ids outside [0, V)) are checked against the restatement of
tests/logit_rules_ref.py, which tests/test_logit_rules_host.py holds to HF where both apply."""
import ctypes
import random

import numpy as np
import pytest
import torch

from logit_rules_ref import hf_process, restate
from test_sampling_gpu import _hf_keep

pytestmark = pytest.mark.gpu


def _pick(buf, V, hist, n_out, kw, sampling=None, u32=None, want_keep=False):
    """buf: device row buffer of ld >= V elements.  Returns (token, processed fp32 row on the CPU, keep mask or None)."""
    from llava_mi355x import _C
    dev = buf.device
    h = torch.tensor(list(hist) or [0], dtype=torch.long, device=dev)
    eos, sup = list(kw.get("eos", ())), list(kw.get("suppress", ()))
    e = (ctypes.c_int64 * max(1, len(eos)))(*eos)
    s = (ctypes.c_int64 * max(1, len(sup)))(*sup)
    out = torch.full((1,), -7, dtype=torch.long, device=dev)
    proc = torch.full((V,), 123.0, dtype=torch.float32, device=dev)
    keep = torch.zeros(V, dtype=torch.uint8, device=dev) if want_keep else None
    T, top_p, top_k = sampling or (0.0, 1.0, 0)
    uo = ctypes.pointer(ctypes.c_uint32(int(u32))) if u32 is not None else None
    _C.check(_C.lib.lmx_op_pick_rules(_C.torch_dtype_code(buf.dtype), _C.ptr(buf), V, buf.numel(), _C.ptr(h), len(hist), n_out,
                                      float(kw.get("penalty", 1.0)), int(kw.get("ngram", 0)), int(kw.get("min_new", 0)), e, len(eos), s, len(sup),
                                      float(T), float(top_p), int(top_k), 0, uo, _C.ptr(out), _C.ptr(proc), _C.ptr(keep), _C.stream_handle()), "lmx_op_pick_rules")
    torch.cuda.synchronize()
    return int(out.item()), proc.cpu(), (keep.cpu().numpy().astype(bool) if want_keep else None)


def _hist(rng, n, alphabet):
    return [rng.choice(alphabet) for _ in range(n)]


def _cases():
    rng = random.Random(11)
    c = []
    # V = 37: only the scalar tail loop of the argmax; histories of 0, 1 (n - 2), 2 (n - 1), 3 (n) ids around n = 3
    c.append(("empty", 37, 37, torch.float32, [], 0, dict(penalty=1.3, ngram=2, suppress=[5])))
    c.append(("one-id", 37, 37, torch.float32, [9], 1, dict(penalty=1.3, ngram=3)))
    c.append(("n-1-ids", 37, 37, torch.bfloat16, [9, 9], 1, dict(penalty=0.8, ngram=3)))
    c.append(("overlap", 37, 37, torch.float32, [4, 4, 4], 2, dict(ngram=3)))                  # the match h[0:2] overlaps the suffix h[1:3]
    c.append(("unigram", 37, 48, torch.float16, _hist(rng, 12, range(37)), 3, dict(ngram=1, penalty=1.3)))      # row pitch > V
    # V = 1000: several loads per thread; 1500 ids (more than threads) from a small alphabet: duplicates, repeated bigrams; 16 suppressed ids
    small = list(range(40, 90))
    c.append(("1500-ids", 1000, 1000, torch.bfloat16, _hist(rng, 1500, small), 700, dict(penalty=0.8, ngram=2, suppress=list(range(100, 116)))))
    c.append(("trigram", 1000, 1000, torch.float32, _hist(rng, 1500, small[:6]), 10, dict(penalty=1.3, ngram=3)))
    # min_new: n_out just below the threshold (EOS ids banned) and just at it (not banned)
    c.append(("min-below", 1000, 1000, torch.float32, _hist(rng, 20, small), 5, dict(min_new=6, eos=[3, 500, 999, 41], penalty=1.3)))
    c.append(("min-at", 1000, 1000, torch.float32, _hist(rng, 20, small), 6, dict(min_new=6, eos=[3, 500, 999, 41], ngram=2)))
    # V = 32000 (the plain pick's register path) and 32768 + 8 (its generic path)
    big = list(range(31000, 31050))
    c.append(("32000", 32000, 32064, torch.float16, _hist(rng, 1500, big), 100, dict(penalty=1.3, ngram=3, min_new=101, eos=[2], suppress=[31999])))
    c.append(("32776", 32776, 32776, torch.float32, _hist(rng, 300, big) + [32775, 32775], 2, dict(penalty=0.8, ngram=2, suppress=[0])))
    # ids outside [0, V): the image marker in the middle, an id >= V — checked against the restatement
    c.append(("marker", 1000, 1000, torch.float32, [7, 8, -200, 7, 8, 1000, 5, 7, 8], 4, dict(penalty=1.3, ngram=2, suppress=[1000, 12], min_new=9, eos=[-1, 6])))
    c.append(("marker-ngram", 1000, 1000, torch.bfloat16, [3, -200, 4, 3, -200], 0, dict(ngram=3, penalty=0.8)))
    return c


CASES = _cases()


def _row(V, ld, dt, hist, seed):
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(ld, generator=g) * 3.0
    for t in set(hist):
        if 0 <= t < V:
            row[t] += 4.0                   # the history's ids are the likely ones: the rules change the pick
    row[V:] = 1e4                           # padding behind the row must never be considered
    return row.to(dt)


def _reference(row, V, hist, n_out, kw):
    f = row[:V].float()
    in_range = all(0 <= t < V for t in list(hist) + list(kw.get("eos", ())) + list(kw.get("suppress", ())))
    return hf_process(f, hist, n_out, **kw) if in_range else restate(f, hist, n_out, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_processed_row_and_greedy_pick(cuda, case):
    name, V, ld, dt, hist, n_out, kw = case
    row = _row(V, ld, dt, hist, seed=V + len(hist))
    want = _reference(row, V, hist, n_out, kw)
    buf = row.to(cuda)
    before = buf.clone()
    tok, got, _ = _pick(buf, V, hist, n_out, kw)
    assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8))             # the logits row stays raw, byte for byte
    assert torch.equal(torch.isinf(got) & (got < 0), torch.isinf(want) & (want < 0)), name
    fin = torch.isfinite(want)
    assert torch.equal(got[fin], want[fin]), (name, (got[fin] != want[fin]).nonzero()[:8])
    assert tok == int(torch.argmax(want)), (name, tok, int(torch.argmax(want)))      # torch.argmax: the first index wins
    if hist and name not in ("min-at",):
        assert not torch.equal(want, row[:V].float()), name                          # the case is not vacuous


def test_all_banned_row_picks_zero(cuda):
    V = 37
    row = _row(V, V, torch.float32, [], 3)
    tok, got, _ = _pick(row.to(cuda), V, list(range(V)), 0, dict(ngram=1))
    assert bool(torch.all(torch.isinf(got) & (got < 0))) and tok == 0


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("1500-ids", "32000", "32776", "marker")], ids=["1500-ids", "32000", "32776", "marker"])
@pytest.mark.parametrize("T,top_p,top_k", [(1.0, 1.0, 0), (0.7, 0.9, 0), (0.8, 0.95, 40)])
def test_sampled_pick(cuda, case, T, top_p, top_k):
    """Survivors = HF's warpers on the processed row (differences only at the nucleus boundary, as in test_sampling_gpu.py); the drawn id = the float64
    inverse CDF over them for the uniform number used."""
    name, V, ld, dt, hist, n_out, kw = case
    row = _row(V, ld, dt, hist, seed=V + len(hist))
    want = _reference(row, V, hist, n_out, kw)
    ref_keep, _ = _hf_keep(want, T, top_p, top_k)
    buf = row.to(cuda)
    tok, _, keep = _pick(buf, V, hist, n_out, kw, sampling=(T, top_p, top_k), u32=123456789, want_keep=True)
    lf = want.numpy()
    diff = np.flatnonzero(keep != ref_keep)
    if len(diff):
        boundary = min(lf[keep].min(), lf[ref_keep].min())
        tied = np.isclose(lf[diff], boundary, rtol=0, atol=0)
        assert (~tied).sum() <= 1, (diff, lf[diff], boundary)
        assert np.all(lf[diff] <= np.partition(lf[keep], 1)[1] + 1e-6)
    assert keep[int(torch.argmax(want))] and not np.any(keep & np.isinf(lf))         # a banned id never survives
    e = np.exp((lf.astype(np.float64) - float(want.max())) / T) * keep
    cdf = np.cumsum(e)
    for u32 in (0, 123456789, 2 ** 31, 2 ** 32 - 1, 3141592653):
        tok, _, _ = _pick(buf, V, hist, n_out, kw, sampling=(T, top_p, top_k), u32=u32)
        assert keep[tok]
        target = (u32 / 2.0 ** 32) * cdf[-1]
        lo = cdf[tok - 1] if tok > 0 else 0.0
        tol = 1e-4 * cdf[-1]          # masses are 31-bit fixed point on the device: up to V * 2^-31 of drift along the CDF
        assert lo - tol <= target <= cdf[tok] + tol, (u32, tok, lo, target, cdf[tok])
