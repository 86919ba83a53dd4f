"""generate(return_dict_in_generate=True, output_scores=True) end to end on the `tiny` synthetic model (fp32 engine, one case in bf16): the device score log
(lmx_seq_set_score_log; csrc/sampling.hip: score_record_kernel) gives HF's `scores` and the tokens' log-probabilities without changing a single id.

Bounds: a log-probability against float64 over the recorded row: 2e-5 + 1e-5 |ref| (tests/test_beam_gpu.py's fp32 log-sum-exp bound); rows against a host
loop over forward(), and single-request rows against decode-batch rows: the decode-vs-prefill bound of tests/test_model_gpu.py
(test_cache_chunk_and_chain_properties): 1e-5 (fp32) or 2e-2 (16-bit) x max(1, max |logit|)."""
import ctypes

import pytest
import torch

from scores_ref import log_softmax64, processed_row

pytestmark = pytest.mark.gpu

PROMPT_SEED = 0          # as tests/test_generate_rules_gpu.py: the plain greedy ids of this prompt repeat an id and a bigram
N_NEW = 16
IMAGE_TOKEN_INDEX = -200
RULED = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
SAMPLED = dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=50)


def _build(dtype):
    from synthetic import build as harness
    from synthetic import recipes as synth
    cfg = synth.CONFIGS["tiny"]
    model = harness.build_model(cfg, dtype=dtype, seed=0)
    ids = torch.from_numpy(synth.make_prompt(cfg, 12, image_positions=(5,), seed=PROMPT_SEED))[None].cuda()
    pix = torch.from_numpy(synth.make_pixels(cfg, 1)).cuda().to(dtype)
    return model, cfg, ids, pix


@pytest.fixture(scope="module")
def tiny(cuda):
    return _build(torch.float32)


def _gen(model, ids, pix, seed=None, **kw):
    kw.setdefault("eos_token_id", -1)
    kw.setdefault("max_new_tokens", N_NEW)
    kw.setdefault("do_sample", False)
    if seed is not None:
        torch.manual_seed(seed)
    return model.generate(inputs=ids, images=pix, **kw)


def _scored(model, ids, pix, seed=None, **kw):
    return _gen(model, ids, pix, seed=seed, return_dict_in_generate=True, output_scores=True, **kw)


@pytest.fixture(scope="module")
def plain_scored(tiny):
    """The plain greedy request's outputs, computed once and left unchanged."""
    model, _, ids, pix = tiny
    return _scored(model, ids, pix)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return (torch.equal(a.sequences, b.sequences) and len(a.scores) == len(b.scores) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a.scores, b.scores))
            and torch.equal(_bits(a.logprobs), _bits(b.logprobs)))


def _check_self_consistent(out, L, greedy):
    """argmax(scores[t]) is the token at t (greedy: first index on ties, torch.argmax); logprobs[t] = float64 log_softmax(scores[t])[tok] within the bound."""
    toks = out.sequences[0, L:].tolist()
    assert len(toks) == len(out.scores) == out.logprobs.shape[1]
    for t, tok in enumerate(toks):
        row = out.scores[t][0].cpu()
        assert bool(torch.isfinite(row[tok])), (t, tok)
        if greedy:
            assert int(torch.argmax(row)) == tok, (t, tok, int(torch.argmax(row)))
        ref = float(log_softmax64(row)[1][tok])
        got = float(out.logprobs[0, t])
        print("step", t, "tok", tok, "logprob", got, "float64", ref)
        assert abs(got - ref) <= 2e-5 + 1e-5 * abs(ref), (t, got, ref)


@pytest.mark.parametrize("name", ["greedy", "ruled", "sampled"])
def test_sequences_unchanged_and_shapes(tiny, plain_scored, name):
    model, cfg, ids, pix = tiny
    kw, seed = {"greedy": ({}, None), "ruled": (RULED, None), "sampled": (SAMPLED, 5)}[name]
    want = _gen(model, ids, pix, seed=seed, **kw)
    out = plain_scored if name == "greedy" else _scored(model, ids, pix, seed=seed, **kw)
    assert isinstance(want, torch.Tensor) and torch.equal(out.sequences, want)
    L, V = ids.shape[1], cfg.vocab_size
    assert out.sequences.shape == (1, L + N_NEW) and len(out.scores) == N_NEW
    assert all(s.shape == (1, V) and s.dtype == torch.float32 and s.is_cuda for s in out.scores)
    assert out.logprobs.shape == (1, N_NEW) and out.logprobs.dtype == torch.float32
    _check_self_consistent(out, L, greedy=name != "sampled")
    assert out["sequences"] is out.sequences and out[0] is out.sequences                     # a ModelOutput: by key and by position too


def test_recorded_rows_are_the_raw_logits_at_the_c_abi(tiny):
    """Greedy, no rules: the recorded row of every step is the step's logits row upcast to fp32, bit for bit — the prefill's returned row, then lmx_decode's."""
    from llava_mi355x import _C
    from llava_mi355x.model import RequestOptions
    model, cfg, ids, pix = tiny
    V, steps = cfg.vocab_size, 6
    cache, first = model._prefill_request(ids, pix, None, RequestOptions(score_log=(steps + 1, True)), return_logits=True)
    try:
        seq = cache.seqs[0]
        bufs = []
        for _ in range(steps):
            buf = torch.zeros(model._vocab_cap, dtype=model.dtype, device=model.device)
            _C.check(_C.lib.lmx_decode(model._h, seq, -1, 1, _C.ptr(buf), 1, _C.stream_handle()), "lmx_decode")
            bufs.append(buf)
        got = model._read_scores(seq, steps + 1, True)
        rows = got["scores"]
        assert rows.shape == (steps + 1, V)
        assert torch.equal(_bits(rows[0]), _bits(first.reshape(-1)[:V].float()))
        for t, buf in enumerate(bufs):
            assert torch.equal(_bits(rows[t + 1]), _bits(buf[:V].float())), t
        assert bool(torch.isfinite(got["logprobs"]).all()) and bool((got["logprobs"] < 0).all())
    finally:
        cache.close()


def _host_rows(model, ids, pix, toks, rules=None):
    """forward() step by step, fed with the request's own ids; scores_ref on the last row of every step."""
    prompt = [t for t in ids[0].tolist() if t != IMAGE_TOKEN_INDEX]          # HF's gather raises on the marker (tests/test_generate_rules_gpu.py)
    out = model.forward(input_ids=ids, images=pix, use_cache=True)
    past, rows, raw_max = out.past_key_values, [], 0.0
    try:
        for t, tok in enumerate(toks):
            raw = out.logits[0, -1]
            raw_max = max(raw_max, float(raw.float().abs().max()))
            rows.append(processed_row(raw, raw.numel(), prompt + toks[:t], t, rules))
            if t + 1 < len(toks):
                out = model.forward(input_ids=torch.tensor([[tok]], device=ids.device), past_key_values=past, use_cache=True)
                past = out.past_key_values
    finally:
        if hasattr(past, "close"):
            past.close()
    return rows, raw_max


def _check_against_host(model, ids, pix, out, tol, rules=None):
    L = ids.shape[1]
    toks = out.sequences[0, L:].tolist()
    rows, raw_max = _host_rows(model, ids, pix, toks, rules)
    bound = tol * max(1.0, raw_max)
    for t, want in enumerate(rows):
        got = out.scores[t][0].cpu()
        assert torch.equal(torch.isinf(got), torch.isinf(want)), t
        fin = torch.isfinite(want)
        err = float((got[fin] - want[fin]).abs().max())
        print("step", t, "max |row - host row|", err, "bound", bound)
        assert err <= bound, (t, err, bound)


def test_rows_against_a_host_loop(tiny, plain_scored):
    model, _, ids, pix = tiny
    _check_against_host(model, ids, pix, plain_scored, 1e-5)
    # with rules: the penalty divides / multiplies the ids of the history (|row| only shrinks or grows by 1.3: the bound is taken on 1.3 x the raw maximum)
    ruled = _scored(model, ids, pix, repetition_penalty=1.3, suppress_tokens=[int(plain_scored.sequences[0, -1])])
    _check_against_host(model, ids, pix, ruled, 1.3e-5, rules=dict(penalty=1.3, suppress=[int(plain_scored.sequences[0, -1])]))


def test_bf16_request(cuda):
    model, cfg, ids, pix = _build(torch.bfloat16)
    want = _gen(model, ids, pix)
    out = _scored(model, ids, pix)
    assert torch.equal(out.sequences, want) and len(out.scores) == N_NEW and out.scores[0].dtype == torch.float32
    _check_self_consistent(out, ids.shape[1], greedy=True)
    _check_against_host(model, ids, pix, out, 2e-2)
    # the rows are bf16 values upcast: every finite entry is representable in bf16
    row = out.scores[3][0]
    assert torch.equal(row, row.to(torch.bfloat16).float())


def test_ruled_and_sampled_rows(tiny, plain_scored):
    model, cfg, ids, pix = tiny
    L = ids.shape[1]
    banned = int(plain_scored.sequences[0, L])
    ruled = _scored(model, ids, pix, suppress_tokens=[banned], no_repeat_ngram_size=1)
    toks = ruled.sequences[0, L:].tolist()
    history = set(t for t in ids[0].tolist() if 0 <= t < cfg.vocab_size)
    for t, tok in enumerate(toks):
        row = ruled.scores[t][0]
        assert float(row[banned]) == float("-inf") and bool(torch.isfinite(row[tok]))
        gone = sorted(history | set(toks[:t]))                       # n-gram size 1: no id of the prompt or of the output so far may come again
        assert bool(torch.isinf(row[gone]).all()), t
    assert not any(torch.equal(a, b) for a, b in zip(ruled.scores, plain_scored.scores))
    sampled = _scored(model, ids, pix, seed=5, **SAMPLED)
    toks = sampled.sequences[0, L:].tolist()
    for t, tok in enumerate(toks):
        row = sampled.scores[t][0]
        n_fin = int(torch.isfinite(row).sum())
        assert 1 <= n_fin <= 50 and bool(torch.isfinite(row[tok])), (t, n_fin)            # top_k = 50: everything else is -inf
        assert bool((torch.isinf(row) & (row < 0)).sum() == row.numel() - n_fin)
        ref = float(log_softmax64(row.cpu())[1][tok])
        assert abs(float(sampled.logprobs[0, t]) - ref) <= 2e-5 + 1e-5 * abs(ref)
    # the first step sees the same logits as the plain request: its survivors are the plain row / temperature (a true fp32 division)
    row0, plain0 = sampled.scores[0][0], plain_scored.scores[0][0]
    fin = torch.isfinite(row0)
    assert torch.equal(row0[fin].cpu(), (plain0.cpu() / torch.tensor(0.7, dtype=torch.float32))[fin.cpu()])
    assert not torch.equal(row0, plain0)


@pytest.mark.parametrize("name", ["greedy", "ruled", "sampled"])
def test_same_bits_however_the_steps_are_issued(tiny, plain_scored, name):
    model, _, ids, pix = tiny
    kw, seed = {"greedy": ({}, None), "ruled": (RULED, None), "sampled": (SAMPLED, 5)}[name]
    base = plain_scored if name == "greedy" else _scored(model, ids, pix, seed=seed, **kw)
    for run_ahead in (1, 5, 16):
        assert _same_bits(_scored(model, ids, pix, seed=seed, run_ahead=run_ahead, **kw), base), (name, run_ahead)
    assert _same_bits(_scored(model, ids, pix, seed=seed, prefill_chunk=8, **kw), base), name
    # a streamer and stopping criteria take the one-step-at-a-time loop
    class Sink:
        def put(self, v): pass
        def end(self): pass
    assert _same_bits(_scored(model, ids, pix, seed=seed, streamer=Sink(), **kw), base), name
    assert _same_bits(_scored(model, ids, pix, seed=seed, stopping_criteria=[lambda full, _: False], **kw), base), name


def test_batch_of_three_with_an_early_stop(tiny, plain_scored):
    """B = 3 through generate_batch, row 0 stopping early at an EOS id.  The fp32 engine's decode batch runs its linears through the GEMM family, a single
    request through the GEMV: the logits agree within the decode-vs-prefill bound, not bit for bit, and so do the rows and log-probabilities (the prefill's
    pick — entry 0 — comes from the packed prefill on one side and lmx_prefill on the other, the same bound)."""
    from synthetic import recipes as synth
    model, cfg, ids, pix = tiny
    L = ids.shape[1]
    prompts = [ids[0]] + [torch.from_numpy(synth.make_prompt(cfg, 12, image_positions=(5,), seed=PROMPT_SEED + s)).cuda() for s in (1, 2)]
    singles_plain = [plain_scored] + [_scored(model, p[None], pix) for p in prompts[1:]]
    others = set(singles_plain[1].sequences[0, L:].tolist()) | set(singles_plain[2].sequences[0, L:].tolist())
    row0 = plain_scored.sequences[0, L:].tolist()
    k = next(i for i, t in enumerate(row0) if 2 <= i < N_NEW - 2 and t not in others and t not in row0[:i])
    eos = row0[k]
    singles = [_scored(model, p[None], pix, eos_token_id=eos) for p in prompts]
    assert singles[0].logprobs.shape[1] == k + 1 and singles[1].logprobs.shape[1] == N_NEW
    out = _scored(model, torch.stack(prompts), torch.cat([pix, pix, pix]), eos_token_id=eos, pad_token_id=0)
    assert isinstance(out.sequences, torch.Tensor) and out.sequences.shape == (3, L + N_NEW) and len(out.scores) == N_NEW and out.logprobs.shape == (3, N_NEW)
    assert all(s.shape == (3, cfg.vocab_size) for s in out.scores)
    for b, single in enumerate(singles):
        n = single.logprobs.shape[1]
        assert out.sequences[b, L:L + n].tolist() == single.sequences[0, L:].tolist(), b
        for t in range(n):
            got, want = out.scores[t][b], single.scores[t][0]
            bound = 1e-5 * max(1.0, float(want.abs().max()))
            assert float((got - want).abs().max()) <= bound, (b, t)
            ref = float(single.logprobs[0, t])
            # each side within the fp32 bound of its own row's float64 value; rows that differ by <= bound move p[tok] and the log-sum-exp by <= bound each
            assert abs(float(out.logprobs[b, t]) - ref) <= 2 * (2e-5 + 1e-5 * abs(ref)) + 2 * bound, (b, t)
    # behind row 0's stop: 0.0, in the rows and in the log-probabilities (HF would go on with the pad continuation: a documented divergence)
    assert all(bool((out.scores[t][0] == 0).all()) for t in range(k + 1, N_NEW))
    assert bool((out.logprobs[0, k + 1:] == 0).all()) and bool((out.logprobs[0, :k + 1] < 0).all())
    assert bool((out.sequences[0, L + k + 1:] == 0).all())


def test_device_stop_records_nothing_past_it(tiny, plain_scored):
    from llava_mi355x import _C
    from llava_mi355x.model import RequestOptions
    model, _, ids, pix = tiny
    L = ids.shape[1]
    row0 = plain_scored.sequences[0, L:].tolist()
    k = next(i for i, t in enumerate(row0) if i >= 2 and t not in row0[:i])
    out = _scored(model, ids, pix, eos_token_id=row0[k])
    assert out.sequences.shape[1] == L + k + 1 and len(out.scores) == k + 1 and out.logprobs.shape == (1, k + 1)
    assert torch.equal(_bits(out.logprobs), _bits(plain_scored.logprobs[:, :k + 1]))
    # at the C ABI: steps queued past the stop leave the log where the stop left it
    cache = model._prefill_request(ids, pix, None, RequestOptions(stop=([row0[k]], []), score_log=(N_NEW, False)))
    try:
        seq = cache.seqs[0]
        _C.check(_C.lib.lmx_decode(model._h, seq, -1, N_NEW - 1, None, 1, _C.stream_handle()), "lmx_decode")
        host = (ctypes.c_float * N_NEW)()
        n = ctypes.c_int32(-1)
        _C.check(_C.lib.lmx_seq_read_scores(seq, host, N_NEW, ctypes.byref(n), None, _C.stream_handle()), "lmx_seq_read_scores")
        assert n.value == k + 1
        assert all(v < 0 for v in list(host)[:k + 1])
        with pytest.raises(_C.LmxError):          # attached without rows
            _C.check(_C.lib.lmx_seq_read_scores(seq, host, N_NEW, ctypes.byref(n), _C.ptr(torch.zeros(4, device=model.device)), _C.stream_handle()), "read_scores")
    finally:
        cache.close()


def test_pool_hygiene(tiny, plain_scored):
    """A scored request's sequence goes back to the pool; the plain request that takes it records nothing and returns a tensor; the next scored one starts at
    entry 0 (same bits as before); a recycled sequence has no log until one is attached."""
    from llava_mi355x import _C
    from llava_mi355x.model import LmxKVCache
    model, _, ids, pix = tiny
    a = _scored(model, ids, pix)
    plain = _gen(model, ids, pix)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, a.sequences)
    assert _same_bits(_scored(model, ids, pix), plain_scored) and _same_bits(a, plain_scored)
    cache = LmxKVCache(model, 1)          # the recycled sequence
    try:
        host = (ctypes.c_float * 4)()
        n = ctypes.c_int32(0)
        with pytest.raises(_C.LmxError):
            _C.check(_C.lib.lmx_seq_read_scores(cache.seqs[0], host, 4, ctypes.byref(n), None, _C.stream_handle()), "read_scores")
    finally:
        cache.close()


def test_compute_transition_scores(tiny, plain_scored):
    model, _, ids, pix = tiny
    L = ids.shape[1]
    for out in (plain_scored, _scored(model, ids, pix, seed=5, **SAMPLED)):
        norm = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
        assert norm.shape == out.logprobs.shape
        assert bool(((norm - out.logprobs).abs() <= 2 * (2e-5 + 1e-5 * out.logprobs.abs())).all())          # both sides are fp32 against the same float64 value
        raw = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=False)
        toks = out.sequences[0, L:].tolist()
        assert raw[0].tolist() == [float(out.scores[t][0, tok]) for t, tok in enumerate(toks)]


def test_argument_handling(tiny, plain_scored):
    model, _, ids, pix = tiny
    only_dict = _gen(model, ids, pix, return_dict_in_generate=True)
    assert only_dict.scores is None and torch.equal(only_dict.sequences, plain_scored.sequences)
    assert torch.equal(_bits(only_dict.logprobs), _bits(plain_scored.logprobs))
    only_scores = _gen(model, ids, pix, output_scores=True)
    assert isinstance(only_scores, torch.Tensor) and torch.equal(only_scores, plain_scored.sequences)
    none = _scored(model, ids, pix, max_new_tokens=0)
    assert none.sequences.shape == ids.shape and none.scores == () and none.logprobs.shape == (1, 0)
    with pytest.raises(NotImplementedError, match="num_beams"):
        _scored(model, ids, pix, num_beams=2)
    model.enable_batching(capacity=2)
    try:
        with pytest.raises(NotImplementedError, match="enable_batching"):
            _scored(model, ids, pix)
        assert torch.equal(_gen(model, ids, pix), plain_scored.sequences)
    finally:
        model.disable_batching()
