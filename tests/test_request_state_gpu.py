"""A request's sampling, stop, rules and score-log state as ONE value (llava_mi355x/model.py: RequestOptions, _apply_request_options; csrc/engine.h:
Seq::end_request) on the `tiny` synthetic model, fp32 verification engine:

  1. a request that carries all four kinds of state at once gives the same sequences, log-probabilities and score rows through generate() with one row,
     generate_batch of that one prompt (per-request prefill) and generate_batch of three prompts against three single generate() calls;
  2. the three ways a request's state ends — the pool round trip, lmx_seq_reset, lmx_seq_truncate — clear exactly what include/llava_mi355x.h says they
     clear: reset keeps the sampling parameters and the stop rule, the other two keep nothing;
  3. generate_batch neither reads nor fills the prefix cache.

Bounds (tests/test_generate_scores_gpu.py): a one-member decode batch takes the single-sequence step, so generate() and generate_batch of one prompt agree
bit for bit.  A batch of three runs its linears through the GEMM family where a single request takes the GEMV: score rows agree within the decode-vs-prefill
bound 1e-5 x max(1, max |row|) (fp32), log-probabilities within twice the fp32 log-sum-exp bound 2e-5 + 1e-5 |ref| plus twice the row bound."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# Prompt seed: chosen on the MI355X among make_prompt seeds 0..3.  With this one the 12 plain greedy ids hold an id at position >= 6 that does not occur
# before it (the stop id of the first two tests; row 2 of the batch of three draws it and stops there), the sampled runs differ from the greedy ids and from
# each other, and the stop rule of the clearance tests holds three different ids.  Seed 2 does not qualify: its draws with and without rules coincide.
# The preconditions are asserted again below.
PROMPT_SEED = 3
N_NEW = 12
SAMPLING = dict(temperature=0.9, top_p=0.8, top_k=20)
RULES = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
ENGINE_SEED = 1234567          # sampler seed of the C-ABI tests (generate() draws its own from torch's CPU generator)


def _build(cuda):
    from synthetic import build as harness, recipes as synth
    cfg = synth.CONFIGS["tiny"]
    return cfg, harness.build_model(cfg, dtype=torch.float32, seed=0, weights=synth.make_weights(cfg, 0))


def _prompt(cfg, cuda, seed):
    from synthetic import recipes as synth
    return torch.from_numpy(synth.make_prompt(cfg, 40, image_positions=(5,), seed=seed))[None].to(cuda)


def _late_new(tokens, start):
    """index >= start of an id that does not occur earlier in the run: a stop rule on it fires exactly there"""
    k = next((i for i in range(start, len(tokens) - 1) if tokens[i] not in tokens[:i]), None)
    assert k is not None, tokens
    return k


@pytest.fixture(scope="module")
def tiny(cuda):
    """(cfg, model, fresh model, ids, pixels, the fresh model's plain greedy ids): computed once, left unchanged."""
    from synthetic import recipes as synth
    cfg, model = _build(cuda)
    _, fresh = _build(cuda)
    ids = _prompt(cfg, cuda, PROMPT_SEED)
    pix = torch.from_numpy(synth.make_pixels(cfg, 1, seed=3)).to(cuda, torch.float32)
    free = fresh.generate(inputs=ids, images=pix, do_sample=False, max_new_tokens=N_NEW, eos_token_id=-1)[0, ids.shape[1]:].tolist()
    return cfg, model, fresh, ids, pix, free


# ---- 1. the paths agree -------------------------------------------------------------------------------------------------------------------------------
def _single(model, ids, pix, eos):
    return model.generate(inputs=ids, images=pix, do_sample=True, max_new_tokens=N_NEW, eos_token_id=eos, return_dict_in_generate=True, output_scores=True,
                          **SAMPLING, **RULES)


def _batch(model, prompts, pix, eos, packed):
    """generate_batch of requests that each carry the four kinds of state -> [(new ids, logprobs [n] CPU, rows [n, V])]"""
    outs, logs = model.generate_batch([p[0] for p in prompts], [pix] * len(prompts), max_new_tokens=N_NEW, eos_token_id=eos, do_sample=True, rules=dict(RULES),
                                      packed_prefill=packed, score_rows=True, **SAMPLING)
    return [(o[p.shape[1]:].tolist(), g["logprobs"], g["scores"]) for o, p, g in zip(outs, prompts, logs)]


def _unpack(out, L):
    """a one-row GenerateScoresOutput in _batch's form"""
    return out.sequences[0, L:].tolist(), out.logprobs[0].cpu(), torch.stack([s[0] for s in out.scores])


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_one_request_through_generate_and_generate_batch(tiny):
    cfg, model, _, ids, pix, free = tiny
    eos = free[_late_new(free, 6)]
    torch.manual_seed(0)
    toks, lp, rows = _unpack(_single(model, ids, pix, eos), ids.shape[1])
    torch.manual_seed(0)
    (btoks, blp, brows), = _batch(model, [ids], pix, eos, packed=False)
    print("generate", toks, "generate_batch", btoks, "greedy", free, "eos", eos)
    assert 1 <= len(toks) <= N_NEW and toks != free[:len(toks)]                 # a draw under rules, not the greedy ids
    assert eos not in toks[:-1] and rows.shape == (len(toks), cfg.vocab_size)
    assert btoks == toks
    assert torch.equal(_bits(blp), _bits(lp)) and torch.equal(_bits(brows), _bits(rows))


def test_three_requests_batched_against_three_single_calls(tiny):
    cfg, model, _, ids, pix, free = tiny
    eos = free[_late_new(free, 6)]
    prompts = [ids] + [_prompt(cfg, ids.device, PROMPT_SEED + s) for s in (1, 2)]
    L = ids.shape[1]
    torch.manual_seed(0)                                                       # one seed draw per request, in request order, on both sides
    singles = [_unpack(_single(model, p, pix, eos), L) for p in prompts]
    torch.manual_seed(0)
    batched = _batch(model, prompts, pix, eos, packed=True)
    for b, ((toks, lp, rows), (btoks, blp, brows)) in enumerate(zip(singles, batched)):
        print("row", b, "single", toks, "batched", btoks)
        assert btoks == toks, b
        assert torch.equal(torch.isinf(brows), torch.isinf(rows)), b
        fin = torch.isfinite(rows)
        bound = 1e-5 * max(1.0, float(rows[fin].abs().max()))
        err = float((brows[fin] - rows[fin]).abs().max())
        lp_err = (blp - lp).abs()
        lp_bound = 2 * (2e-5 + 1e-5 * lp.abs()) + 2 * bound
        print("row", b, "max |rows - single rows|", err, "bound", bound, "max logprob error", float(lp_err.max()), "bound", float(lp_bound.min()))
        assert err <= bound, (b, err, bound)
        assert bool((lp_err <= lp_bound).all()), (b, lp_err, lp_bound)
    assert len({tuple(t) for t, _, _ in singles}) == 3


# ---- 2. the clearance matrix --------------------------------------------------------------------------------------------------------------------------
def _prefill(model, ids, pix, **opts):
    """_prefill_request with the options given by name -> the request's cache; its first pick is on the device"""
    from llava_mi355x.model import RequestOptions
    return model._prefill_request(ids, pix, None, RequestOptions(**opts))


def _tokens(model, seq):
    from llava_mi355x._C import check, lib, stream_handle
    host = (ctypes.c_int64 * 64)(); n = ctypes.c_int32(0)
    check(lib.lmx_seq_read_tokens(seq, host, 64, ctypes.byref(n), stream_handle()), "read_tokens")
    return [int(host[i]) for i in range(n.value)]


def _decode(model, seq):
    from llava_mi355x._C import check, lib, stream_handle
    check(lib.lmx_decode(model._h, seq, -1, N_NEW - 1, None, 1, stream_handle()), "lmx_decode")          # chained on the device: a stop rule cuts them
    return _tokens(model, seq)


def _request(model, ids, pix, **opts):
    """One request on a fresh (or pooled) sequence with the given options -> its ids.  The sequence goes back to the pool."""
    cache = _prefill(model, ids, pix, **opts)
    try:
        return _decode(model, cache.seqs[0])
    finally:
        cache.close()


def _stopped(seq):
    from llava_mi355x._C import check, lib, stream_handle
    f = ctypes.c_int32(0)
    check(lib.lmx_seq_stopped(seq, ctypes.byref(f), stream_handle()), "stopped")
    return bool(f.value)


@pytest.fixture(scope="module")
def loaded_spec(tiny):
    """The request whose state the three entry points end, and what fresh sequences give: `sampled` = its sampler alone (no rules, no stop), `stop` = a rule
    of three ids: one that cuts the loaded request itself, one that would cut `sampled`, one that would cut the plain greedy ids."""
    _, _, fresh, ids, pix, free = tiny
    sampling = (SAMPLING["temperature"], SAMPLING["top_p"], SAMPLING["top_k"], ENGINE_SEED)
    rules = fresh._rules_spec(RULES, set(), ids.shape[1])
    loaded = _request(fresh, ids, pix, sampling=sampling, rules=rules)
    sampled = _request(fresh, ids, pix, sampling=sampling)
    stop = (sorted({loaded[_late_new(loaded, 2)], sampled[_late_new(sampled, 2)], free[_late_new(free, 2)]}), [])
    kept = _request(fresh, ids, pix, sampling=sampling, stop=stop)             # what reset keeps: the sampler and the stop rule, nothing else
    print("greedy", free, "loaded", loaded, "sampled", sampled, "stop", stop, "kept", kept)
    assert len(free) == len(loaded) == len(sampled) == N_NEW and sampled != free and loaded != sampled
    assert len(kept) < N_NEW and kept == sampled[:len(kept)] and kept != free[:len(kept)]
    return sampling, rules, stop, kept


def _load(model, ids, pix, spec):
    """A sequence that carries sampling, a stop rule that has fired, rules and a score log with rows."""
    sampling, rules, stop, _ = spec
    cache = _prefill(model, ids, pix, sampling=sampling, stop=stop, rules=rules, score_log=(N_NEW, True))
    try:
        got = _decode(model, cache.seqs[0])
        assert len(got) < N_NEW and got[-1] in stop[0] and _stopped(cache.seqs[0])
        assert len(model._read_scores(cache.seqs[0], len(got), True)["logprobs"]) == len(got)
    except BaseException:
        cache.close()
        raise
    return cache


def _prefill_on(model, cache, ids, pix, skip=0):
    """The prompt's rows from `skip` on into an existing sequence, no option touched; the first pick is the sequence's own."""
    p = model._prepare_request(ids, pix, None)
    try:
        model._prefill_rows(cache, p["embeds"][:, skip:], None if p["valid"] is None else p["valid"][:, skip:], want_all=False, greedy=True)
    finally:
        p["cache"].close()


def _refuses_scores(seq):
    from llava_mi355x import _C
    host = (ctypes.c_float * 4)(); n = ctypes.c_int32(0)
    with pytest.raises(_C.LmxError, match="no score log"):
        _C.check(_C.lib.lmx_seq_read_scores(seq, host, 4, ctypes.byref(n), None, _C.stream_handle()), "read_scores")


def test_pool_round_trip_clears_everything(tiny, loaded_spec):
    from llava_mi355x._C import lib
    from llava_mi355x.model import LmxKVCache
    _, model, _, ids, pix, free = tiny
    cache = _load(model, ids, pix, loaded_spec)
    handle = cache.seqs[0].value
    cache.close()                                                              # lmx_seq_destroy: to the pool
    cache = LmxKVCache(model, 1)                                               # lmx_seq_create: the same sequence again
    try:
        seq = cache.seqs[0]
        assert seq.value == handle and lib.lmx_seq_length(seq) == 0
        _refuses_scores(seq)
        _prefill_on(model, cache, ids, pix)
        assert _decode(model, seq) == free and not _stopped(seq)
        _refuses_scores(seq)
    finally:
        cache.close()


def test_truncate_clears_everything_but_the_rows_it_keeps(tiny, loaded_spec):
    from llava_mi355x._C import check, lib, stream_handle
    _, model, _, ids, pix, free = tiny
    cache = _load(model, ids, pix, loaded_spec)
    try:
        seq = cache.seqs[0]
        check(lib.lmx_seq_truncate(seq, 24, stream_handle()), "lmx_seq_truncate")          # the first 24 spliced rows are this prompt's (24 % 8 == 0)
        assert lib.lmx_seq_length(seq) == 24
        _refuses_scores(seq)
        _prefill_on(model, cache, ids, pix, skip=24)
        assert _decode(model, seq) == free and not _stopped(seq)              # exact engine: a suffix prefill is a chunked prefill
        _refuses_scores(seq)
    finally:
        cache.close()


def test_reset_keeps_sampling_and_the_stop_rule_only(tiny, loaded_spec):
    from llava_mi355x._C import check, lib, stream_handle
    _, model, _, ids, pix, free = tiny
    _, _, stop, kept = loaded_spec
    cache = _load(model, ids, pix, loaded_spec)
    try:
        seq = cache.seqs[0]
        torch.cuda.synchronize()                                               # lmx_seq_reset: no work on the sequence may be in flight
        check(lib.lmx_seq_reset(seq), "lmx_seq_reset")
        assert lib.lmx_seq_length(seq) == 0 and not _stopped(seq)             # the flag is cleared, the rule is not:
        _refuses_scores(seq)
        _prefill_on(model, cache, ids, pix)
        got = _decode(model, seq)
        print("after reset", got, "a fresh sequence with the sampler and the stop rule", kept)
        assert got == kept and _stopped(seq) and got[-1] in stop[0]           # the old sampler's draws (no rules any more), cut by the old stop id
        _refuses_scores(seq)
    finally:
        cache.close()
    # the pool round trip behind it drops the kept columns as well
    assert _request(model, ids, pix) == free


# ---- 3. generate_batch and the prefix cache -----------------------------------------------------------------------------------------------------------
def test_generate_batch_neither_hits_nor_fills_the_prefix_cache(tiny):
    cfg, model, _, ids, pix, free = tiny
    L = ids.shape[1]
    other = _prompt(cfg, ids.device, PROMPT_SEED + 1)
    model.enable_reuse(images=4, prefixes=4, min_rows=16)
    try:
        first = model.generate(inputs=ids, images=pix, do_sample=False, max_new_tokens=N_NEW, eos_token_id=-1)          # fills the cache with this prompt
        assert first[0, L:].tolist() == free
        before = model.reuse_stats()
        assert before["prefix_entries"] == 1 and before["prefix_hits"] == 0
        for packed in (True, False):
            outs = model.generate_batch([ids[0], other[0]], [pix, pix], max_new_tokens=N_NEW, eos_token_id=-1, packed_prefill=packed)
            assert outs[0][L:].tolist() == free, packed
            after = model.reuse_stats()
            after.update(image_hits=before["image_hits"])                      # the image-feature cache serves generate_batch too: two hits per call
            assert after == before, (packed, after, before)
        # the entry is still there for the request it belongs to
        again = model.generate(inputs=ids, images=pix, do_sample=False, max_new_tokens=N_NEW, eos_token_id=-1)
        assert torch.equal(again, first) and model.reuse_stats()["prefix_hits"] == 1
    finally:
        model.disable_reuse()
