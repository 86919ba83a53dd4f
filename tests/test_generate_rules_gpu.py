"""generate(repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, suppress_tokens=) end to end on the `tiny` synthetic model (fp32 engine): the ids
equal a host loop that runs forward() step by step and applies transformers' own processors to the last row before argmax, they differ from the plain
greedy ids (so the arguments are not swallowed), and every decode path — chained steps, a decode batch with one ruled member, the batching scheduler, a
chunked prefill, sampling — produces the same ids."""
import pytest
import torch

from logit_rules_ref import hf_process

pytestmark = pytest.mark.gpu

# Prompt seed: found by running the CPU oracle's greedy loop (oracle.llava_oracle.greedy_generate, which the fp32 engine reproduces id for id) over
# make_prompt seeds 0, 1, 2, ... and taking the first one whose 16 plain greedy ids hold a repeated id and a repeated bigram and for which each rule
# set below changes the ids.  The precondition is asserted again on the engine's own ids below.
PROMPT_SEED = 0
N_NEW = 16
IMAGE_TOKEN_INDEX = -200


@pytest.fixture(scope="module")
def tiny(cuda):
    from synthetic import build as harness
    from synthetic import recipes as synth
    cfg = synth.CONFIGS["tiny"]
    model = harness.build_model(cfg, dtype=torch.float32, seed=0)
    ids = torch.from_numpy(synth.make_prompt(cfg, 12, image_positions=(5,), seed=PROMPT_SEED))[None].cuda()
    pix = torch.from_numpy(synth.make_pixels(cfg, 1)).cuda()
    plain = model.generate(inputs=ids, images=pix, do_sample=False, max_new_tokens=N_NEW, eos_token_id=-1)[0, ids.shape[1]:].tolist()
    return model, cfg, ids, pix, plain


def _gen(model, ids, pix, **kw):
    kw.setdefault("eos_token_id", -1)
    kw.setdefault("max_new_tokens", N_NEW)
    return model.generate(inputs=ids, images=pix, do_sample=False, **kw)[0, ids.shape[1]:].tolist()


def _host_loop(model, ids, pix, n_new, penalty=1.0, ngram=0, min_new=0, eos=(), suppress=()):
    """forward() step by step; HF's processors on the last row upcast to fp32 (the image marker dropped from the history for the penalty only: HF's gather
    raises on it; for the n-gram processor it stays an id like any other); argmax.  Stops after an EOS id like generate()."""
    prompt = ids[0].tolist()
    out = model.forward(input_ids=ids, images=pix, use_cache=True)
    past, gen = out.past_key_values, []
    try:
        for _ in range(n_new):
            row = out.logits[0, -1].float().cpu()
            h = prompt + gen
            s = hf_process(row, [t for t in h if t != IMAGE_TOKEN_INDEX], len(gen), penalty=penalty)
            # the other processors see the marker as an id of its own: V, with one more (-inf) column for it, since a ban of the marker itself indexes the row
            V = row.numel()
            s = hf_process(torch.cat([s, torch.tensor([float("-inf")])]), [V if t == IMAGE_TOKEN_INDEX else t for t in h], len(gen), ngram=ngram,
                           min_new=min_new, eos=eos, suppress=suppress)[:V]
            tok = int(torch.argmax(s))
            gen.append(tok)
            if tok in eos:
                break
            out = model.forward(input_ids=torch.tensor([[tok]], device=ids.device), past_key_values=past, use_cache=True)
            past = out.past_key_values
    finally:
        if hasattr(past, "close"):
            past.close()
    return gen


def _rule_sets(plain):
    return {
        "penalty": (dict(repetition_penalty=1.3), dict(penalty=1.3)),
        "ngram": (dict(no_repeat_ngram_size=2), dict(ngram=2)),
        "both": (dict(repetition_penalty=1.3, no_repeat_ngram_size=2), dict(penalty=1.3, ngram=2)),
        "min_new": (dict(min_new_tokens=6, eos_token_id=plain[2]), dict(min_new=6, eos=[plain[2]])),
        "suppress": (dict(suppress_tokens=[plain[0]]), dict(suppress=[plain[0]])),
    }


def test_plain_ids_repeat(tiny):
    """The precondition of everything below: without rules the greedy ids repeat an id and a bigram."""
    _, _, _, _, plain = tiny
    assert len(plain) == N_NEW and len(set(plain)) < len(plain), plain
    bigrams = list(zip(plain, plain[1:]))
    assert len(set(bigrams)) < len(bigrams), plain


@pytest.mark.parametrize("name", ["penalty", "ngram", "both", "min_new", "suppress"])
def test_generate_follows_the_rules(tiny, name):
    model, _, ids, pix, plain = tiny
    gen_kw, ref_kw = _rule_sets(plain)[name]
    want = _host_loop(model, ids, pix, N_NEW, **ref_kw)
    got = _gen(model, ids, pix, **gen_kw)
    print(name, "plain", plain, "ruled", got)
    assert got == want, (name, got, want)
    assert got != plain, (name, got)
    if name == "min_new":
        assert plain[2] not in got[:6]
    # the same ids however the steps are issued
    for run_ahead in (1, 5, 16):
        assert _gen(model, ids, pix, run_ahead=run_ahead, **gen_kw) == got, (name, run_ahead)
    assert _gen(model, ids, pix, prefill_chunk=8, **gen_kw) == got, name
    model.enable_batching(capacity=4)
    try:
        assert _gen(model, ids, pix, **gen_kw) == got, name
    finally:
        model.disable_batching()
    # pool hygiene: the next plain request (a recycled sequence) carries no rules
    assert _gen(model, ids, pix) == plain


def test_min_length_folds_into_min_new_tokens(tiny):
    model, _, ids, pix, plain = tiny
    L = ids.shape[1]
    assert _gen(model, ids, pix, min_length=L + 6, eos_token_id=plain[2]) == _gen(model, ids, pix, min_new_tokens=6, eos_token_id=plain[2])
    assert _gen(model, ids, pix, bad_words_ids=[[plain[0]]]) == _gen(model, ids, pix, suppress_tokens=[plain[0]])


def test_batch_with_one_ruled_member(tiny):
    """Three rows decode together, only row 1 carries rules: the launch takes the rules-carrying pick, rows 0 and 2 leave it early and keep their plain ids."""
    from synthetic import recipes as synth
    model, cfg, ids, pix, plain = tiny
    prompts = [ids[0], ids[0], torch.from_numpy(synth.make_prompt(cfg, 12, image_positions=(5,), seed=PROMPT_SEED + 1)).cuda()]
    plain2 = _gen(model, prompts[2][None], pix)
    ruled = _gen(model, ids, pix, repetition_penalty=1.3, no_repeat_ngram_size=2)
    L = ids.shape[1]
    for packed in (True, False):
        outs = model.generate_batch(prompts, [pix, pix, pix], max_new_tokens=N_NEW, eos_token_id=-1, run_ahead=5, packed_prefill=packed,
                                    rules=[None, dict(repetition_penalty=1.3, no_repeat_ngram_size=2), None])
        assert [o[L:].tolist() for o in outs] == [plain, ruled, plain2], packed


def test_sampled_batch_with_one_ruled_member(tiny):
    """The same three rows drawn (fixed seed) twice: no member ruled — the plain launch, whose draws use the register-cached sampler — and row 1 ruled — the
    rules-carrying launch, whose draws all use the streaming sampler.  Rows 0 and 2 carry no rules either time and must draw the same ids."""
    from synthetic import recipes as synth
    model, cfg, ids, pix, _ = tiny
    prompts = [ids[0], ids[0], torch.from_numpy(synth.make_prompt(cfg, 12, image_positions=(5,), seed=PROMPT_SEED + 1)).cuda()]
    L = ids.shape[1]

    def gen(rules):
        torch.manual_seed(7)
        outs = model.generate_batch(prompts, [pix, pix, pix], max_new_tokens=N_NEW, eos_token_id=-1, run_ahead=5, do_sample=True, temperature=1.0,
                                    top_p=0.9, top_k=50, rules=rules)
        return [o[L:].tolist() for o in outs]
    plain = gen(None)
    mixed = gen([None, dict(no_repeat_ngram_size=1), None])
    print("plain", plain, "mixed", mixed)
    assert mixed[0] == plain[0] and mixed[2] == plain[2]
    assert len(set(mixed[1])) == len(mixed[1]) and not set(mixed[1]) & set(ids[0].tolist())        # n = 1: row 1 repeats nothing
    assert len(set(plain[0])) > 1                                                                  # the draws are not one id over and over


def test_sampled_generation_with_rules(tiny):
    """do_sample=True under a fixed seed: chained steps == step by step, and the rules hold on the drawn ids."""
    model, _, ids, pix, _ = tiny

    def gen(**kw):
        torch.manual_seed(5)
        return model.generate(inputs=ids, images=pix, do_sample=True, temperature=1.0, top_p=0.95, max_new_tokens=N_NEW, eos_token_id=-1,
                              no_repeat_ngram_size=1, **kw)[0, ids.shape[1]:].tolist()
    a = gen()
    assert a == gen(run_ahead=1) == gen(run_ahead=5)
    assert len(set(a)) == len(a) and not set(a) & set(ids[0].tolist())          # n = 1: no id of the prompt or of the output comes twice


def test_errors(tiny):
    model, _, ids, pix, _ = tiny
    with pytest.raises(NotImplementedError):
        _gen(model, ids, pix, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError):
        _gen(model, ids, pix, bad_words_ids=[[5, 6]])
    with pytest.raises(ValueError):
        _gen(model, ids, pix, repetition_penalty=-1.0)
    with pytest.raises(ValueError):
        _gen(model, ids, pix, no_repeat_ngram_size=-2)
