"""The decoder's linears — q|k|v (and its q and k|v row ranges), o_proj, gate|up, down_proj, lm_head — as the three layer walks of csrc/engine.cpp launch them
(prefill_piece, decode_step_launch, decode_batch) and as the rotated decode copies follow them.

Launch ledger: which launches a path issues, and how often, is part of what the engine computes (LlamaDecoderLayer's q / k / v / o / gate / up / down projections and
lm_head, HF5:models/llama/modeling_llama.py:243-281, 367-418, once per layer and token block).  The in-situ profile counts every scope by name; the expected maps below are
written out from the walks' source in terms of the layer count, the chained steps and the sequences of a piece, so a launch that goes missing, doubles or changes its
name fails here.

Copies follow launches: a rotated decode copy is laid out for the rows per wave of the launch that reads it.  At a geometry with rows of 2 and 3 load rounds and rows
per wave of 1 (o_proj, down_proj) and 2 (q, k|v, lm_head), decoding on the copies must give the bits of decoding on the plain weights, also after a reload behind
finalize."""
from dataclasses import replace

import pytest
import torch

from test_gemv_rot_gpu import _chained

pytestmark = pytest.mark.gpu

PREFIXES = ("prefill.", "decode.", "decode_batch.")


def _ledger(model, run):
    model.profile(True)
    try:
        run()
        torch.cuda.synchronize()
        prof = model.profile_read()
    finally:
        model.profile(False)
    return {k: v[1] for k, v in prof.items() if k.startswith(PREFIXES)}


def _prefill_map(L, seqs):
    """one piece holding the rows of `seqs` sequences, every sequence ending in it: one GEMM per linear over all rows, RoPE + KV append and attention per sequence
    (tiny is far below the tile count at which the q|k|v GEMM takes RoPE into its epilogue), the head's single-row launch per sequence; one process: no all-reduce"""
    return {"prefill.rmsnorm": 2 * L, "prefill.gemm.qkv": L, "prefill.rope_kv": L * seqs, "prefill.attn": L * seqs, "prefill.gemm.o": L,
            "prefill.gemm.gate_up": L, "prefill.gemm.down": L, "prefill.gemv.lm_head": seqs}


def _decode_map(L, steps, splitq):
    """`steps` chained steps of one lmx_decode call: the token's embedding once, then per step and layer the q|k|v projection in its split-q form (q launch +
    k|v-projection-with-attention launch) or its three-launch form (q|k|v launch + attention launch), o_proj, gate|up, down_proj; per step lm_head and the pick"""
    m = {"decode.embed": 1, "decode.gemv.o": L * steps, "decode.gemv.gate_up": L * steps, "decode.gemv.down": L * steps, "decode.gemv.lm_head": steps,
         "decode.argmax": steps}
    m.update({"decode.gemv.q": L * steps, "decode.kv_attn": L * steps} if splitq else {"decode.gemv.qkv": L * steps, "decode.attn": L * steps})
    return m


def _batch_map(L, steps):
    """`steps` steps of a decode batch of two or more in one process (no all-reduce launch that could carry the next norm): per step and layer four linears, two of
    them behind an RMSNorm launch, and the batched attention; per step the head behind the final norm and the pick"""
    return {"decode_batch.embed": 1, "decode_batch.rmsnorm": (2 * L + 1) * steps, "decode_batch.linear": (4 * L + 1) * steps, "decode_batch.attn": L * steps,
            "decode_batch.argmax": steps}


def _tiny(dtype):
    from synthetic import build as harness, recipes as synth
    cfg = synth.CONFIGS["tiny"]
    assert cfg.num_hidden_layers == 2
    return cfg, harness.build_model(cfg, dtype=dtype, seed=0)


def _prompt(cfg, n, seed, cuda):
    from synthetic import recipes as synth
    return torch.from_numpy(synth.make_prompt(cfg, n, image_positions=(), seed=seed))[None].to(cuda)


# (dtype, decode_splitq, decode_rot, the q|k|v form the step takes): the split-q form exists for 16-bit models only, the rotated copies change no launch.
# The fp32 engine has no rotated copies and refuses decode_rot = 1: its option stays as built
@pytest.mark.parametrize("dtype,splitq,rot,split_form", [(torch.bfloat16, 1, 1, True), (torch.bfloat16, 0, 1, False), (torch.bfloat16, 1, 0, True),
                                                         (torch.float32, 1, None, False)])
def test_launch_ledger_of_a_greedy_generate(cuda, dtype, splitq, rot, split_form):
    cfg, model = _tiny(dtype)
    L, new = cfg.num_hidden_layers, 4
    ids = _prompt(cfg, 12, 9, cuda)
    try:
        model.set_option("decode_splitq", splitq)
        if rot is not None:
            model.set_option("decode_rot", rot)
        got = _ledger(model, lambda: model.generate(inputs=ids, do_sample=False, max_new_tokens=new, eos_token_id=-1))
    finally:
        model.set_option("decode_splitq", 1)
        if rot is not None:
            model.set_option("decode_rot", 1)
    # the first new token is the prefill's pick, the other new - 1 are chained decode steps of one call
    assert got == {**_prefill_map(L, 1), **_decode_map(L, new - 1, split_form)}


def _prefilled_pair(model, cfg, cuda, packed):
    from llava_mi355x import _C
    from llava_mi355x.model import LmxKVCache
    rows = [model.get_model().embed_tokens(_prompt(cfg, n, 20 + n, cuda))[0].to(model.dtype).contiguous() for n in (9, 14)]
    cache = LmxKVCache(model, 2)
    if packed:
        model._prefill_packed(cache.seqs, rows)
    else:
        for s, e in zip(cache.seqs, rows):
            _C.check(_C.lib.lmx_prefill(model._h, s, _C.ptr(e), e.shape[0], 0, None, 0, 1, _C.stream_handle()))
    return cache


def test_launch_ledger_of_a_packed_prefill(cuda):
    cfg, model = _tiny(torch.bfloat16)
    caches = []
    try:
        got = _ledger(model, lambda: caches.append(_prefilled_pair(model, cfg, cuda, True)))
    finally:
        for c in caches:
            c.close()
    assert got == _prefill_map(cfg.num_hidden_layers, 2)


def test_launch_ledger_of_a_two_member_decode_batch(cuda):
    from llava_mi355x.batching import DecodeBatch
    cfg, model = _tiny(torch.bfloat16)
    steps = 3
    cache = _prefilled_pair(model, cfg, cuda, False)
    batch = DecodeBatch(model, 2)
    try:
        got = _ledger(model, lambda: batch.step(cache.seqs, None, steps, True))
    finally:
        batch.close()
        cache.close()
    assert got == _batch_map(cfg.num_hidden_layers, steps)


# ---- copies follow launches at a second geometry -----------------------------------------------------------------------------------------------------------
# hidden 1024 and intermediate 1536: weight rows of 2 and 3 load rounds (512 elements each), so the rotation moves data; o_proj and down_proj are small linears
# without a fused norm (1 row per wave), q, k|v and lm_head take 2
@pytest.fixture(scope="module")
def wide():
    from synthetic import build as harness
    cfg = _wide_cfg()
    return cfg, harness.build_model(cfg, dtype=torch.bfloat16, seed=6)


def _wide_cfg():
    from synthetic import recipes as synth
    cfg = replace(synth.CONFIGS["tiny"], name="wide_2_3_rounds", hidden_size=1024, intermediate_size=1536, num_hidden_layers=2, num_attention_heads=8,
                  num_key_value_heads=4, vocab_size=512, max_position_embeddings=256)
    assert cfg.head_dim == 128
    return cfg


@pytest.mark.parametrize("splitq", [1, 0])
def test_decode_on_the_copies_is_bit_identical_at_2_and_3_rounds(cuda, wide, splitq):
    """20 chained greedy steps from a 100-token prompt: the position crosses the 128-key boundary"""
    cfg, model = wide
    ids = _prompt(cfg, 100, 9, cuda)
    try:
        model.set_option("decode_splitq", splitq)
        model.set_option("decode_rot", 1)
        ia, la = _chained(model, ids, 20)
        model.set_option("decode_rot", 0)
        ib, lb = _chained(model, ids, 20)
    finally:
        model.set_option("decode_splitq", 1)
        model.set_option("decode_rot", 1)
    assert torch.equal(ia, ib)
    assert torch.equal(la, lb), (la.float() - lb.float()).abs().max().item()


def test_reloaded_weights_repack_their_copies_at_2_and_3_rounds(cuda, wide):
    """runs last on the shared model: it rewrites down_proj and q_proj of layer 1 behind finalize"""
    from synthetic import recipes as synth
    cfg, model = wide
    ids = _prompt(cfg, 20, 9, cuda)
    shapes = synth.tensor_shapes(cfg)
    gen = torch.Generator(device=cuda); gen.manual_seed(77)
    for n in ("model.layers.1.mlp.down_proj.weight", "model.layers.1.self_attn.q_proj.weight"):
        shp = shapes[n]
        model.load_tensor(n, torch.randn(shp, generator=gen, device=cuda) / shp[-1] ** 0.5)
    try:
        on = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
        model.set_option("decode_rot", 0)
        off = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
    finally:
        model.set_option("decode_rot", 1)
    assert torch.equal(on, off)


def test_copies_packed_while_the_weights_arrive_follow_the_finished_launch(cuda):
    """decode_rot switched on before any tensor is loaded: every copy is packed as its source arrives.  The norm weights come last here, so the q rows and lm_head
    are packed once before the launch that will read them is known to fuse a norm (which decides its rows per wave) and must follow when it is."""
    from llava_mi355x.model import LlavaLlamaForCausalLM
    from synthetic import build as harness, recipes as synth
    cfg = _wide_cfg()
    model = LlavaLlamaForCausalLM(*harness.hf_configs(cfg), dtype=torch.bfloat16)
    model.set_option("decode_rot", 1)
    names = sorted(synth.tensor_shapes(cfg).items(), key=lambda kv: "norm" in kv[0])      # stable: the norm weights move behind everything else
    for n, shp in names:
        model.load_tensor(n, torch.from_numpy(synth.make_tensor(cfg, n, shp, 6)))
    model.finalize_weights()
    model.get_vision_tower().is_loaded = True
    ids = _prompt(cfg, 20, 9, cuda)
    try:
        on = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
        model.set_option("decode_rot", 0)
        off = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
    finally:
        model.set_option("decode_rot", 1)
    assert torch.equal(on, off)
