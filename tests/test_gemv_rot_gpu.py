"""Rotated decode copies of the batch-1 decode weights (csrc/gemv2.h: gemv2_body's ROT form; csrc/elementwise.hip: gemv_rot_pack_kernel; engine option
"decode_rot") against the plain weights.

The decode-step linears of one new token (HF5:models/llama/modeling_llama.py:163-176,243-281) stream a weight whose rows were re-laid at load: row n of wave
slot s = n // R keeps its logical 1-KiB load round j at physical round (j + (s * step) % NR) % NR.  The kernel walks the physical rounds from its own start
and sums the logical rounds in the plain order, so every output must have the SAME BITS as the plain launch on the plain weight: torch.equal, no tolerance.
Checked per op (every (R, P) form of the single-row launch, fused RMSNorm, residual, steps 1 and 3), for the split-q launch's k | v projection, and through the
engine over 40 chained greedy steps with the option on against off."""
import pytest
import torch

from test_ops_gpu import DT, _fill_cache, _rope_table

pytestmark = pytest.mark.gpu


def _unpack(w_rot, N, K, R, step):
    """inverse gather of the layout, on the host side of the statement: logical 16-byte chunk c of row n sits at physical round (c // 64 + (n // R * step) % NR) % NR"""
    NR = w_rot.shape[1] // 512
    n = torch.arange(N, device=w_rot.device)[:, None]
    c = torch.arange(K // 8, device=w_rot.device)[None, :]
    p = (c // 64 + (n // R * step) % NR) % NR
    chunks = w_rot.view(N, NR * 64, 8)
    return chunks[n, p * 64 + c % 64].reshape(N, K)


# (N, K): NR = 1 (the rotation is the identity) | NR = 2 | NR = 3 with a ragged last round, N no multiple of 4 R | the 7B hidden width, R = 2 |
# the R = 1, P = 8 form, NR = 22, ragged
SHAPES = [(8, 512), (40, 1024), (33, 1032), (64, 4096), (24, 11008)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_on_the_rotated_copy_is_bit_identical(cuda, dt, N, K):
    from llava_mi355x import _C, ops
    torch.manual_seed(N + K)
    T = DT[dt]
    w = (torch.randn(N, K, device=cuda) / K ** 0.5).to(T)
    x = torch.randn(1, K, device=cuda).to(T)
    g = (1 + 0.1 * torch.randn(K, device=cuda)).to(T)
    res = torch.randn(1, N, device=cuda).to(T)
    pitch = _C.lib.lmx_op_gemv_rot_pitch(K)
    assert pitch == -(-K // 512) * 512
    for norm in (None, g):
        R = _C.lib.lmx_op_gemv_rot_rows(N, K, int(norm is not None), _C.ACT_NONE)
        for step in (1, 3):
            w_rot = ops.gemv_rot_pack(w, step, norm=norm is not None)
            assert tuple(w_rot.shape) == (N, pitch)
            assert torch.equal(_unpack(w_rot, N, K, R, step), w), (R, step)
            if K % 512:                                                  # the tail of the ragged logical round is zero, wherever the round went
                NR = pitch // 512
                n = torch.arange(N, device=cuda)
                p = (NR - 1 + (n // R * step) % NR) % NR
                tail = w_rot.view(N, NR, 512)[n, p][:, K % 512:]
                assert not tail.any()
            for r in (None, res):
                ref = ops.gemv(x, w, norm_w=norm, residual=r)
                got = ops.gemv_rot(x, w_rot, K, step, norm_w=norm, residual=r)
                assert torch.equal(got, ref), (R, step, norm is not None, r is not None, (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gate_up_pairing_on_the_rotated_copy_is_bit_identical(cuda, dt):
    """SiLU*mul launch: a wave holds a gate row and its up row, 32 rows apart — the copy follows that wave's slot, not n // R."""
    from llava_mi355x import _C, ops
    torch.manual_seed(5)
    T = DT[dt]
    N, K = 128, 1536
    w = (torch.randn(N, K, device=cuda) / K ** 0.5).to(T)
    x = torch.randn(1, K, device=cuda).to(T)
    g = (1 + 0.1 * torch.randn(K, device=cuda)).to(T)
    ref = ops.gemv(x, w, norm_w=g, act=_C.ACT_SILU_MUL)
    for step in (1, 3):
        w_rot = ops.gemv_rot_pack(w, step, norm=True, act=_C.ACT_SILU_MUL)
        assert torch.equal(ops.gemv_rot(x, w_rot, K, step, norm_w=g, act=_C.ACT_SILU_MUL), ref), step


def test_a_copy_is_refused_where_its_kernel_does_not_run(cuda):
    """No other GEMV form may read a rotated copy: fp32 has no hand-counted stream, and the error is loud."""
    from llava_mi355x import _C, ops
    w = torch.randn(8, 512, device=cuda)
    with pytest.raises(_C.LmxError):
        ops.gemv_rot_pack(w, 1)
    with pytest.raises(_C.LmxError):
        ops.gemv_rot(torch.randn(1, 512, device=cuda), torch.zeros(8, 512, device=cuda), 512, 1)


# the smallest geometry of test_ops_gpu's split-q op test (K = 512: one round) and its smallest with more than one round (K = 1536: NR = 3, GQA)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nh,nkv,D,K", [(4, 4, 128, 512), (4, 2, 128, 1536)])
@pytest.mark.parametrize("pos", [0, 128])
def test_decode_kv_attn_on_rotated_kv_rows_is_bit_identical(cuda, dt, nh, nkv, D, K, pos):
    """decode_kv_attn_kernel with the packed k | v rows against the plain rows: an empty cache, a position just past a 128-key boundary; the granule buffer is
    reused across the launches with the next tag (stale tags of the plain launches in it).  Same attention output, same K / V^T caches."""
    from llava_mi355x import ops
    torch.manual_seed(pos + K)
    T = DT[dt]
    s_max = 256
    table = _rope_table(s_max, D).to(cuda)
    k_past = torch.randn(pos, nkv, D, device=cuda).to(T); v_past = torch.randn(pos, nkv, D, device=cuda).to(T)
    w = (torch.randn((nh + 2 * nkv) * D, K, device=cuda) / K ** 0.5).to(T)
    g = (1 + 0.1 * torch.randn(K, device=cuda)).to(T)
    gran = torch.zeros(2 * nkv * D, dtype=torch.int64, device=cuda)
    tag = 7
    for step in (1, 3):
        w_rot = ops.gemv_rot_pack(w[nh * D:], step, rows_per_wave=2)
        for norm in (g, None):
            x = torch.randn(1, K, device=cuda).to(T)
            q_row = ops.gemv(x, w, norm_w=norm, eps=1e-5)[0]
            q_row[nh * D:] = float("nan")                                # the k | v columns of the row are not to be read
            kc, vt = _fill_cache(k_past, v_past, s_max, T, cuda)
            ref = ops.decode_kv_attn(q_row.clone(), x[0], w[nh * D:], norm, 1e-5, kc, vt, table, pos, nh, nkv, D, granules=gran, tag=tag).clone()
            kc2, vt2 = _fill_cache(k_past, v_past, s_max, T, cuda)
            got = ops.decode_kv_attn(q_row.clone(), x[0], w_rot, norm, 1e-5, kc2, vt2, table, pos, nh, nkv, D, granules=gran, tag=tag + 1, rot=step)
            tag += 2
            assert torch.equal(got, ref), (step, norm is not None, (got.float() - ref.float()).abs().max().item())
            assert torch.equal(kc2, kc) and torch.equal(vt2, vt)


def _chained(model, ids, n):
    out = model.forward(input_ids=ids, use_cache=True)
    past = out.past_key_values
    tok = out.logits[:, -1].argmax(-1, keepdim=True)
    picked = [tok]
    for _ in range(n):
        out = model.forward(input_ids=picked[-1], past_key_values=past, use_cache=True)
        picked.append(out.logits[:, -1].argmax(-1, keepdim=True))
    past.close()
    return torch.cat(picked, 1), out.logits[:, -1].clone()


# the tiny synthetic config (every row one round: the packed pitch and the ROT kernels, identity rotation) and one 7B-width layer (NR = 8 and 22)
@pytest.mark.parametrize("name,layers", [("tiny", None), ("llava15_7b", 1)])
@pytest.mark.parametrize("splitq", [1, 0])
def test_engine_decode_rot_on_against_off(cuda, name, layers, splitq):
    """40 chained greedy steps from a 100-token context (the position crosses the 128-key boundary), decode_rot on against off, with the split-q step and
    with the three-launch form: ids of every step and the final logits equal; generate() (the prefill's lm_head GEMV + the device-side step loop) too."""
    from synthetic import build as harness, recipes as synth
    cfg = synth.CONFIGS[name]
    if layers is not None:
        cfg = synth.with_layers(cfg, layers, 1)
    model = harness.build_model(cfg, dtype=torch.bfloat16, seed=6, device_rng=name != "tiny", **({} if name == "tiny" else {"max_position": 256}))
    ids = torch.from_numpy(synth.make_prompt(cfg, 100, image_positions=(), seed=9))[None].to(cuda)
    try:
        model.set_option("decode_splitq", splitq)
        model.set_option("decode_rot", 0)
        ia, la = _chained(model, ids, 40)
        ga = model.generate(inputs=ids, do_sample=False, max_new_tokens=40, eos_token_id=-1)
        model.set_option("decode_rot", 1)
        ib, lb = _chained(model, ids, 40)
        gb = model.generate(inputs=ids, do_sample=False, max_new_tokens=40, eos_token_id=-1)
    finally:
        model.set_option("decode_splitq", 1)
        model.set_option("decode_rot", 1)
    assert torch.equal(ia, ib)
    assert torch.equal(la, lb), (la.float() - lb.float()).abs().max().item()
    assert torch.equal(ga, gb)


def test_reloading_a_weight_repacks_its_copy(cuda):
    """load_tensor behind finalize rewrites down_proj, q_proj, k_proj, v_proj, o_proj and lm_head: the rotated copies must follow, or decode_rot = 1 would keep
    decoding with the old model."""
    from synthetic import build as harness, recipes as synth
    cfg = synth.with_layers(synth.CONFIGS["llava15_7b"], 1, 1)
    model = harness.build_model(cfg, dtype=torch.bfloat16, seed=6, device_rng=True, max_position=256)
    ids = torch.from_numpy(synth.make_prompt(cfg, 20, image_positions=(), seed=9))[None].to(cuda)
    shapes = synth.tensor_shapes(cfg)
    gen = torch.Generator(device=cuda); gen.manual_seed(77)
    for n in ("model.layers.0.mlp.down_proj.weight", "model.layers.0.self_attn.q_proj.weight", "model.layers.0.self_attn.k_proj.weight",
              "model.layers.0.self_attn.v_proj.weight", "model.layers.0.self_attn.o_proj.weight", "lm_head.weight"):
        shp = shapes[n]
        model.load_tensor(n, torch.randn(shp, generator=gen, device=cuda) / shp[-1] ** 0.5)
    try:
        on = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
        model.set_option("decode_rot", 0)
        off = model.generate(inputs=ids, do_sample=False, max_new_tokens=8, eos_token_id=-1)
    finally:
        model.set_option("decode_rot", 1)
    assert torch.equal(on, off)
