"""Every attention kernel that reads a K / V^T cache, against caches whose slots past the valid length hold zeros, stale finite values or NaN / Inf
(tests/attn_tails.py).  Those tails are the normal state of the caches: a pooled sequence keeps its earlier request's rows, lmx_seq_truncate keeps the cut
rows, and the training step reuses one scratch pair per length for every sample, layer and step.  For every kernel, geometry and tail state:
  1. the output is finite and within TOL[dt] of a float64 statement over the valid keys only;
  2. the output has the same bits for all three tail states (any read of the tail that changes the result changes the bits);
  3. nothing is written outside the output (sentinel rows / columns of a NaN-filled buffer keep their bytes; log-sum-exp entries past q_len too);
  4. both caches keep every byte, tail included, except the slot a decode launch appends.
Lengths put the boundary at len % 64 in {0, 1, 31, 63} and len % 128 in {0, 127}.  Then the two users of stale tails end to end: the training step on
poisoned scratch pairs, and a shorter request on a sequence recycled from a longer one."""
import gc
import math

import pytest
import torch

import forward_ref as FR
from attn_tails import (DT, TAILS, TOL, Window, _attn_ref, _rel_err, _rope_ref, _rope_table, caches_kept, same_bits, tail_caches)

pytestmark = pytest.mark.gpu


def _gen(cuda, seed):
    return torch.Generator(device=cuda).manual_seed(seed)


def _all_tails_agree(outs, what):
    for tail in TAILS[1:]:
        assert same_bits(outs[tail], outs["zero"]), f"{what}: {tail} tail changes the output (max diff " \
            f"{(outs[tail].float() - outs['zero'].float()).abs().max().item():.3e})"


# ---- prefill attention (flash_prefill2_kernel) ------------------------------------------------------------------------------------------------------------
# nh, nkv, D, q_len, q_pos0, kv_len, s_max, causal
FLASH = [
    (32, 32, 128, 1087, 0, 1087, 1152, True),      # the headline prefill: 1087 % 64 = 63
    (32, 8, 128, 705, 0, 705, 768, True),          # grouped-query: % 64 = 1
    (40, 40, 128, 351, 0, 351, 384, True),         # 13B heads: % 64 = 31
    (8, 8, 128, 384, 0, 384, 512, True),           # % 128 = 0, tail tiles after it
    (8, 8, 128, 100, 155, 255, 384, True),         # chunked, q_len < 128: % 128 = 127
    (8, 8, 128, 1, 512, 513, 640, True),           # chunked, one row: % 64 = 1
    (8, 4, 128, 64, 576, 640, 640, True),          # kv_len == s_max
    (4, 2, 64, 191, 0, 191, 256, True),            # head_dim 64, causal: % 64 = 63, % 128 = 63
    (16, 16, 64, 577, 0, 577, 640, False),         # the vision tower (non-causal)
    (4, 4, 128, 1999, 0, 1999, 2048, True),        # a training sample: s_max = round_up(Tn, 128)
]


@pytest.mark.parametrize("with_lse", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nh,nkv,D,q_len,q_pos0,kv_len,s_max,causal", FLASH)
def test_flash_attn_cache_tails(cuda, dt, with_lse, nh, nkv, D, q_len, q_pos0, kv_len, s_max, causal):
    from llava_mi355x import ops
    T = DT[dt]
    g = _gen(cuda, q_len + kv_len + nh)
    q = torch.randn(q_len, nh, D, device=cuda, generator=g).to(T)
    k = torch.randn(kv_len, nkv, D, device=cuda, generator=g).to(T)
    v = torch.randn(kv_len, nkv, D, device=cuda, generator=g).to(T)
    ref = _attn_ref(q.double(), k.double(), v.double(), causal, q_pos0).reshape(q_len, nh * D)
    if with_lse:                                       # log2-domain log-sum-exp of the scaled scores of every row
        s = torch.einsum("qhd,khd->hqk", q.double(), k.double().repeat_interleave(nh // nkv, dim=1)) / math.sqrt(D)
        if causal:
            s = s.masked_fill(torch.arange(kv_len, device=cuda)[None, :] > torch.arange(q_len, device=cuda)[:, None] + q_pos0, float("-inf"))
        lse_ref = torch.logsumexp(s, dim=-1) / math.log(2.0)
    outs = {}
    for tail in TAILS:
        kc, vt = tail_caches(k, v, s_max, T, tail, seed=kv_len)
        before = (kc.clone(), vt.clone())
        win = Window(q_len, nh * D, T, cuda)
        lwin = Window(nh, q_len + 5, torch.float32, cuda, pad=1, pad_c=0) if with_lse else None      # whole rows: the lse buffer is contiguous
        ops.flash_attn(q.view(q_len, nh * D), kc, vt, q_len, kv_len, q_pos0, nh, nkv, D, causal, out=win.out, lse=lwin.out if with_lse else None)
        torch.cuda.synchronize()
        got = win.out.clone()
        assert torch.isfinite(got.float()).all(), f"{tail} tail: non-finite output"
        err = _rel_err(got, ref)
        assert err < TOL[dt], f"{tail} tail: {err:.3e}"
        assert win.untouched_outside(), f"{tail} tail: a write outside the output"
        assert caches_kept(kc, vt, before), f"{tail} tail: the caches changed"
        if with_lse:
            lse = lwin.out[:, :q_len]
            assert torch.isfinite(lse).all(), f"{tail} tail: non-finite log-sum-exp"
            assert (lse.double() - lse_ref).abs().max().item() <= 2e-3, tail
            assert lwin.untouched_outside() and same_bits(lwin.out[:, q_len:], lwin.before[lwin.sl][:, q_len:]), f"{tail} tail: lse written past q_len"
            got = torch.cat([got.view(-1).float(), lse.reshape(-1)])
        outs[tail] = got
    _all_tails_agree(outs, "flash_attn")


# ---- verification / fp32 attention (decode_attn_kernel + combine) -----------------------------------------------------------------------------------------
# D, nh, nkv, rows, past, causal, n_split, s_max   (keys: past + rows when causal, else past)
DECODE = [
    (128, 4, 4, 1, 1086, True, 1, 1152),           # 1087 keys, one split
    (128, 4, 4, 1, 1086, True, 4, 1152),           # ... four splits: the last one ends at the boundary
    (128, 4, 2, 1, 1023, True, 8, 1088),           # % 64 = 0 (% 128 = 0), eight splits
    (128, 4, 4, 1, 254, True, 8, 384),             # % 128 = 127
    (64, 2, 1, 1, 704, True, 4, 768),              # head_dim 64: % 64 = 1
    (128, 2, 2, 40, 30, True, 1, 128),             # causal multi-row: every row its own boundary (31 .. 70)
    (128, 4, 4, 95, 0, True, 1, 128),              # the fp32 training forward / fp32 prefill: rows 0 .. 94 (% 64 = 31 on the last)
    (64, 4, 4, 33, 577, False, 1, 640),            # the fp32 vision tower: 577 keys, non-causal
]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("D,nh,nkv,rows,past,causal,n_split,s_max", DECODE)
def test_decode_attn_cache_tails(cuda, dt, D, nh, nkv, rows, past, causal, n_split, s_max):
    from llava_mi355x import ops
    T = DT[dt]
    Tk = past + rows if causal else past
    g = _gen(cuda, rows + past + n_split)
    q = torch.randn(rows, nh, D, device=cuda, generator=g).to(T)
    k = torch.randn(Tk, nkv, D, device=cuda, generator=g).to(T)
    v = torch.randn(Tk, nkv, D, device=cuda, generator=g).to(T)
    ref = _attn_ref(q.double(), k.double(), v.double(), causal, past if causal else 0).reshape(rows, nh * D)
    outs = {}
    for tail in TAILS:
        kc, vt = tail_caches(k, v, s_max, T, tail, seed=Tk)
        before = (kc.clone(), vt.clone())
        win = Window(rows, nh * D, T, cuda)
        ops.decode_attn(q.view(rows, nh * D), kc, vt, rows, past if causal else 0, Tk, nh, nkv, D, causal, n_split=n_split, out=win.out)
        torch.cuda.synchronize()
        got = win.out.clone()
        assert torch.isfinite(got.float()).all(), f"{tail} tail: non-finite output"
        err = _rel_err(got, ref)
        assert err < TOL[dt], f"{tail} tail: {err:.3e}"
        assert win.untouched_outside(), f"{tail} tail: a write outside the output"
        assert caches_kept(kc, vt, before), f"{tail} tail: the caches changed"
        outs[tail] = got
    _all_tails_agree(outs, "decode_attn")


# ---- single-token decode steps: RoPE + append at `pos` + attention over keys 0..pos ---------------------------------------------------------------------
STEP_POSITIONS = (0, 63, 127, 128, 1087, 1215, 2047)


def _step_ref(row, k_past, v_past, table, pos, nh, nkv, D, T):
    """float64 statement of one decode step (HF rounding points of RoPE: cos / sin and the rotated q / k in the model dtype)."""
    p1 = torch.tensor([pos], device=row.device)
    tb = table.to(T).double()
    q_r = _rope_ref(row[: nh * D].double().view(1, nh, D), p1, tb, D).to(T)
    k_r = _rope_ref(row[nh * D:(nh + nkv) * D].double().view(1, nkv, D), p1, tb, D).to(T)
    v_n = row[(nh + nkv) * D:].view(1, nkv, D)
    ref = _attn_ref(q_r.double(), torch.cat([k_past, k_r], 0).double(), torch.cat([v_past, v_n], 0).double(), False, 0).reshape(nh * D)
    if T != torch.float32:             # 16-bit: the appended key is HF's chain T(T(x c) + T(r s)), evaluated exactly (float64, itself a value of T)
        return ref, FR.rope_chain(row[nh * D:(nh + nkv) * D].view(1, nkv, D), p1, table, {v: k for k, v in DT.items()}[T])[0][0], v_n[0]
    return ref, k_r[0], v_n[0]


def _key_appended(k_row, k_r, dt):
    """The appended K row: bit-equal to the chain for 16-bit dtypes; float keeps the max-norm."""
    return torch.equal(k_row.double(), k_r) if dt != "f32" else _rel_err(k_row, k_r) < TOL[dt]


def _check_step(cuda, what, dt, nh, nkv, D, pos, s_max, run, row=None):
    """run(qkv_row, kc, vt, table, out_row) launches one decode step writing its output row into out_row.  Checks 1-4 for all tail states, plus the append."""
    T = DT[dt]
    g = _gen(cuda, pos * 3 + nh + D)
    k_past = torch.randn(pos, nkv, D, device=cuda, generator=g).to(T)
    v_past = torch.randn(pos, nkv, D, device=cuda, generator=g).to(T)
    if row is None:
        row = torch.randn((nh + 2 * nkv) * D, device=cuda, generator=g).to(T)
    table = _rope_table(s_max, D).to(cuda)
    ref, k_r, v_n = _step_ref(row, k_past, v_past, table, pos, nh, nkv, D, T)
    outs = {}
    for tail in TAILS:
        kc, vt = tail_caches(k_past, v_past, s_max, T, tail, seed=pos)
        before = (kc.clone(), vt.clone())
        win = Window(1, nh * D, T, cuda)
        run(row.clone(), kc, vt, table, win.row)
        torch.cuda.synchronize()
        got = win.row.clone()
        assert torch.isfinite(got.float()).all(), f"{what}, {tail} tail: non-finite output"
        err = _rel_err(got, ref)
        assert err < TOL[dt], f"{what}, {tail} tail: {err:.3e}"
        assert win.untouched_outside(), f"{what}, {tail} tail: a write outside the output"
        assert caches_kept(kc, vt, before, appended=pos), f"{what}, {tail} tail: a cache slot other than {pos} changed"
        assert _key_appended(kc[:, pos], k_r, dt) and torch.equal(vt[:, :, pos], v_n), f"{what}, {tail} tail: wrong append"
        outs[tail] = got
    _all_tails_agree(outs, what)


def _scratch(nh, D, s_max, out, cuda):
    from llava_mi355x import ops
    ws, cnt, _ = ops.decode_attn_scratch(nh, (s_max + 127) // 128, D, out.dtype, cuda)
    return ws, cnt, out


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nh,nkv,D,pos", [(8, 4, 128, p) for p in STEP_POSITIONS] + [(8, 8, 64, 127), (8, 8, 64, 1087)])
def test_decode_attn_step_cache_tails(cuda, dt, nh, nkv, D, pos):
    from llava_mi355x import ops
    s_max = 2048
    _check_step(cuda, "decode_attn_step", dt, nh, nkv, D, pos, s_max,
                lambda row, kc, vt, tb, out: ops.decode_attn_step(row, kc, vt, tb, pos, nh, nkv, D, scratch=_scratch(nh, D, s_max, out, cuda)))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pos", STEP_POSITIONS)
def test_decode_kv_attn_cache_tails(cuda, dt, pos):
    from llava_mi355x import ops
    nh, nkv, D, K, s_max = 8, 4, 128, 512, 2048
    T = DT[dt]
    g = _gen(cuda, pos + 11)
    w = (torch.randn((nh + 2 * nkv) * D, K, device=cuda, generator=g) / K ** 0.5).to(T)
    nw = (1 + 0.1 * torch.randn(K, device=cuda, generator=g)).to(T)
    x = torch.randn(1, K, device=cuda, generator=g).to(T)
    row = ops.gemv(x, w, norm_w=nw, eps=1e-5)[0]                         # q | k | v (pre-RoPE): the reference's input

    def run(r, kc, vt, tb, out):
        r[nh * D:] = float("nan")                                         # the k | v columns are computed inside the launch, never read
        gran = torch.zeros(2 * nkv * D, dtype=torch.int64, device=cuda)
        ops.decode_kv_attn(r, x[0], w[nh * D:], nw, 1e-5, kc, vt, tb, pos, nh, nkv, D, granules=gran, tag=1, scratch=_scratch(nh, D, s_max, out, cuda))
    _check_step(cuda, "decode_kv_attn", dt, nh, nkv, D, pos, s_max, run, row=row)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pos,s_max", [(p, 2048) for p in STEP_POSITIONS] + [(4095, 4096), (3000, 4096)])
def test_decode_fused_cache_tails(cuda, dt, D, pos, s_max):
    """decode_fused_kernel for one sequence: the fp32 engine's decode step (128-key chunks, 32 of them at s_max 4096, merged by the last to arrive)."""
    from llava_mi355x import ops
    nh, nkv = 8, 4
    pos_word = torch.tensor([pos], dtype=torch.int32, device=cuda)
    _check_step(cuda, "decode_fused", dt, nh, nkv, D, pos, s_max,
                lambda row, kc, vt, tb, out: ops.decode_fused(row, kc, vt, tb, pos_word, nh, nkv, D, scratch=_scratch(nh, D, s_max, out, cuda)))


# ---- the decode batch's chunked form (decode_fused_kernel with a sequence table: head_dim 64, or fp32) -------------------------------------------------
BATCH_POSITIONS = (0, 63, 64, 127, 1087, 1215, 2047, 1, 128, 640)


@pytest.mark.parametrize("dt,D", [("bf16", 64), ("f16", 64), ("f32", 64), ("f32", 128)])
@pytest.mark.parametrize("n_seq,nh,nkv", [(10, 8, 8), (10, 8, 2)])
def test_decode_attn_batch_chunked_cache_tails(cuda, dt, D, n_seq, nh, nkv):
    from llava_mi355x import ops
    T, s_max = DT[dt], 2048
    g = _gen(cuda, n_seq + nh + nkv + D)
    pos = [BATCH_POSITIONS[i % len(BATCH_POSITIONS)] for i in range(n_seq)]
    past = [(torch.randn(p, nkv, D, device=cuda, generator=g).to(T), torch.randn(p, nkv, D, device=cuda, generator=g).to(T)) for p in pos]
    qkv = torch.randn(n_seq, (nh + 2 * nkv) * D, device=cuda, generator=g).to(T)
    table = _rope_table(s_max, D).to(cuda)
    refs = [_step_ref(qkv[z], past[z][0], past[z][1], table, pos[z], nh, nkv, D, T) for z in range(n_seq)]
    words = [torch.tensor([p], dtype=torch.int32, device=cuda) for p in pos]
    outs = {}
    for tail in TAILS:
        caches = [tail_caches(k, v, s_max, T, tail, seed=z) for z, (k, v) in enumerate(past)]
        before = [(kc.clone(), vt.clone()) for kc, vt in caches]
        win = Window(n_seq, nh * D, T, cuda)
        src = qkv.clone()
        ops.decode_attn_batch(src, [c[0] for c in caches], [c[1] for c in caches], words, table, nh, nkv, D, n_split=max(pos) // 128 + 1, out=win.out)
        torch.cuda.synchronize()
        assert torch.equal(src, qkv)
        got = win.out.clone()
        assert win.untouched_outside(), f"{tail} tail: a write outside the output"
        for z in range(n_seq):
            ref, k_r, v_n = refs[z]
            assert torch.isfinite(got[z].float()).all(), f"{tail} tail, sequence {z} (pos {pos[z]}): non-finite output"
            err = _rel_err(got[z], ref)
            assert err < TOL[dt], f"{tail} tail, sequence {z} (pos {pos[z]}): {err:.3e}"
            kc, vt = caches[z]
            assert caches_kept(kc, vt, before[z], appended=pos[z]), f"{tail} tail, sequence {z}: a cache slot other than {pos[z]} changed"
            assert _key_appended(kc[:, pos[z]], k_r, dt) and torch.equal(vt[:, :, pos[z]], v_n), f"{tail} tail, sequence {z}: wrong append"
        outs[tail] = got
    _all_tails_agree(outs, "decode_attn_batch")


# ---- end to end: the training step's scratch pairs, the engine's sequence pool --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_step_ignores_poisoned_kv_scratch(cuda, dtype):
    """TrainStep keeps one K / V^T scratch pair per length, reused by every sample, layer and step.  Filled with NaN / Inf between two steps, it must change
    nothing: loss and every gradient have the same bits as the same two steps of a freshly built TrainStep (the step is bit-reproducible).  The batch's two
    samples are 37 and 30 rows long (22- and 15-token prompts with one 16-row image): their boundaries fall inside a 64-key tile."""
    from oracle import llava_oracle as O
    from synthetic import recipes as synth
    from test_train_step_gpu import build_step, make_batch
    cfg = synth.CONFIGS["tiny"]
    wnp = synth.make_weights(cfg, 0)
    ids, mask, labels, pix = make_batch(cfg)
    with torch.no_grad():
        feats = O.vision_tower(O.to_torch_weights(wnp), cfg, pix)

    def two_steps(poison):
        ts = build_step(cfg, wnp, dtype, cuda)
        ts.forward_backward(ids, labels, mask, image_features=feats)
        torch.cuda.synchronize()
        assert ts._kv_pairs, "the forward made no scratch pair"
        if poison:
            for kc, vt in ts._kv_pairs.values():
                kc.fill_(float("nan"))
                vt.fill_(float("inf"))
                vt[:, :, ::3] = float("nan")
        loss, _ = ts.forward_backward(ids, labels, mask, image_features=feats)
        torch.cuda.synchronize()
        return loss.clone(), {k: g.clone() for k, g in ts.g.items()}

    l_ref, g_ref = two_steps(False)
    l_bad, g_bad = two_steps(True)
    assert torch.isfinite(l_ref) and same_bits(l_bad, l_ref), (l_bad.item(), l_ref.item())
    for k in g_ref:
        assert torch.isfinite(g_bad[k].float()).all(), f"{k}: non-finite gradient"
        assert same_bits(g_bad[k], g_ref[k]), k


def test_pooled_sequence_serves_a_shorter_request_bit_identically(cuda):
    """A request's sequence goes back to the pool when its cache is dropped (lmx_seq_destroy) and the next request takes it (lmx_seq_create) with the earlier
    request's K / V rows still in place.  A shorter request on that sequence must produce the same logits, bit for bit, as on a freshly built model."""
    from synthetic import build as harness, recipes as synth
    cfg = synth.CONFIGS["tiny"]
    wnp = synth.make_weights(cfg, 0)
    dt = torch.bfloat16
    model = harness.build_model(cfg, dtype=dt, seed=0, weights=wnp)
    fresh = harness.build_model(cfg, dtype=dt, seed=0, weights=wnp)
    pix = torch.from_numpy(synth.make_pixels(cfg, 1, seed=3)).to(cuda, dt)

    def request(m, n_prompt, n_new, seed):
        ids = torch.from_numpy(synth.make_prompt(cfg, n_prompt, image_positions=(5,), seed=seed))[None].to(cuda)
        out = m.forward(input_ids=ids, images=pix, use_cache=True)
        cache, logits = out.past_key_values, [out.logits[0, -1].clone()]
        for _ in range(n_new):
            tok = logits[-1].argmax().view(1, 1)
            out = m.forward(input_ids=tok, past_key_values=cache, use_cache=True)
            logits.append(out.logits[0, -1].clone())
        torch.cuda.synchronize()
        return cache, torch.stack(logits)

    long_cache, _ = request(model, 200, 24, seed=2)                     # 215 prompt rows + 24 steps: fills most of the 256-slot cache
    recycled = long_cache.seqs[0].value
    del long_cache
    gc.collect()
    short_cache, got = request(model, 40, 8, seed=4)
    assert short_cache.seqs[0].value == recycled, "the shorter request did not take the pooled sequence"
    _, want = request(fresh, 40, 8, seed=4)
    assert torch.isfinite(got).all()
    assert same_bits(got, want), (got - want).abs().max().item()
    short_cache.close()
