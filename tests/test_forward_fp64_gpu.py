"""RoPE with the KV append, RMSNorm, LayerNorm and the attention family, each HIP kernel against the float64 statements of forward_ref.py, element by element:
bit equality where the arithmetic is exact (RoPE and the appended key rows of 16-bit models, the V^T columns, RMSNorm outside its flippable set), the DERIVED
bounds elsewhere.  The bounds are proven on the CPU by test_forward_ref_host.py (honest emulations inside, mutants outside) on the very inputs used here — they
are drawn on the CPU with fixed seeds by forward_ref.py.  Every test prints its worst err / bound (`pytest -s`).

All calls go through the C ABI (`lmx_op_*`).  Not reached at op level, so not covered: launch_attn_probs and the strided (ldx != H) norm launches."""
import pytest
import torch

import forward_ref as F
from forward_ref import DT
from test_ops_gpu import _fill_cache

pytestmark = pytest.mark.gpu


def _to(cuda, *ts):
    return [t.to(cuda) for t in ts]


# ---- RoPE + KV append ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.ROPE_DTYPES)
@pytest.mark.parametrize("k_rows", [False, True])
@pytest.mark.parametrize("D,nh,nkv", F.ROPE_GEOMS)
def test_rope_kv_is_the_exact_chain(cuda, dt, k_rows, D, nh, nkv):
    """q in place, the K-cache rows and (k_rows) the k columns of the row: HF's chain T(T(x c) + T(r s)), bit for bit for bf16 / f16, within the three fp32
    roundings for float; V^T columns exact; nothing outside the window [pos0, pos0 + T) touched.  T in {1, 63, 64, 65, 150}: the grid is ceil(T / 64)."""
    from llava_mi355x import ops
    s_max = F.ROPE_S_MAX
    table = F.rope_table(s_max, D).to(cuda)
    worst = 0.0
    for T in F.ROPE_T:
        src = F.rope_inputs(D, nh, nkv, T, dt).to(cuda)
        for pos0 in F.rope_pos0(T):
            what = f"T {T} pos0 {pos0}"
            qkv = src.clone()
            k, vt = ops.alloc_kv(nkv, s_max, D, DT[dt])
            ops.rope_kv(qkv, k, vt, table, pos0, nh, nkv, D, k_rows=k_rows)
            pos = torch.arange(pos0, pos0 + T, device=cuda)
            worst = max(worst, F.rope_check(qkv[:, : nh * D].view(T, nh, D), src[:, : nh * D].view(T, nh, D), pos, table, dt, what + " q"))
            k_src = src[:, nh * D:(nh + nkv) * D].view(T, nkv, D)
            worst = max(worst, F.rope_check(k[:, pos0:pos0 + T].permute(1, 0, 2), k_src, pos, table, dt, what + " K cache"))
            if k_rows:
                assert torch.equal(qkv[:, nh * D:(nh + nkv) * D].view(T, nkv, D), k[:, pos0:pos0 + T].permute(1, 0, 2)), what + ": k columns != K cache rows"
            else:
                assert torch.equal(qkv[:, nh * D:(nh + nkv) * D], src[:, nh * D:(nh + nkv) * D]), what + ": k columns changed"
            assert torch.equal(qkv[:, (nh + nkv) * D:], src[:, (nh + nkv) * D:]), what + ": v columns changed"
            assert torch.equal(vt[:, :, pos0:pos0 + T].permute(2, 0, 1), src[:, (nh + nkv) * D:].view(T, nkv, D)), what + ": V^T columns"
            assert k[:, :pos0].abs().sum() == 0 and k[:, pos0 + T:].abs().sum() == 0, what + ": K cache outside the window"
            assert vt[:, :, :pos0].abs().sum() == 0 and vt[:, :, pos0 + T:].abs().sum() == 0, what + ": V^T outside the window"
    print(f"rope_kv {dt}: worst err / bound {worst:.3f}")


# ---- norms --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("H", F.RMS_H)
def test_rmsnorm_is_the_rounding_chain(cuda, dt, H):
    """round_T(round_T(x inv) w): equality outside norm_chain's flippable set (at most 1 % of a row, asserted), one ulp of the first rounding inside it; float:
    the derived bound.  H walks rmsnorm_reg_kernel<T, 1 .. 4>, rows that leave threads idle, and rmsnorm_kernel; rows incl. the offset and the constant row."""
    from llava_mi355x import ops
    for rows in F.NORM_ROWS:
        x, w, _ = _to(cuda, *F.norm_inputs(rows, H, dt))
        r, frac = F.rmsnorm_check(ops.rmsnorm(x, w, F.NORM_EPS), x, w, dt, what=f"rmsnorm {rows + 2} x {H} {dt}")
        print(f"rmsnorm {rows + 2} x {H} {dt}: {'worst err / bound' if dt == 'f32' else 'share off the chain'} {r:.4f}, flippable share {frac:.4f}")


@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("H", F.LN_H)
def test_layernorm_two_pass_chain(cuda, dt, H):
    """The two-pass, fp32-statistics chain with one final rounding, inside ulp_T(ref) + the derived fp32 term.  H walks layernorm_wave_kernel<T, 1 | 2 | 4> and the
    generic kernel; 5 + 2 rows leave the wave kernel's last workgroup three idle waves."""
    from llava_mi355x import ops
    for rows in F.NORM_ROWS:
        x, w, b = _to(cuda, *F.norm_inputs(rows, H, dt))
        r = F.layernorm_check(ops.layernorm(x, w, b, F.NORM_EPS), x, w, b, dt, what=f"layernorm {rows + 2} x {H} {dt}")
        print(f"layernorm {rows + 2} x {H} {dt}: worst err / bound {r:.3f}")


# ---- prefill ------------------------------------------------------------------------------------------------------------------------------------------------------
def _prefill(cuda, dt, q, k, v, causal, past, what):
    from llava_mi355x import ops
    Tq, nh, D = q.shape
    Tk, nkv, _ = k.shape
    q, k, v = _to(cuda, q, k, v)
    kc, vt = _fill_cache(k, v, ((Tk + 63) // 64) * 64 + 64, DT[dt], cuda)
    R = F.AttnRef(q, k, v, causal, past)
    E = R.prefill_bound(dt)
    got = ops.flash_attn(q.view(Tq, nh * D), kc, vt, Tq, Tk, past, nh, nkv, D, causal)
    r_out = F.check(got.view(Tq, nh, D), R.ref, E, dt, what)
    lse = torch.full((nh, Tq), float("nan"), dtype=torch.float32, device=cuda)
    got2 = ops.flash_attn(q.view(Tq, nh * D), kc, vt, Tq, Tk, past, nh, nkv, D, causal, lse=lse)
    r_out = max(r_out, F.check(got2.view(Tq, nh, D), R.ref, E, dt, what + " (lse requested)"))
    r_lse = F.check(lse, R.lse2, R.lse_bound(), "f32", what + " lse")
    print(f"{what}: worst err / bound {r_out:.3f}, lse {r_lse:.3f}")


@pytest.mark.parametrize("dt", F.PREFILL_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("D,nh,nkv,Tq,past,causal", F.PREFILL_CASES)
def test_flash_prefill_per_element(cuda, dt, flat, D, nh, nkv, Tq, past, causal):
    """flash_prefill2_kernel: |got - round_T(ref)| <= 2 u_T sum_j p_ij |v_jd| + ulp_T(ref) at every element, with and without the lse output, and the lse inside
    its derived bound (it replaces a flat 2e-3): f16, head_dim 64, GQA, past > 0, the non-causal 577-row form of the vision tower, one query row."""
    q, k, v = F.attn_inputs(D, nh, nkv, Tq, past + Tq, dt, Tq + D, flat)
    _prefill(cuda, dt, q, k, v, causal, past, f"prefill {dt} D {D} {nh}/{nkv} heads Tq {Tq} past {past} causal {causal} flat {flat}")


@pytest.mark.parametrize("dt", F.PREFILL_DTYPES)
def test_flash_prefill_forced_rescale_per_element(cuda, dt):
    q, k, v = F.forced_rescale_inputs(dt)
    _prefill(cuda, dt, q, k, v, True, 0, f"prefill {dt} forced rescale")


# ---- decode: P kept in fp32 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("D,nh,nkv,rows,past,causal,n_split", F.DECODE_CASES)
def test_decode_attn_per_element(cuda, dt, flat, D, nh, nkv, rows, past, causal, n_split):
    from llava_mi355x import ops
    Tk = past + rows if causal else F.DECODE_NONCAUSAL_KEYS
    q, k, v = _to(cuda, *F.attn_inputs(D, nh, nkv, rows, Tk, dt, rows + past, flat))
    kc, vt = _fill_cache(k, v, ((Tk + 63) // 64) * 64 + 64, DT[dt], cuda)
    got = ops.decode_attn(q.view(rows, nh * D), kc, vt, rows, past, Tk, nh, nkv, D, causal, n_split=n_split)
    R = F.AttnRef(q, k, v, causal, past)
    r = F.check(got.view(rows, nh, D), R.ref, R.decode_attn_bound(n_split), dt, "decode_attn")
    print(f"decode_attn {dt} D {D} rows {rows} past {past} n_split {n_split} flat {flat}: worst err / bound {r:.3f}")


def _step(cuda, dt, nh, nkv, D, pos, flat, run, what):
    """One decode step: output inside the derived bound, the appended K row bit-equal to the chain (float: inside the rope bound), V^T exact, no other slot moved."""
    s_max = F.STEP_S_MAX
    table = F.rope_table(s_max, D).to(cuda)
    row, k_past, v_past = _to(cuda, *F.step_inputs(nh, nkv, D, pos, dt, flat=flat))
    kc, vt = _fill_cache(k_past, v_past, s_max, DT[dt], cuda)
    before = (kc.clone(), vt.clone())
    out = run(row.clone(), kc, vt, table)
    R, k_new, kE, v_new = F.step_ref(row, k_past, v_past, table, pos, nh, nkv, D, dt)
    r = F.check(out.view(1, nh, D), R.ref, R.step_bound(pos // 128 + 1), dt, what)
    ra = F.append_check(kc[:, pos], k_new, kE, dt, what + ": appended key")
    assert torch.equal(vt[:, :, pos], v_new), what + ": appended value"
    keep = torch.ones(s_max, dtype=torch.bool, device=cuda); keep[pos] = False
    assert torch.equal(kc[:, keep], before[0][:, keep]) and torch.equal(vt[:, :, keep], before[1][:, :, keep]), what + ": a cache slot other than pos changed"
    print(f"{what}: worst err / bound {r:.3f}, appended key {ra:.3f}")


@pytest.mark.parametrize("dt", F.PREFILL_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("nh,nkv,D", F.STEP_GEOMS)
@pytest.mark.parametrize("pos", F.STEP_POS)
def test_decode_attn_step_per_element(cuda, dt, flat, nh, nkv, D, pos):
    from llava_mi355x import ops
    _step(cuda, dt, nh, nkv, D, pos, flat, lambda row, kc, vt, tb: ops.decode_attn_step(row, kc, vt, tb, pos, nh, nkv, D),
          f"decode_attn_step {dt} {nh}/{nkv} x {D} pos {pos} flat {flat}")


@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("nh,nkv,D", F.STEP_GEOMS)
@pytest.mark.parametrize("pos", F.STEP_POS)
def test_decode_fused_per_element(cuda, dt, flat, nh, nkv, D, pos):
    from llava_mi355x import ops
    _step(cuda, dt, nh, nkv, D, pos, flat, lambda row, kc, vt, tb: ops.decode_fused(row, kc, vt, tb, pos, nh, nkv, D),
          f"decode_fused {dt} {nh}/{nkv} x {D} pos {pos} flat {flat}")


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("f16", 128), ("f32", 128), ("bf16", 64)])
def test_decode_attn_batch_per_element(cuda, dt, D):
    """The batched decode attention on test_decode_batch_attn_gpu's own sequences at its smallest batch (4 sequences, 32 heads over 8 kv heads, positions mixed
    over piece / chunk boundaries): decode_attn_wave_kernel for 16-bit head_dim 128, the chunked decode_fused_kernel with a sequence table otherwise."""
    from llava_mi355x import ops
    from test_decode_batch_attn_gpu import _build
    n_seq, nh, nkv, s_max = 4, 32, 8, 2048
    table = F.rope_table(s_max, D).to(cuda)
    pos, qkv, seqs = _build(cuda, DT[dt], n_seq, nh, nkv, D, s_max, "zero", n_seq + nh)
    n_split = max(pos) // 128 + 1
    out = ops.decode_attn_batch(qkv.clone(), [s[2] for s in seqs], [s[3] for s in seqs], [s[4] for s in seqs], table, nh, nkv, D, n_split=n_split)
    wave = D == 128 and dt != "f32"
    worst = 0.0
    for z, (k_past, v_past, kc, vt, _) in enumerate(seqs):
        what = f"sequence {z} (pos {pos[z]})"
        R, k_new, kE, v_new = F.step_ref(qkv[z], k_past, v_past, table, pos[z], nh, nkv, D, dt)
        worst = max(worst, F.check(out[z].view(1, nh, D), R.ref, R.batch_wave_bound() if wave else R.step_bound(n_split), dt, what))
        F.append_check(kc[:, pos[z]], k_new, kE, dt, what + ": appended key")
        assert torch.equal(vt[:, :, pos[z]], v_new), what + ": appended value"
    print(f"decode_attn_batch {dt} D {D} ({'wave' if wave else 'chunked'} form): worst err / bound {worst:.3f}")
